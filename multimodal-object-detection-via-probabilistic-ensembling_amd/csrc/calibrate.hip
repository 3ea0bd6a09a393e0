// Temperature calibration of the detectors' class posteriors (gfx950).
//   pe_calibrated_softmax   : p = softmax(logits / T) in float64 over a flat [M, K+1] tensor (all K+1 columns stored)
//   pe_log_softmax          : the same with log p_k = z_k - m - log(sum_j e_j) stored
//   pe_temperature_nll      : sum_i -log softmax(logits_i / T)[label_i] and d/d(log T), for up to 64 candidate T in one launch
// The row arithmetic is csrc/softmax_row.h, shared with the pack kernel (csrc/pack.hip: pe_proben_pack_logits,
// pe_proben_pack_log_posteriors), so a row gets the same bits from either.  Built with -ffp-contract=off like the other ProbEn code.
#include "common.h"
#include "reduce2.h"
#include "softmax_row.h"

namespace {

// flat [M, k1] -> [M, k1]; 256 threads, grid-stride over row groups.  LOGP (pe_log_softmax): out = log p.
template <bool LOGP>
__global__ __launch_bounds__(256) void calibrated_softmax_kernel(const float* logits, long long M, int k1, double T, double* out) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (long long)gridDim.x * 4;
    if (k1 <= 64) {
        const int G = pe::group_width(k1), rpp = 64 / G, col = lane & (G - 1);
        for (long long r0 = wave * rpp; r0 < M; r0 += waves * rpp) {      // wave-uniform
            const long long r = r0 + lane / G;
            const bool live = r < M;
            double lp = 0.0;
            const double p = pe::softmax_group<LOGP>(logits + r * k1, live, col, k1, G, T, &lp);
            if (live && col < k1) out[r * k1 + col] = LOGP ? lp : p;
        }
    } else if (LOGP) {
        for (long long r = wave * 64 + lane; r < M; r += waves * 64) pe::softmax_serial(logits + r * k1, k1, T, nullptr, 0, -1, out + r * k1);
    } else {
        for (long long r = wave * 64 + lane; r < M; r += waves * 64) pe::softmax_serial(logits + r * k1, k1, T, out + r * k1, k1, -1);
    }
}

constexpr int kNllThreads = 256, kNllWaves = kNllThreads / 64;

struct NllArgs {
    const float* logits;
    const int32_t* labels;
    long long M;
    int k1, n_t;
    double T[64];
    double* partial;     // [blocks, n_t, 2], added up by pe::launch_finish (csrc/reduce2.h)
    int32_t* flags;      // pe::flag_excluded: rows with a label outside [0, K]
};

// Lane = candidate temperature, wavefront = row: the 64 lanes read the same logits (one cache line, broadcast) and each keeps its own
// two sums.  Wave w of block g takes rows g * kNllWaves + w, + gridDim.x * kNllWaves, ...: a fixed order for a fixed (M, grid).
__global__ __launch_bounds__(kNllThreads) void temperature_nll_kernel(NllArgs a) {
    __shared__ double part[kNllWaves][64][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double T = a.T[lane < a.n_t ? lane : 0];
    double nll = 0.0, dnll = 0.0;
    const long long step = (long long)gridDim.x * kNllWaves;
    for (long long r = (long long)blockIdx.x * kNllWaves + w; r < a.M; r += step) {
        const int y = a.labels[r];
        if (y < 0 || y >= a.k1) {
            if (lane == 0) pe::flag_excluded(a.flags, r);
            continue;
        }
        const float* row = a.logits + r * a.k1;
        double m = pe::kNegInf;
        for (int k = 0; k < a.k1; ++k) {
            const double z = (double)row[k] / T;
            m = (z > m || z != z) ? z : m;
        }
        double s = 0.0, sz = 0.0;
        for (int k = 0; k < a.k1; ++k) {
            const double z = (double)row[k] / T;
            const double e = exp(z - m);
            s += e;
            sz += e * (z - m);
        }
        const double zy = (double)row[y] / T - m;
        nll += log(s) - zy;           // -log softmax(z)[y]
        dnll += zy - sz / s;          // d/d(log T): z_y - sum_k p_k z_k (the shift by m cancels)
    }
    part[w][lane][0] = nll;
    part[w][lane][1] = dnll;
    __syncthreads();
    if (threadIdx.x < a.n_t) {
        double s0 = part[0][lane][0], s1 = part[0][lane][1];
        for (int v = 1; v < kNllWaves; ++v) { s0 += part[v][lane][0]; s1 += part[v][lane][1]; }
        double* o = a.partial + ((size_t)blockIdx.x * a.n_t + lane) * 2;
        o[0] = s0;
        o[1] = s1;
    }
}

int flat_softmax_impl(const char* what, const float* logits, int64_t num_rows, int32_t num_columns, double temperature, double* out,
                      bool logp, void* stream) {
    PE_CHECK_ARG(pe::finite_positive(temperature), "%s: temperature %g is not finite and > 0", what, temperature);
    PE_CHECK_ARG(num_rows >= 0, "%s: num_rows %lld", what, (long long)num_rows);
    PE_CHECK_ARG(num_columns >= 2, "%s: num_columns %d (K + 1) < 2", what, num_columns);
    if (num_rows == 0) return PE_OK;
    PE_CHECK_ARG(logits && out, "%s: null pointer", what);
    const int rows_per_wave = num_columns <= 64 ? 64 / pe::group_width(num_columns) : 64;
    const long long waves = (num_rows + rows_per_wave - 1) / rows_per_wave;
    const int blocks = (int)std::min<long long>((waves + 3) / 4, 4096);
    if (logp)
        hipLaunchKernelGGL(calibrated_softmax_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, (long long)num_rows,
                           (int)num_columns, temperature, out);
    else
        hipLaunchKernelGGL(calibrated_softmax_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, (long long)num_rows,
                           (int)num_columns, temperature, out);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}

}  // namespace

extern "C" int pe_calibrated_softmax(const float* logits, int64_t num_rows, int32_t num_columns, double temperature,
                                     double* out_probs, void* stream) {
    return flat_softmax_impl("pe_calibrated_softmax", logits, num_rows, num_columns, temperature, out_probs, false, stream);
}

extern "C" int pe_log_softmax(const float* logits, int64_t num_rows, int32_t num_columns, double temperature, double* out_log_probs,
                              void* stream) {
    return flat_softmax_impl("pe_log_softmax", logits, num_rows, num_columns, temperature, out_log_probs, true, stream);
}

extern "C" int pe_temperature_nll(const float* logits, const int32_t* labels, int64_t num_rows, int32_t num_columns,
                                  const double* temperatures_host, int32_t num_temperatures, double* workspace,
                                  double* out, int32_t* out_flags, void* stream) {
    PE_CHECK_ARG(num_temperatures >= 1 && num_temperatures <= 64, "pe_temperature_nll: num_temperatures %d not in [1,64]",
                 num_temperatures);
    PE_CHECK_ARG(temperatures_host, "pe_temperature_nll: null pointer (temperatures)");
    for (int t = 0; t < num_temperatures; ++t)
        PE_CHECK_ARG(pe::finite_positive(temperatures_host[t]), "pe_temperature_nll: temperature %g (candidate %d) is not finite and > 0",
                     temperatures_host[t], t);
    PE_CHECK_ARG(num_rows >= 0, "pe_temperature_nll: num_rows %lld", (long long)num_rows);
    PE_CHECK_ARG(num_columns >= 2, "pe_temperature_nll: num_columns %d (K + 1) < 2", num_columns);
    PE_CHECK_ARG(workspace && out && out_flags, "pe_temperature_nll: null pointer (workspace / out / out_flags)");
    PE_CHECK_ARG(num_rows == 0 || (logits && labels), "pe_temperature_nll: null pointer (logits / labels)");
    NllArgs a{};
    a.logits = logits; a.labels = labels; a.M = num_rows; a.k1 = num_columns; a.n_t = num_temperatures;
    for (int t = 0; t < num_temperatures; ++t) a.T[t] = temperatures_host[t];
    a.partial = workspace; a.flags = out_flags;
    // the grid is a function of num_rows alone: same input, same partition, same bits
    const int blocks = (int)std::max<long long>(1, std::min<long long>((num_rows + kNllWaves - 1) / kNllWaves,
                                                                        PE_TEMPERATURE_NLL_MAX_BLOCKS));
    if (int st = pe::zero_flags(out_flags, (hipStream_t)stream, "pe_temperature_nll")) return st;
    hipLaunchKernelGGL(temperature_nll_kernel, dim3(blocks), dim3(kNllThreads), 0, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH("pe_temperature_nll");
    return pe::launch_finish(workspace, blocks, 2 * num_temperatures, 0, nullptr, out, (hipStream_t)stream, "pe_temperature_nll");
}
