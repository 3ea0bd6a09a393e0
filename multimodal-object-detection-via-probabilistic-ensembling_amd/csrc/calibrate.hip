// Temperature calibration of the detectors' class posteriors (gfx950).
//   pe_calibrated_softmax   : p = softmax(logits / T) in float64 over a flat [M, K+1] tensor (all K+1 columns stored)
//   pe_log_softmax          : the same with log p_k = z_k - m - log(sum_j e_j) stored
//   pe_temperature_nll      : sum_i -log softmax(logits_i / T)[label_i] and d/d(log T), for up to 64 candidate T in one launch
// The row arithmetic is csrc/softmax_row.h, shared with the pack kernel (csrc/pack.hip: pe_proben_pack_logits,
// pe_proben_pack_log_posteriors), so a row gets the same bits from either.  Built with -ffp-contract=off like the other ProbEn code.
#include "common.h"
#include "softmax_row.h"
#include "sweep.h"

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

// the model of pe::sweep (csrc/sweep.h): an item is a row, a candidate a temperature, the sums are the NLL and d NLL / d(log T).  The 64
// lanes read the same logits (one cache line, broadcast).  The candidates stay in the kernel arguments: the workspace is all partials.
struct NllModel {
    static constexpr int kMaxValues = 2;
    using Shared = pe::NoShared;
    struct Lane { double T; };
    const float* logits;
    const int32_t* labels;
    long long items;     // = M
    int k1, nc;
    double T[64];
    double* partial;     // [blocks, nc, 2], added up by pe::launch_finish (csrc/reduce2.h)
    int32_t* flags;      // pe::flag_excluded: rows with a label outside [0, K]

    __host__ __device__ __forceinline__ int values() const { return 2; }
    __device__ __forceinline__ void setup(Shared&) const {}
    __device__ __forceinline__ void load(Lane& L, int c, Shared&) const { L.T = T[c]; }
    __device__ __forceinline__ bool item(const Lane& L, double (&acc)[kMaxValues], long long r, Shared&) const {
        const int y = labels[r];
        if (y < 0 || y >= k1) return false;
        const float* row = logits + r * k1;
        double m = pe::kNegInf;
        for (int k = 0; k < k1; ++k) {
            const double z = (double)row[k] / L.T;
            m = (z > m || z != z) ? z : m;
        }
        double s = 0.0, sz = 0.0;
        for (int k = 0; k < k1; ++k) {
            const double z = (double)row[k] / L.T;
            const double e = exp(z - m);
            s += e;
            sz += e * (z - m);
        }
        const double zy = (double)row[y] / L.T - m;
        acc[0] += log(s) - zy;           // -log softmax(z)[y]
        acc[1] += zy - sz / s;           // d/d(log T): z_y - sum_k p_k z_k (the shift by m cancels)
        return true;
    }
};

__global__ __launch_bounds__(pe::kSweepThreads) void temperature_nll_kernel(NllModel m) { pe::sweep(m); }

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
    NllModel m{};
    m.logits = logits; m.labels = labels; m.items = num_rows; m.k1 = num_columns; m.nc = num_temperatures;
    for (int t = 0; t < num_temperatures; ++t) m.T[t] = temperatures_host[t];
    m.partial = workspace; m.flags = out_flags;
    return pe::launch_sweep(temperature_nll_kernel, m, PE_TEMPERATURE_NLL_MAX_BLOCKS, out, (hipStream_t)stream, "pe_temperature_nll");
}
