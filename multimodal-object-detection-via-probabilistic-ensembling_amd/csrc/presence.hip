// Presence evidence of log-posterior ProbEn (gfx950): the fit's objective.
//   pe_bias_nll : sum over clusters of -log softmax(base_c + b)[y_c] and its gradient in b, for up to 64 candidate rows b in one launch
// One row of the presence table is a bias-only softmax regression over the clusters of its pattern: base = the fused log-posterior at a
// zero table, b = the row.  Layout as pe_temperature_nll / pe_pool_nll: lane = candidate, wavefront = cluster.  A cluster is K + 1 <= 16
// doubles that every lane reads from the same address (a broadcast); a lane keeps its candidate and its 1 + (K + 1) accumulators in
// registers, so every loop over the columns is unrolled to PE_BIAS_NLL_MAX_COLUMNS and predicated.  Per cluster, in column order:
//   a_j = base_j + b_j,  top = max_j a_j,  e_j = exp(a_j - top),  tot = sum_j e_j,
//   nll += log(tot) - (a_y - top),  grad_j += e_j / tot - [y = j].
// Built with -ffp-contract=off like the other ProbEn code.
#include "common.h"
#include "reduce2.h"

namespace {

constexpr int kBiasThreads = 256, kBiasWaves = kBiasThreads / 64;
constexpr int kMaxCols = PE_BIAS_NLL_MAX_COLUMNS;

struct BiasArgs {
    const double* base;         // [C, k1]
    const int32_t* labels;      // [C]
    const double* cand;         // [nc, k1] (the head of the workspace)
    int C, k1, nc;
    double* partial;            // [blocks, nc, 1 + k1], added up by pe::launch_finish (csrc/reduce2.h)
    int32_t* flags;             // pe::flag_excluded: excluded clusters
};

// the candidates travel as kernel arguments, 256 doubles a launch, into the head of the workspace: stream-ordered, and the host
// array is free again when pe_bias_nll returns
struct StageArgs {
    double v[256];
    double* dst;
    int n;
};

__global__ __launch_bounds__(256) void bias_stage_kernel(StageArgs a) {
    if ((int)threadIdx.x < a.n) a.dst[threadIdx.x] = a.v[threadIdx.x];
}

// Wave w of block g takes clusters g * kBiasWaves + w, + gridDim.x * kBiasWaves, ...: a fixed order for a fixed (C, grid).
__global__ __launch_bounds__(kBiasThreads) void bias_nll_kernel(BiasArgs a) {
    __shared__ double part[kBiasWaves][1 + kMaxCols][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k1 = a.k1;
    double b[kMaxCols], grad[kMaxCols], nll = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxCols; ++j) {
        b[j] = j < k1 ? a.cand[(size_t)(lane < a.nc ? lane : 0) * k1 + j] : 0.0;
        grad[j] = 0.0;
    }
    const int step = gridDim.x * kBiasWaves;
    for (int c = blockIdx.x * kBiasWaves + wv; c < a.C; c += step) {              // wave-uniform
        const int y = a.labels[c];
        const double* row = a.base + (size_t)c * k1;
        double x[kMaxCols];
        bool bad = y < 0 || y >= k1;
#pragma unroll
        for (int j = 0; j < kMaxCols; ++j) {
            x[j] = j < k1 ? row[j] : 0.0;                                         // every lane the same address
            bad = bad || !(fabs(x[j]) < __builtin_huge_val());                    // NaN or infinite
        }
        if (bad) {
            if (lane == 0) pe::flag_excluded(a.flags, c);
            continue;
        }
        double top = 0.0, ay = 0.0;
#pragma unroll
        for (int j = 0; j < kMaxCols; ++j) {
            if (j < k1) {
                x[j] = x[j] + b[j];
                top = (j == 0 || x[j] > top) ? x[j] : top;
                ay = j == y ? x[j] : ay;
            }
        }
        double tot = 0.0;
#pragma unroll
        for (int j = 0; j < kMaxCols; ++j) {
            if (j < k1) {
                x[j] = exp(x[j] - top);
                tot += x[j];
            }
        }
        nll += log(tot) - (ay - top);
#pragma unroll
        for (int j = 0; j < kMaxCols; ++j)
            if (j < k1) grad[j] += x[j] / tot - (j == y ? 1.0 : 0.0);
    }
    part[wv][0][lane] = nll;
#pragma unroll
    for (int j = 0; j < kMaxCols; ++j) part[wv][1 + j][lane] = grad[j];
    __syncthreads();
    // thread (v, lane): value v of candidate lane, the block's waves in wave order
    for (int v = wv; v < 1 + k1; v += kBiasWaves) {
        if (lane < a.nc) {
            double s = part[0][v][lane];
            for (int u = 1; u < kBiasWaves; ++u) s += part[u][v][lane];
            a.partial[((size_t)blockIdx.x * a.nc + lane) * (1 + k1) + v] = s;
        }
    }
}

}  // namespace

extern "C" int pe_bias_nll(const double* base, const int32_t* labels, int32_t num_clusters, int32_t num_columns,
                           const double* candidates_host, int32_t num_candidates, double* workspace, double* out, int32_t* out_flags,
                           void* stream) {
    const char* what = "pe_bias_nll";
    PE_CHECK_ARG(num_candidates >= 1 && num_candidates <= 64, "%s: num_candidates %d not in [1,64]", what, num_candidates);
    PE_CHECK_ARG(num_columns >= 2, "%s: num_columns %d (K + 1) < 2", what, num_columns);
    if (num_columns > PE_BIAS_NLL_MAX_COLUMNS) {
        pe::set_error("%s: num_columns %d (K + 1) above %d: a lane keeps its candidate and 1 + (K + 1) accumulators in registers (the fusion "
                      "itself takes K <= 62; the fit does not)", what, num_columns, PE_BIAS_NLL_MAX_COLUMNS);
        return PE_ERR_UNSUPPORTED;
    }
    PE_CHECK_ARG(candidates_host, "%s: null pointer (candidates)", what);
    for (int i = 0; i < num_candidates * num_columns; ++i) {
        const double x = candidates_host[i];
        PE_CHECK_ARG(x == x && x > -__builtin_huge_val() && x < __builtin_huge_val(), "%s: candidate entry %g (candidate %d, column %d) is not finite",
                     what, x, i / num_columns, i % num_columns);
    }
    PE_CHECK_ARG(num_clusters >= 0, "%s: num_clusters %d < 0", what, num_clusters);
    PE_CHECK_ARG(workspace && out && out_flags, "%s: null pointer (workspace / out / out_flags)", what);
    PE_CHECK_ARG(num_clusters == 0 || (base && labels), "%s: null pointer (base / labels)", what);
    hipStream_t st = (hipStream_t)stream;
    const int nw = num_candidates * num_columns, nv = num_candidates * (1 + num_columns);
    if (int rc = pe::zero_flags(out_flags, st, what)) return rc;
    if (num_clusters == 0) {        // nothing to add up: zeros, no launch
        if (hipMemsetAsync(out, 0, (size_t)nv * sizeof(double), st) != hipSuccess) {
            pe::set_error("%s: hipMemsetAsync of the result failed", what);
            return PE_ERR_HIP;
        }
        return PE_OK;
    }
    for (int o = 0; o < nw; o += 256) {
        StageArgs s{};
        s.n = std::min(256, nw - o);
        s.dst = workspace + o;
        for (int i = 0; i < s.n; ++i) s.v[i] = candidates_host[o + i];
        hipLaunchKernelGGL(bias_stage_kernel, dim3(1), dim3(256), 0, st, s);
        PE_CHECK_LAUNCH("pe_bias_nll (candidates)");
    }
    BiasArgs a{};
    a.base = base; a.labels = labels; a.cand = workspace; a.C = num_clusters; a.k1 = num_columns; a.nc = num_candidates;
    a.partial = workspace + nw; a.flags = out_flags;
    // the grid is a function of num_clusters alone: same input, same partition, same bits
    const int blocks = std::min((num_clusters + kBiasWaves - 1) / kBiasWaves, PE_BIAS_NLL_MAX_BLOCKS);
    hipLaunchKernelGGL(bias_nll_kernel, dim3(blocks), dim3(kBiasThreads), 0, st, a);
    PE_CHECK_LAUNCH(what);
    return pe::launch_finish(a.partial, blocks, nv, 0, nullptr, out, st, what);
}
