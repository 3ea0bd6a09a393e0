// Presence evidence of log-posterior ProbEn (gfx950): the fit's objective.
//   pe_bias_nll : sum over clusters of -log softmax(base_c + b)[y_c] and its gradient in b, for up to 64 candidate rows b in one launch
// One row of the presence table is a bias-only softmax regression over the clusters of its pattern: base = the fused log-posterior at a
// zero table, b = the row.  The candidate sweep of csrc/sweep.h: lane = candidate, wavefront = cluster.  A cluster is K + 1 <= 16
// doubles that every lane reads from the same address (a broadcast); a lane keeps its candidate and its 1 + (K + 1) accumulators in
// registers, so every loop over the columns is unrolled to PE_BIAS_NLL_MAX_COLUMNS and predicated.  Per cluster, in column order:
//   a_j = base_j + b_j,  top = max_j a_j,  e_j = exp(a_j - top),  tot = sum_j e_j,
//   nll += log(tot) - (a_y - top),  grad_j += e_j / tot - [y = j].
// Built with -ffp-contract=off like the other ProbEn code.
#include "common.h"
#include "sweep.h"

namespace {

constexpr int kMaxCols = PE_BIAS_NLL_MAX_COLUMNS;

struct BiasArgs {
    const double* base;         // [C, k1]
    const int32_t* labels;      // [C]
    const double* cand;         // [nc, k1] (the head of the workspace)
    int items, k1, nc;          // items = C
    double* partial;            // [blocks, nc, 1 + k1], added up by pe::launch_finish (csrc/reduce2.h)
    int32_t* flags;             // pe::flag_excluded: excluded clusters
    __host__ __device__ int values() const { return 1 + k1; }
};

// pe::sweep's loop written out (as a model of the template the kernel takes 184 VGPRs for 154 and loses a wave per SIMD); the staging,
// the write-out and the launch are the shared ones.  Wave w of block g takes clusters g * 4 + w, + gridDim.x * 4, ...
__global__ __launch_bounds__(pe::kSweepThreads) void bias_nll_kernel(BiasArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k1 = a.k1;
    double b[kMaxCols], acc[1 + kMaxCols] = {};      // the NLL, then the gradient
#pragma unroll
    for (int j = 0; j < kMaxCols; ++j) b[j] = j < k1 ? a.cand[(size_t)(lane < a.nc ? lane : 0) * k1 + j] : 0.0;
    const int step = gridDim.x * pe::kSweepWaves;
    for (int c = blockIdx.x * pe::kSweepWaves + wv; c < a.items; c += step) {              // wave-uniform
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
        acc[0] += log(tot) - (ay - top);
#pragma unroll
        for (int j = 0; j < kMaxCols; ++j)
            if (j < k1) acc[1 + j] += x[j] / tot - (j == y ? 1.0 : 0.0);
    }
    pe::sweep_store(acc, a.nc, a.values(), a.partial);
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
    const int nw = num_candidates * num_columns;
    if (int rc = pe::stage_candidates(candidates_host, nw, workspace, st, "pe_bias_nll (candidates)")) return rc;
    BiasArgs a{};
    a.base = base; a.labels = labels; a.cand = workspace; a.items = num_clusters; a.k1 = num_columns; a.nc = num_candidates;
    a.partial = workspace + nw; a.flags = out_flags;
    return pe::launch_sweep(bias_nll_kernel, a, PE_BIAS_NLL_MAX_BLOCKS, out, st, what);
}
