// Pooling weights of log-posterior ProbEn (gfx950): the fit's objective.
//   pe_pool_nll : sum over clusters of -log s_label(w) and its gradient in w, s = the pooled posterior pe_proben_fuse_batch_pooled
//                 forms, for up to 64 candidate weight vectors in one launch
// Layout as pe_temperature_nll (csrc/calibrate.hip): lane = candidate, wavefront = cluster.  a_j is linear in w,
//   a_j(w) = sum_d w_d G_dj + lp_j,   G_dj = S_dj - n_d lp_j,   S_dj = the cluster's rows of detector d summed over log p_t[j],
// so a wavefront reads its cluster's rows ONCE (lane = column, coalesced, member order) into the table G [num_detectors][K + 1] in LDS
// and all 64 candidates work from that table (every lane reads the same address: a broadcast).  d NLL / d w_d = sum_j s_j G_dj - G_d,label.
// Built with -ffp-contract=off like the other ProbEn code.
#include "common.h"
#include "reduce2.h"

namespace {

constexpr int kPoolThreads = 256, kPoolWaves = kPoolThreads / 64;
constexpr int kMaxDet = PE_POOL_MAX_DETECTORS, kMaxCols = 64;

struct PoolArgs {
    const double* log_probs;        // [N, k1]
    const int32_t* row_source;      // [N]
    const int32_t* member_rows;     // [M]
    const int32_t* cluster_offsets; // [C + 1]
    const int32_t* labels;          // [C]
    const double* log_prior;        // optional [k1]
    const double* weights;          // [nc, D] (the head of the workspace)
    long long N, M;
    int C, k1, D, nc;
    double* partial;                // [blocks, nc, 1 + D], added up by pe::launch_finish (csrc/reduce2.h)
    int32_t* flags;                 // pe::flag_excluded: excluded clusters
};

// the candidates travel as kernel arguments, 256 doubles a launch, into the head of the workspace: stream-ordered, and the host
// array is free again when pe_pool_nll returns
struct StageArgs {
    double v[256];
    double* dst;
    int n;
};

__global__ __launch_bounds__(256) void pool_stage_kernel(StageArgs a) {
    if ((int)threadIdx.x < a.n) a.dst[threadIdx.x] = a.v[threadIdx.x];
}

// Wave w of block g takes clusters g * kPoolWaves + w, + gridDim.x * kPoolWaves, ...: a fixed order for a fixed (C, grid).
__global__ __launch_bounds__(kPoolThreads) void pool_nll_kernel(PoolArgs a) {
    __shared__ double G[kPoolWaves][kMaxDet][kMaxCols];
    __shared__ double part[kPoolWaves][1 + kMaxDet][64];
    __shared__ double LP[kMaxCols];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k1 = a.k1, D = a.D;
    double w[kMaxDet];
#pragma unroll
    for (int d = 0; d < kMaxDet; ++d) w[d] = d < D ? a.weights[(size_t)(lane < a.nc ? lane : 0) * D + d] : 0.0;
    double nll = 0.0, grad[kMaxDet];
#pragma unroll
    for (int d = 0; d < kMaxDet; ++d) grad[d] = 0.0;
    if (threadIdx.x < kMaxCols) LP[threadIdx.x] = (a.log_prior && (int)threadIdx.x < k1) ? a.log_prior[threadIdx.x] : 0.0;
    __syncthreads();
    const double lpl = LP[lane];      // lane = column while the table is built
    const int step = gridDim.x * kPoolWaves;
    for (int c = blockIdx.x * kPoolWaves + wv; c < a.C; c += step) {              // wave-uniform
        const int beg = a.cluster_offsets[c], end = a.cluster_offsets[c + 1];
        const int y = a.labels[c];
        bool bad = end - beg < 2 || beg < 0 || (long long)end > a.M || y < 0 || y >= k1;
        if (!bad) {
            for (int base = beg; base < end; base += 64) {                        // every member row and its source in range?
                bool rb = false;
                if (base + lane < end) {
                    const int r = a.member_rows[base + lane];
                    rb = r < 0 || r >= a.N;
                    if (!rb) {
                        const int s = a.row_source[r];
                        rb = s < 0 || s >= D;
                    }
                }
                bad = bad || __ballot(rb) != 0ull;
            }
        }
        if (bad) {
            if (lane == 0) pe::flag_excluded(a.flags, c);
            continue;
        }
        // ---- the table: lane j sums column j of the cluster's rows per detector, in member order; then G = S - n_d lp ----
        double (*g)[kMaxCols] = G[wv];
        int nd[kMaxDet];
#pragma unroll
        for (int d = 0; d < kMaxDet; ++d) { g[d][lane] = 0.0; nd[d] = 0; }
        for (int t = beg; t < end; ++t) {
            const int r = a.member_rows[t];            // wave-uniform loads
            const int s = a.row_source[r];
            if (lane < k1) g[s][lane] += a.log_probs[(size_t)r * k1 + lane];
#pragma unroll
            for (int d = 0; d < kMaxDet; ++d) nd[d] += d == s ? 1 : 0;
        }
        if (a.log_prior) {
#pragma unroll
            for (int d = 0; d < kMaxDet; ++d)
                if (d < D && lane < k1) g[d][lane] -= (double)nd[d] * lpl;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the table is read by the other lanes of this wave
        __builtin_amdgcn_wave_barrier();
        // ---- lane = candidate ----
        auto col = [&](int j) {
            double acc = 0.0;
#pragma unroll
            for (int d = 0; d < kMaxDet; ++d)
                if (d < D) acc += w[d] * g[d][j];
            if (a.log_prior) acc += LP[j];
            return acc;
        };
        double top = col(0);
        for (int j = 1; j < k1; ++j) {
            const double v = col(j);
            top = (v > top || v != v) ? v : top;
        }
        double tot = 0.0, eg[kMaxDet];
#pragma unroll
        for (int d = 0; d < kMaxDet; ++d) eg[d] = 0.0;
        for (int j = 0; j < k1; ++j) {
            const double e = exp(col(j) - top);
            tot += e;
#pragma unroll
            for (int d = 0; d < kMaxDet; ++d)
                if (d < D) eg[d] += e * g[d][j];
        }
        nll += log(tot) - (col(y) - top);
#pragma unroll
        for (int d = 0; d < kMaxDet; ++d)
            if (d < D) grad[d] += eg[d] / tot - g[d][y];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // before the next cluster overwrites the table
        __builtin_amdgcn_wave_barrier();
    }
    part[wv][0][lane] = nll;
#pragma unroll
    for (int d = 0; d < kMaxDet; ++d) part[wv][1 + d][lane] = grad[d];
    __syncthreads();
    // thread (v, lane): value v of candidate lane, the block's waves in wave order
    for (int v = wv; v < 1 + D; v += kPoolWaves) {
        if (lane < a.nc) {
            double s = part[0][v][lane];
            for (int u = 1; u < kPoolWaves; ++u) s += part[u][v][lane];
            a.partial[((size_t)blockIdx.x * a.nc + lane) * (1 + D) + v] = s;
        }
    }
}

}  // namespace

extern "C" int pe_pool_nll(const double* log_probs, const int32_t* row_source, int64_t num_rows, int32_t num_columns,
                           const int32_t* member_rows, int64_t num_members, const int32_t* cluster_offsets, const int32_t* labels,
                           int32_t num_clusters, const double* log_prior, const double* weights_host, int32_t num_candidates,
                           int32_t num_detectors, double* workspace, double* out, int32_t* out_flags, void* stream) {
    const char* what = "pe_pool_nll";
    PE_CHECK_ARG(num_candidates >= 1 && num_candidates <= 64, "%s: num_candidates %d not in [1,64]", what, num_candidates);
    PE_CHECK_ARG(num_detectors >= 1 && num_detectors <= PE_POOL_MAX_DETECTORS, "%s: num_detectors %d not in [1,%d]", what, num_detectors,
                 PE_POOL_MAX_DETECTORS);
    PE_CHECK_ARG(weights_host, "%s: null pointer (weights)", what);
    for (int i = 0; i < num_candidates * num_detectors; ++i) {
        const double x = weights_host[i];
        PE_CHECK_ARG(x == x && x >= 0.0 && x < __builtin_huge_val(), "%s: weight %g (candidate %d, detector %d) is not finite and >= 0", what,
                     x, i / num_detectors, i % num_detectors);
    }
    PE_CHECK_ARG(num_rows >= 0 && num_members >= 0 && num_clusters >= 0, "%s: num_rows %lld, num_members %lld, num_clusters %d", what,
                 (long long)num_rows, (long long)num_members, num_clusters);
    PE_CHECK_ARG(num_rows <= 0x7fffffffLL && num_members <= 0x7fffffffLL, "%s: num_rows %lld / num_members %lld do not fit the int32 indices",
                 what, (long long)num_rows, (long long)num_members);
    PE_CHECK_ARG(num_columns >= 2 && num_columns <= 64, "%s: num_columns %d (K + 1) not in [2,64]", what, num_columns);
    PE_CHECK_ARG(workspace && out && out_flags, "%s: null pointer (workspace / out / out_flags)", what);
    PE_CHECK_ARG(num_clusters == 0 || (cluster_offsets && labels), "%s: null pointer (cluster_offsets / labels)", what);
    PE_CHECK_ARG(num_members == 0 || member_rows, "%s: null pointer (member_rows)", what);
    PE_CHECK_ARG(num_rows == 0 || (log_probs && row_source), "%s: null pointer (log_probs / row_source)", what);
    hipStream_t st = (hipStream_t)stream;
    const int nw = num_candidates * num_detectors, nv = num_candidates * (1 + num_detectors);
    for (int o = 0; o < nw; o += 256) {
        StageArgs s{};
        s.n = std::min(256, nw - o);
        s.dst = workspace + o;
        for (int i = 0; i < s.n; ++i) s.v[i] = weights_host[o + i];
        hipLaunchKernelGGL(pool_stage_kernel, dim3(1), dim3(256), 0, st, s);
        PE_CHECK_LAUNCH("pe_pool_nll (weights)");
    }
    PoolArgs a{};
    a.log_probs = log_probs; a.row_source = row_source; a.member_rows = member_rows; a.cluster_offsets = cluster_offsets;
    a.labels = labels; a.log_prior = log_prior; a.weights = workspace; a.N = num_rows; a.M = num_members; a.C = num_clusters;
    a.k1 = num_columns; a.D = num_detectors; a.nc = num_candidates; a.partial = workspace + nw; a.flags = out_flags;
    // the grid is a function of num_clusters alone: same input, same partition, same bits
    const int blocks = std::max(1, std::min((num_clusters + kPoolWaves - 1) / kPoolWaves, PE_POOL_NLL_MAX_BLOCKS));
    if (int rc = pe::zero_flags(out_flags, st, what)) return rc;
    hipLaunchKernelGGL(pool_nll_kernel, dim3(blocks), dim3(kPoolThreads), 0, st, a);
    PE_CHECK_LAUNCH(what);
    return pe::launch_finish(a.partial, blocks, nv, 0, nullptr, out, st, what);
}
