// Pooling weights of log-posterior ProbEn (gfx950): the fit's objective.
//   pe_pool_nll : sum over clusters of -log s_label(w) and its gradient in w, s = the pooled posterior pe_proben_fuse_batch_pooled
//                 forms, for up to 64 candidate weight vectors in one launch
// The candidate sweep of csrc/sweep.h: lane = candidate, wavefront = cluster.  a_j is linear in w,
//   a_j(w) = sum_d w_d G_dj + lp_j,   G_dj = S_dj - n_d lp_j,   S_dj = the cluster's rows of detector d summed over log p_t[j],
// so a wavefront reads its cluster's rows ONCE (lane = column, coalesced, member order) into the table G [num_detectors][K + 1] in LDS
// and all 64 candidates work from that table (every lane reads the same address: a broadcast).  d NLL / d w_d = sum_j s_j G_dj - G_d,label.
// Built with -ffp-contract=off like the other ProbEn code.
#include "common.h"
#include "sweep.h"

namespace {

constexpr int kMaxDet = PE_POOL_MAX_DETECTORS, kMaxCols = 64;

// the model of pe::sweep (csrc/sweep.h): an item is a cluster, the sums are the NLL and the D gradient entries
struct PoolModel {
    static constexpr int kMaxValues = 1 + kMaxDet;
    struct Shared {
        double G[pe::kSweepWaves][kMaxDet][kMaxCols];      // a wave's table
        double LP[kMaxCols];                               // log_prior, 0 without one
    };
    struct Lane {
        double w[kMaxDet];
        double lpl;                 // LP[lane]: lane = column while the table is built
    };
    const double* log_probs;        // [N, k1]
    const int32_t* row_source;      // [N]
    const int32_t* member_rows;     // [M]
    const int32_t* cluster_offsets; // [C + 1]
    const int32_t* labels;          // [C]
    const double* log_prior;        // optional [k1]
    const double* weights;          // [nc, D] (the head of the workspace)
    long long N, M;
    int items, k1, D, nc;           // items = C
    double* partial;                // [blocks, nc, 1 + D], added up by pe::launch_finish (csrc/reduce2.h)
    int32_t* flags;                 // pe::flag_excluded: excluded clusters

    __host__ __device__ __forceinline__ int values() const { return 1 + D; }
    __device__ __forceinline__ void setup(Shared& sh) const {
        if (threadIdx.x < kMaxCols) sh.LP[threadIdx.x] = (log_prior && (int)threadIdx.x < k1) ? log_prior[threadIdx.x] : 0.0;
    }
    __device__ __forceinline__ void load(Lane& L, int c, Shared& sh) const {
#pragma unroll
        for (int d = 0; d < kMaxDet; ++d) L.w[d] = d < D ? weights[(size_t)c * D + d] : 0.0;
        L.lpl = sh.LP[threadIdx.x & 63];
    }
    __device__ __forceinline__ bool item(const Lane& L, double (&acc)[kMaxValues], int c, Shared& sh) const {
        const int lane = threadIdx.x & 63;
        const int beg = cluster_offsets[c], end = cluster_offsets[c + 1];
        const int y = labels[c];
        bool bad = end - beg < 2 || beg < 0 || (long long)end > M || y < 0 || y >= k1;
        if (!bad) {
            for (int base = beg; base < end; base += 64) {                        // every member row and its source in range?
                bool rb = false;
                if (base + lane < end) {
                    const int r = member_rows[base + lane];
                    rb = r < 0 || r >= N;
                    if (!rb) {
                        const int s = row_source[r];
                        rb = s < 0 || s >= D;
                    }
                }
                bad = bad || __ballot(rb) != 0ull;
            }
        }
        if (bad) return false;
        // ---- the table: lane j sums column j of the cluster's rows per detector, in member order; then G = S - n_d lp ----
        double (*g)[kMaxCols] = sh.G[threadIdx.x >> 6];
        int nd[kMaxDet];
#pragma unroll
        for (int d = 0; d < kMaxDet; ++d) { g[d][lane] = 0.0; nd[d] = 0; }
        for (int t = beg; t < end; ++t) {
            const int r = member_rows[t];            // wave-uniform loads
            const int s = row_source[r];
            if (lane < k1) g[s][lane] += log_probs[(size_t)r * k1 + lane];
#pragma unroll
            for (int d = 0; d < kMaxDet; ++d) nd[d] += d == s ? 1 : 0;
        }
        if (log_prior) {
#pragma unroll
            for (int d = 0; d < kMaxDet; ++d)
                if (d < D && lane < k1) g[d][lane] -= (double)nd[d] * L.lpl;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the table is read by the other lanes of this wave
        __builtin_amdgcn_wave_barrier();
        // ---- lane = candidate ----
        auto col = [&](int j) {
            double a = 0.0;
#pragma unroll
            for (int d = 0; d < kMaxDet; ++d)
                if (d < D) a += L.w[d] * g[d][j];
            if (log_prior) a += sh.LP[j];
            return a;
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
        acc[0] += log(tot) - (col(y) - top);
#pragma unroll
        for (int d = 0; d < kMaxDet; ++d)
            if (d < D) acc[1 + d] += eg[d] / tot - g[d][y];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // before the next cluster overwrites the table
        __builtin_amdgcn_wave_barrier();
        return true;
    }
};

__global__ __launch_bounds__(pe::kSweepThreads) void pool_nll_kernel(PoolModel m) { pe::sweep(m); }

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
    const int nw = num_candidates * num_detectors;
    if (int rc = pe::stage_candidates(weights_host, nw, workspace, st, "pe_pool_nll (weights)")) return rc;
    PoolModel m{};
    m.log_probs = log_probs; m.row_source = row_source; m.member_rows = member_rows; m.cluster_offsets = cluster_offsets;
    m.labels = labels; m.log_prior = log_prior; m.weights = workspace; m.N = num_rows; m.M = num_members; m.items = num_clusters;
    m.k1 = num_columns; m.D = num_detectors; m.nc = num_candidates; m.partial = workspace + nw; m.flags = out_flags;
    return pe::launch_sweep(pool_nll_kernel, m, PE_POOL_NLL_MAX_BLOCKS, out, st, what);
}
