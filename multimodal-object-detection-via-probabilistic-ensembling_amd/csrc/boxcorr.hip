// Correlated box fusion, box_fusion "c-avg" (gfx950): the detectors' box errors share a correlation matrix P [D][D], D <= 4.
//   pe_box_gls_batch   : the generalised-least-squares mean of every cluster of two or more rows, a second launch after the fusion
//   pe_box_pair_stats  : the fit's sufficient statistics, cross products of the members' normalised residuals per detector pair
// Built with -ffp-contract=off like the other ProbEn code.  DESIGN.md section 19.
//
// THE RULE.  Cluster rows t in ascending input-row order, var_t the (scaled) variance, s_t = sqrt(var_t), d = d_t the row's detector,
// a_d = 1 - P[d][d].  Covariance C_tu = R_tu s_t s_u with R = diag(a) + G P G' (G the m x D membership matrix): P[a][b] between rows of
// different detectors, P[d][d] between two rows of one detector, 1 on the diagonal.  y = C^-1 1, Y = sum_t y_t, lambda_t = y_t / Y,
// box_c = sum_t coord_c(t) * lambda_t, out_var = 1 / Y.  Woodbury's identity makes it a 4 x 4 system per cluster:
//   u_t = 1 / s_t,  g_d = (sum_{t in d} u_t) / a_d,  nn_d = n_d / a_d  (n_d the cluster's rows of detector d),
//   (I + P diag(nn)) w = P g,  y_t = (1 / var_t) / a_d - w_d / (a_d * s_t).
// P = 0 gives w = 0 exactly and y_t = 1 / var_t: the weights of "v-avg".  I + P diag(nn) is a diagonal scaling of the symmetric
// positive definite I + nn^1/2 P nn^1/2, so the elimination needs no pivoting; a detector absent from the cluster (and every d >= D)
// has a zero column / an identity row.  That matrix - equivalently R - is positive definite for every cluster with at most one row per
// detector under a matrix calibration.check_box_correlation passed, and for every composition when P itself is positive semidefinite; a
// cluster for which it is not (several rows of one detector under an off-diagonal entry the diagonal cannot carry) shows a pivot <= 0
// and gets NaN for its box and variance, like a cluster with a row of an unknown detector.
//
// THE SUMMATION ORDER of pe_box_pair_stats (no floating-point atomics; the grid is a function of the cluster count alone: same input,
// same bits).  z_t = r_t / s_t, s_t = sqrt(var_t), r = get_deltas(member box, the cluster's ground truth) as in pe_variance_stats; a first
// kernel, a thread per member row, leaves r_t, s_t and the member's detector (-1: excluded) in the workspace, and the products are
// formed from those: r_tc^2 / var_t is pe_variance_stats' term, r_tc r_uc / (s_t s_u) the same three operations.  Thread g of the
// min(ceil(clusters / 256), PE_BOX_PAIR_MAX_BLOCKS) workgroups takes clusters g, g + threads, ... in order.  Inside a cluster the member
// rows t are walked in order: first q_t = ((e_0 + e_1) + e_2) + e_3, e_c = r_tc^2 / var_t, is added to Q_d, then for every later member u
// in order p_tu = ((f_0 + f_1) + f_2) + f_3, f_c = r_tc r_uc / (s_t s_u), is added to S_ab, {a, b} = {d_t, d_u}.  A workgroup adds its 256 threads in a
// stride-halving tree in LDS; pe::launch_finish (csrc/reduce2.h) adds the workgroups' partials in its stated order.
#include "common.h"
#include "reduce2.h"
#include "box_residual.h"

namespace {

constexpr int kMaxDet = PE_BOX_CORR_MAX_DETECTORS;
static_assert(kMaxDet == 4, "the elimination and the predicated selects are written out for four detectors");

// ---------------------------------------------------------------------------------------------------------------------------------
// pe_box_gls_batch
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kGlsThreads = 256;
constexpr int kGlsTile = 1024;        // rows staged in LDS at a time: 1024 * (5 * 8 + 2 * 4) = 48 KiB; an image of up to 2048 rows takes two tiles

struct GlsArgs {
    const double* boxes;
    const double* vars;
    const int32_t* source;
    const int32_t* cluster;
    const int32_t* offsets;
    const int32_t* row_counts;
    const int32_t* counts;
    const double* corr;
    int32_t D, max_rows;
    double* out_boxes;
    double* out_vars;
};

// x = (d == 0 ? v0 : d == 1 ? v1 : ...): a select, never an array indexed at run time
__device__ __forceinline__ double pick4(int d, double v0, double v1, double v2, double v3) {
    return d == 0 ? v0 : d == 1 ? v1 : d == 2 ? v2 : v3;
}

// (I + P diag(nn)) w = P g by Gaussian elimination without pivoting, fully unrolled: every index is a compile-time constant.
// The leading minors are those of I + nn^1/2 P nn^1/2 (a diagonal similarity keeps them), so the four pivots are all > 0 exactly when
// the cluster's R is positive definite; returns whether they are.
__device__ __forceinline__ bool solve4(const double (&P)[kMaxDet][kMaxDet], const double (&nn)[kMaxDet], const double (&g)[kMaxDet],
                                       double (&w)[kMaxDet]) {
    double A[kMaxDet][kMaxDet], b[kMaxDet];
#pragma unroll
    for (int i = 0; i < kMaxDet; ++i) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kMaxDet; ++j) {
            A[i][j] = (i == j ? 1.0 : 0.0) + P[i][j] * nn[j];
            acc += P[i][j] * g[j];
        }
        b[i] = acc;
    }
#pragma unroll
    for (int k = 0; k < kMaxDet - 1; ++k) {
#pragma unroll
        for (int i = k + 1; i < kMaxDet; ++i) {
            const double f = A[i][k] / A[k][k];
#pragma unroll
            for (int j = k + 1; j < kMaxDet; ++j) A[i][j] -= f * A[k][j];
            b[i] -= f * b[k];
        }
    }
    bool pd = true;
#pragma unroll
    for (int i = kMaxDet - 1; i >= 0; --i) {
        double acc = b[i];
#pragma unroll
        for (int j = i + 1; j < kMaxDet; ++j) acc -= A[i][j] * w[j];
        w[i] = acc / A[i][i];
        pd = pd && A[i][i] > 0.0;
    }
    return pd;
}

// A workgroup per image, the image's rows staged in LDS a tile at a time, a thread per fused row k (groups of 256 when an image has
// more).  Three walks over the rows with cluster == k, each in ascending row order: n_d and sum u_t; Y; the four coordinates with
// lambda_t = y_t / Y (the order of "v-avg": the weight is divided before it multiplies the coordinate).  Every lane reads the same LDS
// address (a broadcast); all loop bounds and every barrier are workgroup-uniform.  Each output element is written once, by its thread.
__global__ __launch_bounds__(kGlsThreads) void box_gls_kernel(GlsArgs a) {
    __shared__ double sc[4][kGlsTile], sv[kGlsTile];
    __shared__ int32_t ssrc[kGlsTile], scl[kGlsTile];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int beg = a.offsets[img];
    const int n = a.row_counts ? a.row_counts[img] : a.offsets[img + 1] - beg;
    const int cnt = a.counts[img];
    if (cnt <= 0 || n < 2 || n > a.max_rows || cnt > n) return;      // counts == -1 (rows above the fusion's bound), empty, nothing to fuse
    double P[kMaxDet][kMaxDet], ad[kMaxDet];
#pragma unroll
    for (int i = 0; i < kMaxDet; ++i) {
#pragma unroll
        for (int j = 0; j < kMaxDet; ++j) P[i][j] = (i < a.D && j < a.D) ? a.corr[i * a.D + j] : 0.0;      // uniform: scalar loads
        ad[i] = 1.0 - P[i][i];
    }
    const int ntiles = (n + kGlsTile - 1) / kGlsTile;
    int staged = -1;                                                  // workgroup-uniform
    auto stage = [&](int t) {
        if (t == staged) return;
        __syncthreads();                                              // the previous tile has been read by every thread
        const int r0 = t * kGlsTile, m = min(kGlsTile, n - r0);
        for (int r = tid; r < m; r += kGlsThreads) {
            const size_t o = (size_t)beg + r0 + r;
            sc[0][r] = a.boxes[o * 4]; sc[1][r] = a.boxes[o * 4 + 1]; sc[2][r] = a.boxes[o * 4 + 2]; sc[3][r] = a.boxes[o * 4 + 3];
            sv[r] = a.vars[o];
            ssrc[r] = a.source[o];
            scl[r] = a.cluster[o];
        }
        __syncthreads();
        staged = t;
    };
    for (int k0 = 0; k0 < cnt; k0 += kGlsThreads) {
        const int k = k0 + tid;                                       // k >= cnt matches no row: the thread only keeps the barriers
        // ---- walk 1: n_d, sum u_t ----
        double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0, u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0;
        int m = 0;
        bool bad = false;
        for (int t = 0; t < ntiles; ++t) {
            stage(t);
            const int rows = min(kGlsTile, n - t * kGlsTile);
            for (int r = 0; r < rows; ++r) {
                if (scl[r] != k || k >= cnt) continue;
                const int d = ssrc[r];
                const double u = 1.0 / sqrt(sv[r]);
                bad = bad || d < 0 || d >= a.D;
                ++m;
                n0 += d == 0 ? 1.0 : 0.0; n1 += d == 1 ? 1.0 : 0.0; n2 += d == 2 ? 1.0 : 0.0; n3 += d == 3 ? 1.0 : 0.0;
                u0 += d == 0 ? u : 0.0; u1 += d == 1 ? u : 0.0; u2 += d == 2 ? u : 0.0; u3 += d == 3 ? u : 0.0;
            }
        }
        const double nn[kMaxDet] = {n0 / ad[0], n1 / ad[1], n2 / ad[2], n3 / ad[3]};
        const double g[kMaxDet] = {u0 / ad[0], u1 / ad[1], u2 / ad[2], u3 / ad[3]};
        double w[kMaxDet];
        bad = !solve4(P, nn, g, w) || bad;          // R not positive definite: no such distribution, NaN like a bad source
        auto weight = [&](int r) {
            const int d = ssrc[r];
            const double var = sv[r], s = sqrt(var), adt = pick4(d, ad[0], ad[1], ad[2], ad[3]);
            return (1.0 / var) / adt - pick4(d, w[0], w[1], w[2], w[3]) / (adt * s);
        };
        // ---- walk 2: Y ----
        double Y = 0.0;
        for (int t = 0; t < ntiles; ++t) {
            stage(t);
            const int rows = min(kGlsTile, n - t * kGlsTile);
            for (int r = 0; r < rows; ++r)
                if (scl[r] == k && k < cnt) Y += weight(r);
        }
        // ---- walk 3: the coordinates ----
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
        for (int t = 0; t < ntiles; ++t) {
            stage(t);
            const int rows = min(kGlsTile, n - t * kGlsTile);
            for (int r = 0; r < rows; ++r) {
                if (scl[r] != k || k >= cnt) continue;
                const double lam = weight(r) / Y;
                c0 += sc[0][r] * lam; c1 += sc[1][r] * lam; c2 += sc[2][r] * lam; c3 += sc[3][r] * lam;
            }
        }
        if (k < cnt && m >= 2) {
            const double nan = __builtin_nan("");
            const size_t o = (size_t)beg + k;
            a.out_boxes[o * 4] = bad ? nan : c0; a.out_boxes[o * 4 + 1] = bad ? nan : c1;
            a.out_boxes[o * 4 + 2] = bad ? nan : c2; a.out_boxes[o * 4 + 3] = bad ? nan : c3;
            if (a.out_vars) a.out_vars[o] = bad ? nan : 1.0 / Y;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// pe_box_pair_stats
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kPairThreads = 256;
constexpr int kPairs = kMaxDet * (kMaxDet + 1) / 2;      // 10 detector pairs a <= b
constexpr int kHalf = kPairs + kMaxDet;                   // 14 counts (N_ab, M_d), then 14 sums (S_ab, Q_d)

struct PairArgs {
    const double* boxes;            // [N, 4] the packed rows
    const double* vars;             // [N]
    const int32_t* source;          // [N]
    const int32_t* member_rows;     // [M]
    const int32_t* cluster_offsets; // [C + 1]
    const int32_t* match;           // [C] ground-truth index of the cluster, -1: none
    const double* gt;               // [G, 4]
    long long N, M, G;
    int32_t C, D;
    double w[4];
    double* r;                      // [M, 4] the member's residual
    double* sv;                     // [M, 2] sqrt(var), var
    int32_t* zsrc;                  // [M] the member's detector, -1: takes no part
    double* partial;                // [blocks, 28]
    int32_t* flags;
};

// a thread per member row: its cluster by bisection over the offsets, its residual, sqrt(var) and var, and its detector (or -1)
__global__ __launch_bounds__(kPairThreads) void box_residual_kernel(PairArgs a) {
    const long long i = (long long)blockIdx.x * kPairThreads + threadIdx.x;
    if (i >= a.M) return;
    int lo = 0, hi = a.C;           // cluster_offsets[lo] <= i < cluster_offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.cluster_offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const int g = a.match[lo];
    int out_src = -1;
    double z[4] = {0.0, 0.0, 0.0, 0.0}, sd = 1.0, vv = 1.0;
    if (g >= 0 && g < a.G) {        // a cluster without a ground-truth box adds nothing and is no exclusion
        const int row = a.member_rows[i];
        bool ok = row >= 0 && row < a.N;
        double v = 0.0;
        int d = -1;
        if (ok) {
            v = a.vars[row];
            d = a.source[row];
            ok = v > 0.0 && v < __builtin_huge_val() && d >= 0 && d < a.D;
        }
        if (ok && pe::box_residual(a.boxes + (size_t)row * 4, a.gt + (size_t)g * 4, a.w, z)) {      // pe_variance_stats' residual
            sd = sqrt(v);
            vv = v;
            out_src = d;
        } else {
            pe::flag_excluded(a.flags, i);
        }
    }
    for (int c = 0; c < 4; ++c) a.r[(size_t)i * 4 + c] = z[c];
    a.sv[(size_t)i * 2] = sd;
    a.sv[(size_t)i * 2 + 1] = vv;
    a.zsrc[i] = out_src;
}

// index of the pair a <= b among the 10: row a of the upper triangle starts at a * 4 - a (a - 1) / 2
__device__ __forceinline__ int pair_index(int a, int b) { return a * 4 - (a * (a - 1)) / 2 + (b - a); }

__global__ __launch_bounds__(kPairThreads) void box_pair_kernel(PairArgs a) {
    __shared__ double x[kPairThreads][kHalf];
    double S[kHalf];                // S_ab [10], Q_d [4]
    long long Nc[kHalf];            // N_ab [10], M_d [4]
#pragma unroll
    for (int v = 0; v < kHalf; ++v) { S[v] = 0.0; Nc[v] = 0; }
    const int step = gridDim.x * kPairThreads;
    for (int c = blockIdx.x * kPairThreads + threadIdx.x; c < a.C; c += step) {
        const int m0 = a.cluster_offsets[c], m1 = a.cluster_offsets[c + 1];
        for (int t = m0; t < m1; ++t) {
            const int dt = a.zsrc[t];
            if (dt < 0) continue;
            const double* zt = a.r + (size_t)t * 4;
            const double z0 = zt[0], z1 = zt[1], z2 = zt[2], z3 = zt[3];
            const double st = a.sv[(size_t)t * 2], vt = a.sv[(size_t)t * 2 + 1];
            const double q = ((z0 * z0 / vt + z1 * z1 / vt) + z2 * z2 / vt) + z3 * z3 / vt;
#pragma unroll
            for (int d = 0; d < kMaxDet; ++d) {
                S[kPairs + d] += d == dt ? q : 0.0;
                Nc[kPairs + d] += d == dt ? 1 : 0;
            }
            for (int u = t + 1; u < m1; ++u) {
                const int du = a.zsrc[u];
                if (du < 0) continue;
                const double* zu = a.r + (size_t)u * 4;
                const double den = st * a.sv[(size_t)u * 2];
                const double p = ((z0 * zu[0] / den + z1 * zu[1] / den) + z2 * zu[2] / den) + z3 * zu[3] / den;
                const int idx = pair_index(min(dt, du), max(dt, du));
#pragma unroll
                for (int v = 0; v < kPairs; ++v) {
                    S[v] += v == idx ? p : 0.0;
                    Nc[v] += v == idx ? 1 : 0;
                }
            }
        }
    }
    // the sums, then the counts through the same LDS array: a stride-halving tree, the same pairs whatever the data
#pragma unroll
    for (int v = 0; v < kHalf; ++v) x[threadIdx.x][v] = S[v];
    pe::block_tree(x, kPairThreads);
    if (threadIdx.x == 0)
        for (int v = 0; v < kHalf; ++v) a.partial[(size_t)blockIdx.x * 2 * kHalf + kHalf + v] = x[0][v];
    __syncthreads();
    long long (*xi)[kHalf] = reinterpret_cast<long long (*)[kHalf]>(x);
#pragma unroll
    for (int v = 0; v < kHalf; ++v) xi[threadIdx.x][v] = Nc[v];
    pe::block_tree(xi, kPairThreads);
    if (threadIdx.x == 0)
        for (int v = 0; v < kHalf; ++v) a.partial[(size_t)blockIdx.x * 2 * kHalf + v] = __longlong_as_double(xi[0][v]);
}

}  // namespace

extern "C" int pe_box_gls_batch(const double* boxes, const double* variances, const int32_t* row_source, const int32_t* cluster,
                                const int32_t* offsets, const int32_t* row_counts, const int32_t* counts, int32_t num_images,
                                int32_t max_rows_per_image, const double* correlation, int32_t num_detectors, double* out_boxes,
                                double* out_vars, void* stream) {
    const char* what = "pe_box_gls_batch";
    PE_CHECK_ARG(num_images >= 0, "%s: num_images < 0", what);
    PE_CHECK_ARG(num_detectors >= 1 && num_detectors <= PE_BOX_CORR_MAX_DETECTORS, "%s: num_detectors %d not in [1,%d]", what, num_detectors,
                 PE_BOX_CORR_MAX_DETECTORS);
    // an image's rows are staged in LDS a tile of 1024 at a time (48 bytes per row: 48 KiB), so the capacity is the fusion's own bound
    PE_CHECK_ARG(max_rows_per_image >= 1 && max_rows_per_image <= 2048, "%s: max_rows_per_image %d not in [1,2048]", what, max_rows_per_image);
    if (num_images == 0) return PE_OK;
    PE_CHECK_ARG(boxes && variances && row_source && cluster && offsets && counts, "%s: null input pointer", what);
    PE_CHECK_ARG(correlation, "%s: null input pointer (correlation)", what);
    PE_CHECK_ARG(out_boxes, "%s: null output pointer", what);
    GlsArgs a{boxes, variances, row_source, cluster, offsets, row_counts, counts, correlation, num_detectors, (max_rows_per_image + 1) & ~1,
              out_boxes, out_vars};
    hipLaunchKernelGGL(box_gls_kernel, dim3(num_images), dim3(kGlsThreads), 0, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}

extern "C" int pe_box_pair_stats(const double* boxes, const double* variances, const int32_t* row_source, int64_t num_rows,
                                 const int32_t* member_rows, int64_t num_members, const int32_t* cluster_offsets,
                                 const int32_t* cluster_match, int32_t num_clusters, const double* gt_boxes, int64_t num_gt, int32_t num_detectors,
                                 const float* bbox_reg_weights_host, double* workspace, double* out, int32_t* out_flags, void* stream) {
    const char* what = "pe_box_pair_stats";
    PE_CHECK_ARG(num_detectors >= 1 && num_detectors <= PE_BOX_CORR_MAX_DETECTORS, "%s: num_detectors %d not in [1,%d]", what, num_detectors,
                 PE_BOX_CORR_MAX_DETECTORS);
    PE_CHECK_ARG(num_clusters >= 0 && num_rows >= 0 && num_gt >= 0 && num_members >= 0 && num_members <= 0x7fffffff,
                 "%s: num_clusters %d, num_rows %lld, num_members %lld, num_gt %lld", what, num_clusters, (long long)num_rows,
                 (long long)num_members, (long long)num_gt);
    PE_CHECK_ARG(workspace && out && out_flags, "%s: null pointer (workspace / out / out_flags)", what);
    PE_CHECK_ARG(num_clusters == 0 || (member_rows && cluster_offsets && cluster_match), "%s: null pointer (member_rows / cluster_offsets / cluster_match)",
                 what);
    PE_CHECK_ARG(num_clusters == 0 || (boxes && variances && row_source && (gt_boxes || num_gt == 0)),
                 "%s: null pointer (boxes / variances / row_source / gt_boxes)", what);
    PairArgs a{};
    if (int rc = pe::bbox_reg_weights(bbox_reg_weights_host, a.w, what)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = pe::zero_flags(out_flags, st, what)) return rc;
    if (num_clusters == 0) {        // nothing to add up: zeros, no launch
        if (hipMemsetAsync(out, 0, 2 * kHalf * sizeof(double), st) != hipSuccess) {
            pe::set_error("%s: hipMemsetAsync of the result failed", what);
            return PE_ERR_HIP;
        }
        return PE_OK;
    }
    const long long M = num_members;        // = cluster_offsets[num_clusters]: the caller holds it (it sized the workspace from it)
    a.boxes = boxes; a.vars = variances; a.source = row_source; a.member_rows = member_rows; a.cluster_offsets = cluster_offsets;
    a.match = cluster_match; a.gt = gt_boxes; a.N = num_rows; a.M = M; a.G = num_gt; a.C = num_clusters; a.D = num_detectors;
    a.r = workspace;
    a.sv = workspace + 4 * M;
    a.zsrc = reinterpret_cast<int32_t*>(workspace + 6 * M);
    a.partial = workspace + 6 * M + (M + 1) / 2;
    a.flags = out_flags;
    if (M > 0) {
        hipLaunchKernelGGL(box_residual_kernel, dim3(pe::ceil_div(M, kPairThreads)), dim3(kPairThreads), 0, st, a);
        PE_CHECK_LAUNCH("pe_box_pair_stats (residuals)");
    }
    // the grid is a function of num_clusters alone: same input, same partition, same bits
    const int blocks = std::min(pe::ceil_div(num_clusters, kPairThreads), PE_BOX_PAIR_MAX_BLOCKS);
    hipLaunchKernelGGL(box_pair_kernel, dim3(blocks), dim3(kPairThreads), 0, st, a);
    PE_CHECK_LAUNCH(what);
    return pe::launch_finish(a.partial, blocks, 2 * kHalf, kHalf, reinterpret_cast<long long*>(out), out + kHalf, st, what);
}
