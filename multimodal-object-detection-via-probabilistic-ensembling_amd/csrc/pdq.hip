// Probability-based Detection Quality (gfx950): the pair quality of every (ground truth, detection) pair of every image.
//   pe_pdq_pair_quality : q = sqrt(Q_S * Q_L), exp(FG), exp(BG) and Q_L per pair, the ground truths that take part, the exclusion flags
// (the one-to-one assignment over q is host work: pe_pdq_assign, csrc/pdq_assign.cpp).  The rule is stated in include/proben_hip.h and
// DESIGN.md section 30; tests/pdq_ref.py restates it densely in NumPy.
//
// One workgroup of 256 threads per detection, then ceil(G / 256) workgroups that decide which ground truths take part (a thread each).
// A detection's pixel probability is separable, P(v, u) = px[u] * py[v], so its workgroup
//   1  fills px, qx [W] and py, qy [H] in LDS: W + H pairs of erfc, not one per pixel;
//   2  adds B_all = sum over {P > tau} of the background term over the window {px > tau} x {py > tau} (P > tau is tested per pixel:
//      the window only bounds the walk, so nothing depends on px and py being unimodal to the last bit);
//   3  per ground truth of the image adds, over the ground truth's own rectangle, F (the foreground terms) and B_in (the background
//      terms where P > tau): FG = F / n_g, BG = (B_all - B_in) / n_g.  The work of a pair is the ground truth's rectangle.
// Every sum: a thread adds the pixels i = t, t + 256, ... of the rectangle (row-major) in that order, then pe::block_tree adds the 256
// threads.  No floating-point atomics: the same input gives the same bits.  Built with -ffp-contract=off.
#include "common.h"
#define PE_REDUCE2_FLAGS_ONLY
#include "reduce2.h"
#include "box_residual.h"
#include "test_hooks.h"

namespace {

constexpr int kThreads = 256;
constexpr double kEps = 1e-14;
constexpr double kSqrt2 = 1.4142135623730951;

// Phi(z) = 0.5 erfc(-z / sqrt 2), Phic(z) = 0.5 erfc(z / sqrt 2)
__device__ __forceinline__ double Phi(double z) { return 0.5 * erfc(-z / kSqrt2); }
__device__ __forceinline__ double Phic(double z) { return 0.5 * erfc(z / kSqrt2); }

// p = Phi(a) Phi(b) and its complement q = Phic(a) + Phi(a) Phic(b): a sum of positive terms
__device__ __forceinline__ void axis_soft(double a, double b, double& p, double& q) {
    const double pa = Phi(a);
    p = pa * Phi(b);
    q = Phic(a) + pa * Phic(b);
}

// entry i of an axis table: the pixel centre i + 0.5 against the box side [lo, hi] with corner deviation s
__device__ __forceinline__ void axis_entry(int i, double lo, double hi, double s, double& p, double& q) {
    const double c = (double)i + 0.5;
    if (s == 0.0) {
        p = (lo <= c && c <= hi) ? 1.0 : 0.0;
        q = 1.0 - p;
    } else {
        axis_soft((c - lo) / s, (hi - (double)i - 0.5) / s, p, q);
    }
}

// log max(P, eps) and log max(Q, eps) of P = px py, Q = qx + px qy.  Above one half a logarithm is taken of the complement,
// log1p(-Q) = log P: the same number, without the cancellation of log near 1.
__device__ __forceinline__ double term_fg(double P, double Q) { return P > 0.5 ? log1p(-Q) : log(fmax(P, kEps)); }
__device__ __forceinline__ double term_bg(double P, double Q) { return Q > 0.5 ? log1p(-P) : log(fmax(Q, kEps)); }

// the smallest i in [0, n] with i + 0.5 >= x (n when there is none; x is finite)
__device__ __forceinline__ int first_centre_ge(double x, int n) {
    if (!(x > 0.5)) return 0;
    if (x > (double)n) return n;
    int i = (int)ceil(x - 0.5);
    i = max(0, min(i, n));
    while (i > 0 && (double)(i - 1) + 0.5 >= x) --i;
    while (i < n && (double)i + 0.5 < x) ++i;
    return i;
}

__device__ __forceinline__ bool finite4(const double* b) {
    const double inf = __builtin_huge_val();
    return fabs(b[0]) < inf && fabs(b[1]) < inf && fabs(b[2]) < inf && fabs(b[3]) < inf;       // NaN fails every comparison
}

struct Args {
    const double* det_boxes;
    const double* det_vars;
    const double* det_lp;
    const int32_t* det_off;
    const double* gt_boxes;
    const int32_t* gt_cls;
    const int32_t* gt_crowd;
    const int32_t* gt_off;
    const int32_t* image_hw;
    const long long* pair_off;
    int B, K, M, G;
    long long pairs;
    int entries;          // the LDS tables hold this many: an image with W + H above it is not walked
    double cx, cy;        // sqrt(1 / wx^2 + 1 / (4 ww^2)), sqrt(1 / wy^2 + 1 / (4 wh^2))
    double tau;
    double* q;
    double* fg;
    double* bg;
    double* label;
    int32_t* gt_live;
    int32_t* flags;       // [4]: pe::flag_excluded over the detections, then over the ground truths
};

// the image of row r under offsets [B + 1]: the b with off[b] <= r < off[b + 1], or -1 (offsets that do not rise)
__device__ __forceinline__ int image_of(const int32_t* off, int B, int r) {
    int lo = 0, hi = B;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] <= r) lo = mid + 1;
        else hi = mid;
    }
    return (lo < B && off[lo] <= r && r < off[lo + 1]) ? lo : -1;
}

// the clipped pixel rectangle [u0, u1) x [v0, v1) of a ground truth that takes part; false when it is ignored
__device__ __forceinline__ bool gt_rect(const Args& a, int g, int H, int W, int& u0, int& u1, int& v0, int& v1) {
    const double* b = a.gt_boxes + (size_t)g * 4;
    if (a.gt_crowd[g] != 0 || !finite4(b)) return false;
    const int c = a.gt_cls[g];
    if (c < 0 || c >= a.K) return false;
    u0 = first_centre_ge(b[0], W); u1 = first_centre_ge(b[2], W);
    v0 = first_centre_ge(b[1], H); v1 = first_centre_ge(b[3], H);
    return u1 > u0 && v1 > v0;
}

__device__ __forceinline__ bool image_ok(const Args& a, int b, int& H, int& W) {
    H = a.image_hw[2 * b];
    W = a.image_hw[2 * b + 1];
    return H >= 1 && W >= 1 && (long long)H + W <= a.entries;
}

__global__ __launch_bounds__(kThreads) void pdq_pair_quality_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    if ((int)blockIdx.x >= a.M) {
        // ---- the ground truths that take part: a thread each
        const long long gl = ((long long)blockIdx.x - a.M) * kThreads + t;
        if (gl >= a.G) return;
        const int g = (int)gl;
        const int b = image_of(a.gt_off, a.B, g);
        int H, W, u0, u1, v0, v1;
        const bool live = b >= 0 && image_ok(a, b, H, W) && gt_rect(a, g, H, W, u0, u1, v0, v1);
        a.gt_live[g] = live ? 1 : 0;
        if (!live) pe::flag_excluded(a.flags + 2, g);
        return;
    }
    // ---- a detection (every condition below is uniform over the workgroup)
    const int d = blockIdx.x;
    const int b = image_of(a.det_off, a.B, d);
    if (b < 0) return;
    const int d0 = a.det_off[b], d1 = a.det_off[b + 1], g0 = a.gt_off[b], g1 = a.gt_off[b + 1];
    const long long po = a.pair_off[b];
    const int Mb = d1 - d0, Gb = g1 - g0;
    // offsets that would leave the tables: nothing of this image is read or written
    if (d0 < 0 || d1 > a.M || g0 < 0 || g1 > a.G || Gb < 0 || po < 0 || po + (long long)Gb * Mb > a.pairs) return;
    const long long pair0 = po + (d - d0);

    int H, W;
    const bool img = image_ok(a, b, H, W);
    const double* box = a.det_boxes + (size_t)d * 4;
    const double x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3], var = a.det_vars[d];
    const double bw = x2 - x1, bh = y2 - y1;
    const bool ok = img && finite4(box) && bw > 0.0 && bh > 0.0 && var >= 0.0 && var < __builtin_huge_val();
    if (!ok) {
        for (int k = t; k < Gb; k += kThreads) {
            const long long p = pair0 + (long long)k * Mb;
            a.q[p] = 0.0; a.fg[p] = 0.0; a.bg[p] = 0.0; a.label[p] = 0.0;
        }
        if (t == 0) pe::flag_excluded(a.flags, d);
        return;
    }

    double (*red)[2] = reinterpret_cast<double (*)[2]>(smem);                 // [256][2]
    int* win = reinterpret_cast<int*>(smem + kThreads * 2 * sizeof(double));    // [4] (16 bytes)
    double* px = reinterpret_cast<double*>(smem + kThreads * 2 * sizeof(double) + 16);
    double* qx = px + W;
    double* py = qx + W;
    double* qy = py + H;

    // ---- phase 1: the four tables and the window of px > tau, py > tau
    if (t == 0) { win[0] = W; win[1] = -1; win[2] = H; win[3] = -1; }
    __syncthreads();
    const double sd = sqrt(var);
    const double sx = sd * bw * a.cx, sy = sd * bh * a.cy;
    for (int i = t; i < W + H; i += kThreads) {
        double p, q;
        if (i < W) {
            axis_entry(i, x1, x2, sx, p, q);
            px[i] = p; qx[i] = q;
            if (p > a.tau) { atomicMin(&win[0], i); atomicMax(&win[1], i); }
        } else {
            const int v = i - W;
            axis_entry(v, y1, y2, sy, p, q);
            py[v] = p; qy[v] = q;
            if (p > a.tau) { atomicMin(&win[2], v); atomicMax(&win[3], v); }
        }
    }
    __syncthreads();
    const int wu0 = win[0], wu1 = win[1] + 1, wv0 = win[2], wv1 = win[3] + 1;      // empty: wu1 <= wu0 or wv1 <= wv0
    const int ww = max(wu1 - wu0, 0), wh = max(wv1 - wv0, 0);

    // ---- phase 2: B_all over the window
    double ball = 0.0;
    {
        double s = 0.0;
        const int n = ww * wh;           // W * H <= (PE_PDQ_MAX_TABLE / 2)^2: an int holds it
        for (int i = t; i < n; i += kThreads) {
            const int v = wv0 + i / ww, u = wu0 + i % ww;
            const double P = px[u] * py[v];
            if (P > a.tau) s += term_bg(P, qx[u] + px[u] * qy[v]);
        }
        red[t][0] = s; red[t][1] = 0.0;
        pe::block_tree(red, kThreads);
        __syncthreads();
        ball = red[0][0];
    }

    // ---- phase 3: the ground truths of the image, over their own rectangles
    for (int k = 0; k < Gb; ++k) {
        const int g = g0 + k;
        const long long p = pair0 + (long long)k * Mb;
        int u0, u1, v0, v1;
        if (!gt_rect(a, g, H, W, u0, u1, v0, v1)) {
            if (t == 0) { a.q[p] = 0.0; a.fg[p] = 0.0; a.bg[p] = 0.0; a.label[p] = 0.0; }
            continue;
        }
        const int rw = u1 - u0;
        const int n = rw * (v1 - v0);
        double f = 0.0, bin = 0.0;
        for (int i = t; i < n; i += kThreads) {
            const int v = v0 + i / rw, u = u0 + i % rw;
            const double P = px[u] * py[v], Q = qx[u] + px[u] * qy[v];
            f += term_fg(P, Q);
            if (P > a.tau) bin += term_bg(P, Q);
        }
        __syncthreads();                 // the previous round's red[0] has been read
        red[t][0] = f; red[t][1] = bin;
        pe::block_tree(red, kThreads);
        if (t == 0) {
            const double FG = red[0][0] / (double)n;
            // a window inside the rectangle leaves no background pixel: the empty sum, not the difference of two equal ones
            const bool inside = ww == 0 || wh == 0 || (wu0 >= u0 && wu1 <= u1 && wv0 >= v0 && wv1 <= v1);
            const double BG = inside ? 0.0 : (ball - red[0][1]) / (double)n;
            const double QL = exp(a.det_lp[(size_t)d * (a.K + 1) + a.gt_cls[g]]);
            a.q[p] = sqrt(exp(FG + BG) * QL);
            a.fg[p] = exp(FG);
            a.bg[p] = exp(BG);
            a.label[p] = QL;
        }
    }
}

// tests only (csrc/test_hooks.h): the two terms of n pixels from their four arguments, through the functions the kernel above calls
__global__ __launch_bounds__(kThreads) void pdq_terms_kernel(const double* ax, const double* bx, const double* ay, const double* by, long long n,
                                                             double* out_fg, double* out_bg) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    double pxi, qxi, pyi, qyi;
    axis_soft(ax[i], bx[i], pxi, qxi);
    axis_soft(ay[i], by[i], pyi, qyi);
    const double P = pxi * pyi, Q = qxi + pxi * qyi;
    out_fg[i] = term_fg(P, Q);
    out_bg[i] = term_bg(P, Q);
}

}  // namespace

extern "C" int pe_pdq_pair_quality(const double* det_boxes, const double* det_vars, const double* det_log_probs, const int32_t* det_offsets,
                                   const double* gt_boxes, const int32_t* gt_classes, const int32_t* gt_crowd, const int32_t* gt_offsets,
                                   const int32_t* image_hw, const int64_t* pair_offsets, int32_t num_images, int32_t num_classes,
                                   int32_t num_dets, int32_t num_gt, int64_t num_pairs, int32_t max_width_plus_height,
                                   const float* bbox_reg_weights_host, double tau, double* out_q, double* out_fg, double* out_bg,
                                   double* out_label, int32_t* out_gt_live, int32_t* out_flags, void* stream) {
    PE_CHECK_ARG(num_images >= 0 && num_dets >= 0 && num_gt >= 0 && num_pairs >= 0,
                 "pe_pdq_pair_quality: num_images %d, num_dets %d, num_gt %d, num_pairs %lld: a negative count", num_images, num_dets, num_gt,
                 (long long)num_pairs);
    PE_CHECK_ARG(num_classes >= 1, "pe_pdq_pair_quality: num_classes %d", num_classes);
    PE_CHECK_ARG(tau >= 0.0 && tau < 1.0, "pe_pdq_pair_quality: tau %g is not in [0, 1)", tau);
    PE_CHECK_ARG(max_width_plus_height >= 0, "pe_pdq_pair_quality: max_width_plus_height %d", max_width_plus_height);
    PE_CHECK_ARG(max_width_plus_height <= PE_PDQ_MAX_TABLE,
                 "pe_pdq_pair_quality: W + H = %d is above %d: the four tables of a detection (16 bytes per column and per row) are kept in 64 KiB "
                 "of LDS", max_width_plus_height, PE_PDQ_MAX_TABLE);
    PE_CHECK_ARG(out_flags, "pe_pdq_pair_quality: null pointer (out_flags)");
    PE_CHECK_ARG(num_images == 0 || (det_offsets && gt_offsets && image_hw && pair_offsets),
                 "pe_pdq_pair_quality: null pointer (det_offsets / gt_offsets / image_hw / pair_offsets)");
    PE_CHECK_ARG(num_dets == 0 || (num_images > 0 && det_boxes && det_vars && det_log_probs),
                 "pe_pdq_pair_quality: null pointer (det_boxes / det_vars / det_log_probs), or detections without images");
    PE_CHECK_ARG(num_gt == 0 || (num_images > 0 && gt_boxes && gt_classes && gt_crowd && out_gt_live),
                 "pe_pdq_pair_quality: null pointer (gt_boxes / gt_classes / gt_crowd / out_gt_live), or ground truth without images");
    PE_CHECK_ARG(num_pairs == 0 || (out_q && out_fg && out_bg && out_label), "pe_pdq_pair_quality: null output (q / fg / bg / label)");
    PE_CHECK_ARG(num_pairs <= (int64_t)num_dets * num_gt, "pe_pdq_pair_quality: num_pairs %lld for %d detections and %d ground truths",
                 (long long)num_pairs, num_dets, num_gt);
    Args a{};
    double w[4];
    if (int rc = pe::bbox_reg_weights(bbox_reg_weights_host, w, "pe_pdq_pair_quality")) return rc;
    a.cx = sqrt(1.0 / (w[0] * w[0]) + 1.0 / (4.0 * (w[2] * w[2])));
    a.cy = sqrt(1.0 / (w[1] * w[1]) + 1.0 / (4.0 * (w[3] * w[3])));
    a.det_boxes = det_boxes; a.det_vars = det_vars; a.det_lp = det_log_probs; a.det_off = det_offsets;
    a.gt_boxes = gt_boxes; a.gt_cls = gt_classes; a.gt_crowd = gt_crowd; a.gt_off = gt_offsets;
    a.image_hw = image_hw; a.pair_off = (const long long*)pair_offsets;
    a.B = num_images; a.K = num_classes; a.M = num_dets; a.G = num_gt; a.pairs = num_pairs;
    a.entries = max_width_plus_height; a.tau = tau;
    a.q = out_q; a.fg = out_fg; a.bg = out_bg; a.label = out_label; a.gt_live = out_gt_live; a.flags = out_flags;
    const size_t lds = kThreads * 2 * sizeof(double) + 16 + 2 * sizeof(double) * (size_t)max_width_plus_height;
    PE_ENSURE_LDS(pdq_pair_quality_kernel, lds, "pe_pdq_pair_quality");
    if (hipMemsetAsync(out_flags, 0, 4 * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
        pe::set_error("pe_pdq_pair_quality: hipMemsetAsync of the flags failed");
        return PE_ERR_HIP;
    }
    const long long blocks = (long long)num_dets + (num_gt + kThreads - 1) / kThreads;
    if (blocks == 0) return PE_OK;
    hipLaunchKernelGGL(pdq_pair_quality_kernel, dim3((unsigned)blocks), dim3(kThreads), lds, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH("pe_pdq_pair_quality");
    return PE_OK;
}

extern "C" int pe_test_pdq_terms(const double* ax, const double* bx, const double* ay, const double* by, long long n, double* out_fg,
                                 double* out_bg, void* stream) {
    PE_CHECK_ARG(n >= 0, "pe_test_pdq_terms: n %lld", n);
    if (n == 0) return PE_OK;
    PE_CHECK_ARG(ax && bx && ay && by && out_fg && out_bg, "pe_test_pdq_terms: null pointer");
    hipLaunchKernelGGL(pdq_terms_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, ax, bx, ay, by,
                       n, out_fg, out_bg);
    PE_CHECK_LAUNCH("pe_test_pdq_terms");
    return PE_OK;
}
