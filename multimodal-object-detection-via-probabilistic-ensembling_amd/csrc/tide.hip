// TIDE error typing per image (gfx950): Bolya, Foley, Hays, Hoffman, "TIDE: A General Toolbox for Identifying Object Detection
// Errors", ECCV 2020, restated for this project's evaluator.  DESIGN.md 32 states the rule (steps A to D) and include/proben_hip.h the
// layout; tests/tide_ref.py restates it in NumPy.
//
// One workgroup of four wavefronts per image; nothing is shared between workgroups.  The image's ground truths (box, category, crowd
// flag) and their state live in LDS, the detections stay in global memory in the caller's total order.
//   A. base matching, csrc/cocoeval.cpp eval_pair at t_f and area range 0: a wavefront per category walks that category's detections
//      in order (a ballot over 64 detections' categories finds them), serial as the rule is.  Lanes take the ground truths; the wave
//      reduction carries (IoU, index) under eval_pair's rule: the largest IoU not below the threshold, the LATER ground truth on a
//      tie, regular ground truths before crowd ones.  eval_pair's `v < best` lets a NaN IoU through and then everything after it:
//      with a NaN among the candidates the last candidate wins, whatever its IoU - kept, because the rule is eval_pair's.
//      Categories own disjoint ground truths, so the wavefronts do not meet.
//   B. a wavefront per unmatched detection: the plain IoU against the non-crowd ground truths, two max reductions (own class, other
//      classes) in which the LOWEST index wins a tie; the type by the priority Loc, Cls, Dupe, Bkg, Both.
//   C. a thread per ground truth: matched / covered by a Loc error / covered by a Cls error / missed.
//   D. wavefront 0 walks the Loc errors and wavefront 1 the Cls errors, each in the total order: an error claims its partner if A
//      left it unmatched and no earlier error of the same walk holds it.
// float64, built with -ffp-contract=off: every comparison is the NumPy restatement's.  No floating-point atomics.
#include "common.h"

namespace {

constexpr int kWaves = 4, kThreads = 64 * kWaves;
enum : int { kTP = 0, kCls = 1, kLoc = 2, kBoth = 3, kDupe = 4, kBkg = 5, kIgnored = 6 };
enum : int { kGtMatched = 1, kGtLoc = 2, kGtCls = 4, kGtMissed = 8 };

struct TideArgs {
    const double* det_box;
    const int32_t* det_cat;
    const int32_t* det_off;      // device copy [B + 1]
    const double* gt_box;
    const int32_t* gt_cat;
    const uint8_t* gt_crowd;
    const int32_t* gt_off;       // device copy [B + 1]
    int K, num_dets, num_gt;
    double t_f, t_b;
    int32_t* out_match;
    int32_t* out_type;
    int32_t* out_partner;
    int32_t* out_claim;
    int32_t* out_gt;
};

// "x beats the holder" of the two reductions; an index below 0 holds nothing
__device__ __forceinline__ bool later_wins(double xv, int xi, double v, int i) { return xi >= 0 && (i < 0 || xv > v || (xv == v && xi > i)); }
__device__ __forceinline__ bool lower_wins(double xv, int xi, double v, int i) { return xi >= 0 && (i < 0 || xv > v || (xv == v && xi < i)); }

__device__ __forceinline__ void reduce_later(double& v, int& i) {
    for (int o = 32; o > 0; o >>= 1) {
        const double xv = __shfl_xor(v, o);
        const int xi = __shfl_xor(i, o);
        if (later_wins(xv, xi, v, i)) { v = xv; i = xi; }
    }
}
__device__ __forceinline__ void reduce_lower(double& v, int& i) {
    for (int o = 32; o > 0; o >>= 1) {
        const double xv = __shfl_xor(v, o);
        const int xi = __shfl_xor(i, o);
        if (lower_wins(xv, xi, v, i)) { v = xv; i = xi; }
    }
}
__device__ __forceinline__ int reduce_max(int i) {
    for (int o = 32; o > 0; o >>= 1) i = max(i, __shfl_xor(i, o));
    return i;
}

// eval_pair's fold over the candidates of one group (regular or crowd) spread over the lanes: the ground truth it ends on, or -1
struct Fold {
    double v = 0.0;
    int i = -1, last = -1;
    bool nan = false;
    __device__ __forceinline__ void take(double x, int g, double thr) {
        last = g;
        if (x != x) nan = true;
        else if (x >= thr && (i < 0 || x >= v)) { v = x; i = g; }
    }
    __device__ __forceinline__ int finish() {
        if (__ballot(nan) != 0ull) return reduce_max(last);
        reduce_later(v, i);
        return i;
    }
};

__global__ __launch_bounds__(kThreads) void tide_kernel(TideArgs a) {
    __shared__ double gbox[PE_TIDE_MAX_GT * 4];
    __shared__ int gcat[PE_TIDE_MAX_GT];
    __shared__ int gmatch[PE_TIDE_MAX_GT];       // the image-local detection A matched it to (a crowd box: the last one), or -1
    __shared__ int gstate[PE_TIDE_MAX_GT];       // kGtLoc | kGtCls
    __shared__ uint8_t gcrowd[PE_TIDE_MAX_GT];
    __shared__ uint8_t gclaim[2][PE_TIDE_MAX_GT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int d0 = a.det_off[b], d1 = a.det_off[b + 1], g0 = a.gt_off[b], g1 = a.gt_off[b + 1];
    const int D = d1 - d0, G = g1 - g0;
    // the wrapper checked the host offsets these are a copy of: an image that would leave the arrays or the LDS is left unwritten
    if (d0 < 0 || D < 0 || d1 > a.num_dets || D > PE_TIDE_MAX_DETS || g0 < 0 || G < 0 || g1 > a.num_gt || G > PE_TIDE_MAX_GT) return;

    for (int g = tid; g < G; g += kThreads) {
        for (int c = 0; c < 4; ++c) gbox[g * 4 + c] = a.gt_box[(size_t)(g0 + g) * 4 + c];
        gcat[g] = a.gt_cat[g0 + g];
        gcrowd[g] = a.gt_crowd[g0 + g] != 0;
        gmatch[g] = -1;
        gstate[g] = 0;
        gclaim[0][g] = gclaim[1][g] = 0;
    }
    for (int d = tid; d < D; d += kThreads) {
        a.out_match[d0 + d] = -1;
        a.out_type[d0 + d] = kBkg;
        a.out_partner[d0 + d] = -1;
        a.out_claim[d0 + d] = 0;
    }
    __syncthreads();

    // A
    const double thr = fmin(a.t_f, 1 - 1e-10);
    for (int k = wave; k < a.K; k += kWaves) {
        bool has = false;
        for (int g = lane; g < G; g += 64) has |= gcat[g] == k;
        if (__ballot(has) == 0ull) continue;                      // wave-uniform: its detections stay unmatched
        for (int c = 0; c < D; c += 64) {
            const int cat = c + lane < D ? a.det_cat[d0 + c + lane] : -1;
            unsigned long long todo = __ballot(cat == k);
            while (todo) {
                const int d = c + __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const double* db = a.det_box + (size_t)(d0 + d) * 4;
                const double dx = db[0], dy = db[1], dw = db[2], dh = db[3], da = dw * dh;
                Fold regular, crowd;
                for (int g = lane; g < G; g += 64) {
                    if (gcat[g] != k) continue;
                    const bool cr = gcrowd[g];
                    if (!cr && gmatch[g] >= 0) continue;
                    const double gx = gbox[g * 4], gy = gbox[g * 4 + 1], gw = gbox[g * 4 + 2], gh = gbox[g * 4 + 3], ga = gw * gh;
                    const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx), h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
                    const double inter = (w <= 0 || h <= 0) ? 0.0 : w * h;
                    const double uni = cr ? da : da + ga - inter;
                    (cr ? crowd : regular).take(inter / uni, g, thr);
                }
                int m = regular.finish();
                if (m < 0) m = crowd.finish();                    // wave-uniform
                if (m >= 0) {
                    gmatch[m] = d;                                // every lane stores the same value: the next walk of this wave sees it
                    if (lane == 0) {
                        a.out_match[d0 + d] = m;
                        a.out_type[d0 + d] = gcrowd[m] ? kIgnored : kTP;
                    }
                }
            }
        }
    }
    __syncthreads();

    // B
    for (int d = wave; d < D; d += kWaves) {
        if (a.out_match[d0 + d] >= 0) continue;                   // wave-uniform
        const int k = a.det_cat[d0 + d];
        const double* db = a.det_box + (size_t)(d0 + d) * 4;
        const double dx = db[0], dy = db[1], dw = db[2], dh = db[3], da = dw * dh;
        double own = 0.0, other = 0.0;
        int own_g = -1, other_g = -1;
        for (int g = lane; g < G; g += 64) {
            if (gcrowd[g]) continue;
            const double gx = gbox[g * 4], gy = gbox[g * 4 + 1], gw = gbox[g * 4 + 2], gh = gbox[g * 4 + 3], ga = gw * gh;
            const double w = fmin(dx + dw, gx + gw) - fmax(dx, gx), h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
            const double inter = (w <= 0 || h <= 0) ? 0.0 : w * h;
            const double v = inter > 0 ? inter / (da + ga - inter) : 0.0;
            if (!(v >= 0)) continue;                              // a NaN or a negative quotient of degenerate boxes holds nothing
            if (gcat[g] == k) {
                if (own_g < 0 || v > own) { own = v; own_g = g; }
            } else if (other_g < 0 || v > other) { other = v; other_g = g; }
        }
        reduce_lower(own, own_g);
        reduce_lower(other, other_g);
        if (own_g < 0) own = 0.0;
        if (other_g < 0) other = 0.0;
        int type, partner = -1;
        if (a.t_b <= own && own < a.t_f) { type = kLoc; partner = own_g; }
        else if (other >= a.t_f) { type = kCls; partner = other_g; }
        else if (own >= a.t_f) { type = kDupe; partner = own_g; }
        else if (other < a.t_b) type = kBkg;
        else type = kBoth;
        if (lane == 0) {
            a.out_type[d0 + d] = type;
            a.out_partner[d0 + d] = partner;
            if (partner >= 0 && type == kLoc) atomicOr(&gstate[partner], kGtLoc);
            if (partner >= 0 && type == kCls) atomicOr(&gstate[partner], kGtCls);
        }
    }
    __syncthreads();

    // C
    for (int g = tid; g < G; g += kThreads) {
        const int matched = gmatch[g] >= 0, cover = gstate[g] & (kGtLoc | kGtCls);
        a.out_gt[g0 + g] = (matched ? kGtMatched : 0) | cover | ((!gcrowd[g] && !matched && !cover) ? kGtMissed : 0);
    }

    // D
    if (wave < 2) {
        const int want = wave == 0 ? kLoc : kCls;
        uint8_t* held = gclaim[wave];
        for (int c = 0; c < D; c += 64) {
            const int d = c + lane;
            const int type = d < D ? a.out_type[d0 + d] : -1;
            const int p = type == want ? a.out_partner[d0 + d] : -1;
            unsigned long long todo = __ballot(p >= 0 && p < G && gmatch[p] < 0);
            bool mine = false;
            while (todo) {
                const int bit = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int pp = __shfl(p, bit);
                if (held[pp] == 0) {                              // wave-uniform
                    held[pp] = 1;
                    mine |= lane == bit;
                }
            }
            if (mine) a.out_claim[d0 + d] = 1;
        }
    }
}

}  // namespace

extern "C" int pe_tide_classify(const double* det_boxes, const int32_t* det_cats, const int32_t* det_offsets_host, const double* gt_boxes,
                                const int32_t* gt_cats, const uint8_t* gt_crowd, const int32_t* gt_offsets_host, int32_t num_images,
                                int32_t num_classes, int32_t num_dets, int32_t num_gt, double t_f, double t_b, int32_t* offsets_ws,
                                int32_t* out_match, int32_t* out_type, int32_t* out_partner, int32_t* out_claim, int32_t* out_gt,
                                void* stream) {
    const char* what = "pe_tide_classify";
    PE_CHECK_ARG(num_images >= 0 && num_classes >= 1 && num_dets >= 0 && num_gt >= 0, "%s: bad sizes (num_images %d, num_classes %d, num_dets %d, num_gt %d)",
                 what, num_images, num_classes, num_dets, num_gt);
    PE_CHECK_ARG(t_b >= 0.0 && t_b < t_f && t_f <= 1.0, "%s: thresholds t_b %g, t_f %g are not in 0 <= t_b < t_f <= 1", what, t_b, t_f);
    if (num_classes > PE_TIDE_MAX_CLASSES) {
        pe::set_error("%s: %d classes, at most %d", what, num_classes, PE_TIDE_MAX_CLASSES);
        return PE_ERR_UNSUPPORTED;
    }
    if (num_images == 0) return PE_OK;
    PE_CHECK_ARG(det_offsets_host && gt_offsets_host && offsets_ws, "%s: null pointer (det_offsets_host / gt_offsets_host / offsets_ws)", what);
    PE_CHECK_ARG(num_dets == 0 || (det_boxes && det_cats && out_match && out_type && out_partner && out_claim),
                 "%s: null pointer (det_boxes / det_cats / out_match / out_type / out_partner / out_claim)", what);
    PE_CHECK_ARG(num_gt == 0 || (gt_boxes && gt_cats && gt_crowd && out_gt), "%s: null pointer (gt_boxes / gt_cats / gt_crowd / out_gt)", what);
    PE_CHECK_ARG(det_offsets_host[0] == 0 && det_offsets_host[num_images] == num_dets && gt_offsets_host[0] == 0 &&
                     gt_offsets_host[num_images] == num_gt,
                 "%s: offsets must start at 0 and end at num_dets %d / num_gt %d (det %d .. %d, gt %d .. %d)", what, num_dets, num_gt,
                 det_offsets_host[0], det_offsets_host[num_images], gt_offsets_host[0], gt_offsets_host[num_images]);
    for (int b = 0; b < num_images; ++b)
        PE_CHECK_ARG(det_offsets_host[b + 1] >= det_offsets_host[b] && gt_offsets_host[b + 1] >= gt_offsets_host[b],
                     "%s: offsets of image %d are not monotone (det %d -> %d, gt %d -> %d)", what, b, det_offsets_host[b],
                     det_offsets_host[b + 1], gt_offsets_host[b], gt_offsets_host[b + 1]);
    for (int b = 0; b < num_images; ++b) {
        const int D = det_offsets_host[b + 1] - det_offsets_host[b], G = gt_offsets_host[b + 1] - gt_offsets_host[b];
        if (D > PE_TIDE_MAX_DETS || G > PE_TIDE_MAX_GT) {
            pe::set_error("%s: image %d has %d detections and %d ground truths, at most %d and %d", what, b, D, G, PE_TIDE_MAX_DETS,
                          PE_TIDE_MAX_GT);
            return PE_ERR_UNSUPPORTED;
        }
    }
    const size_t bytes = (size_t)(num_images + 1) * sizeof(int32_t);
    hipError_t e = hipMemcpyAsync(offsets_ws, det_offsets_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpyAsync(offsets_ws + num_images + 1, gt_offsets_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) {
        pe::set_error("%s: copying the offsets failed: %s", what, hipGetErrorString(e));
        return PE_ERR_HIP;
    }
    const TideArgs args{det_boxes, det_cats, offsets_ws, gt_boxes, gt_cats, gt_crowd, offsets_ws + num_images + 1, num_classes, num_dets,
                        num_gt, t_f, t_b, out_match, out_type, out_partner, out_claim, out_gt};
    hipLaunchKernelGGL(tide_kernel, dim3((unsigned)num_images), dim3(kThreads), 0, (hipStream_t)stream, args);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}
