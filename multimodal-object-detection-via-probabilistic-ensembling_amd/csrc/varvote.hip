// Variance voting for the box head on gfx950 (He, Zhu, Wang, Savvides, Zhang: "Bounding Box Regression with Uncertainty for Accurate
// Object Detection", CVPR 2019, section 3.3): after the class-aware NMS has chosen which candidates survive, the four coordinates of
// every survivor b become the mean of its same-class candidates i with IoU(b, i) > 0, weighted by
//     w_i = p_i / var_i,   p_i = exp(-(1 - IoU(b, i))^2 / sigma_t),   var_i = exp(head[orow_i, 5K+1])   (the candidate's OWN row).
// It sits where the reference's fast_rcnn_inference_single_image (modeling/roi_heads/fast_rcnn.py:43-147) has batched_nms's keep in
// hand and gathers boxes[keep]: between pe_nms_batched and pe_boxhead_finalize, which reads the voted array in place of cand_boxes.
// The reference does not vote; the step is opt-in (rcnn.DetectorConfig.var_voting) and DESIGN.md section 31 states the rule.
//
// Arithmetic: var_i = expf(...) in float32 as boxhead_finalize_kernel computes it, then everything in float64, one IEEE operation per
// operation of the rule (built with -ffp-contract=off).  IoU is finetune.pairwise_iou's expression as in csrc/variance.hip.  A
// candidate votes only with a finite variance > 0; a kept box that is no voter of itself (bad variance, or no area) keeps its bits.
//
// One workgroup per image.  The candidates are staged in LDS in tiles of PE_VAR_VOTE_TILE (x1, y1, x2, y2, class, 1 / var: 28 bytes
// each; the variance is exponentiated once per candidate and tile); one tile holds every candidate of an image at FLIR settings, and then
// it is staged once.  A wavefront takes a kept box; lane l adds the candidates l, l + 64, ... in ascending order into five float64
// partial sums (sum w, sum w x1 .. sum w y2), which one xor-butterfly (32, 16, .. 1: a + b and b + a are the same bits, so every lane
// ends with the same sums) combines.  No atomics and nothing shared between workgroups: image n's output is a function of image n.
#include <math.h>

#include "common.h"

namespace {
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / pe::kWave;
constexpr int kTile = PE_VAR_VOTE_TILE;
constexpr int kMaxK = 80;
constexpr int kMaxCand = 16384;          // pe_nms_batched's row limit, as rcnn.py sizes cand_max
static_assert(kTile % pe::kWave == 0, "lane l must see the candidates l, l + 64, ... of every tile");

struct VoteArgs {
    const float* head;
    int head_stride, N, per_image, K, cand_max, max_det;
    const float* cand_boxes;     // [N, cand_max, 4]
    const int32_t* cand_class;   // [N, cand_max]
    const int32_t* cand_rows;    // [N, cand_max, 2] (filtered row id, original row id)
    const int32_t* cand_counts;  // [N]
    const int32_t* keep;         // [N, max_det]
    const int32_t* keep_counts;  // [N]
    double sigma_t;
    float* out_boxes;            // [N, cand_max, 4]
};

constexpr size_t kLdsBytes = (size_t)kTile * (sizeof(float4) + sizeof(double) + sizeof(int32_t));

// 1 / var of a proposal row, 0 where the row does not vote (NaN, 0, inf; an original row id outside the image's rows is never read)
__device__ __forceinline__ double inverse_variance(const VoteArgs& a, int n, int orow) {
    if (orow < 0 || orow >= a.per_image) return 0.0;
    const float v = expf(a.head[((size_t)n * a.per_image + orow) * a.head_stride + 5 * a.K + 1]);
    return (v > 0.f && v < INFINITY) ? 1.0 / (double)v : 0.0;
}

__global__ __launch_bounds__(kThreads) void boxhead_var_vote_kernel(VoteArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    float4* tbox = reinterpret_cast<float4*>(lds);
    double* tinv = reinterpret_cast<double*>(lds + (size_t)kTile * sizeof(float4));
    int32_t* tcls = reinterpret_cast<int32_t*>(lds + (size_t)kTile * (sizeof(float4) + sizeof(double)));
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = min(max(a.cand_counts[n], 0), a.cand_max);
    const int kc = min(max(a.keep_counts[n], 0), a.max_det);
    const float* in = a.cand_boxes + (size_t)n * a.cand_max * 4;
    float* out = a.out_boxes + (size_t)n * a.cand_max * 4;
    for (int e = tid; e < count * 4; e += kThreads) out[e] = in[e];
    __syncthreads();                        // a kept row's copy is in memory before the wave that votes for it writes the row again
    const int tiles = (count + kTile - 1) / kTile;
    for (int base = 0; base < kc; base += kWaves) {          // workgroup-uniform bounds: every wave stages, a live wave votes
        const int j = base + wave;
        int b = j < kc ? a.keep[(size_t)n * a.max_det + j] : -1;
        if (b < 0 || b >= count) b = -1;                     // a keep id outside the candidate list is skipped
        double bx1 = 0, by1 = 0, bx2 = 0, by2 = 0, area_b = 0, inv_b = 0;
        int cls_b = -1;
        if (b >= 0) {
            bx1 = in[b * 4]; by1 = in[b * 4 + 1]; bx2 = in[b * 4 + 2]; by2 = in[b * 4 + 3];
            area_b = (bx2 - bx1) * (by2 - by1);
            cls_b = a.cand_class[(size_t)n * a.cand_max + b];
            inv_b = inverse_variance(a, n, a.cand_rows[((size_t)n * a.cand_max + b) * 2 + 1]);
        }
        double sw = 0, sx1 = 0, sy1 = 0, sx2 = 0, sy2 = 0;
        for (int t = 0; t < tiles; ++t) {
            const int c0 = t * kTile, m = min(kTile, count - c0);
            if (tiles > 1 || base == 0) {
                __syncthreads();            // the tile in LDS has been read by every wave
                for (int k = tid; k < m; k += kThreads) {
                    const size_t c = (size_t)n * a.cand_max + c0 + k;
                    const float* q = in + (size_t)(c0 + k) * 4;
                    tbox[k] = make_float4(q[0], q[1], q[2], q[3]);
                    tcls[k] = a.cand_class[c];
                    tinv[k] = inverse_variance(a, n, a.cand_rows[c * 2 + 1]);
                }
                __syncthreads();
            }
            if (b < 0) continue;
            for (int k = lane; k < m; k += pe::kWave) {
                const double iv = tinv[k];
                if (tcls[k] != cls_b || !(iv > 0.0)) continue;
                const float4 q = tbox[k];
                const double x1 = q.x, y1 = q.y, x2 = q.z, y2 = q.w;
                const double w = fmax(fmin(bx2, x2) - fmax(bx1, x1), 0.0);
                const double h = fmax(fmin(by2, y2) - fmax(by1, y1), 0.0);
                const double inter = w * h;
                const double uni = area_b + (x2 - x1) * (y2 - y1) - inter;
                const double iou = inter > 0.0 ? inter / uni : 0.0;
                if (!(iou > 0.0)) continue;
                const double d = 1.0 - iou;
                const double wt = exp(-(d * d) / a.sigma_t) * iv;
                sw += wt; sx1 += wt * x1; sy1 += wt * y1; sx2 += wt * x2; sy2 += wt * y2;
            }
        }
        if (b < 0) continue;                // wave-uniform
        for (int o = 32; o >= 1; o >>= 1) {
            sw += __shfl_xor(sw, o); sx1 += __shfl_xor(sx1, o); sy1 += __shfl_xor(sy1, o);
            sx2 += __shfl_xor(sx2, o); sy2 += __shfl_xor(sy2, o);
        }
        // b votes for itself when its variance qualifies and IoU(b, b) > 0 by the loop's own expression; then sw >= 1 / var_b > 0
        const double self_inter = fmax(bx2 - bx1, 0.0) * fmax(by2 - by1, 0.0);
        const bool self = inv_b > 0.0 && self_inter > 0.0 && self_inter / (area_b + area_b - self_inter) > 0.0;
        if (self && lane < 4) {
            const double s = lane == 0 ? sx1 : lane == 1 ? sy1 : lane == 2 ? sx2 : sy2;
            out[b * 4 + lane] = (float)(s / sw);
        }
    }
}
}  // namespace

extern "C" int pe_boxhead_var_vote(const float* head, int32_t head_stride, int32_t N, int32_t per_image, int32_t num_classes,
                                   int32_t cand_max, int32_t max_det, const float* cand_boxes, const int32_t* cand_class,
                                   const int32_t* cand_rows, const int32_t* cand_counts, const int32_t* keep,
                                   const int32_t* keep_counts, float sigma_t, float* out_boxes, void* stream) {
    PE_CHECK_ARG(head && cand_boxes && cand_class && cand_rows && cand_counts && keep && keep_counts,
                 "pe_boxhead_var_vote: null input");
    PE_CHECK_ARG(out_boxes, "pe_boxhead_var_vote: null output");
    PE_CHECK_ARG(N >= 0 && per_image >= 1, "pe_boxhead_var_vote: N %d, per_image %d", N, per_image);
    PE_CHECK_ARG(num_classes >= 1 && num_classes <= kMaxK, "pe_boxhead_var_vote: num_classes %d not in [1,%d]", num_classes, kMaxK);
    PE_CHECK_ARG(head_stride >= 5 * num_classes + 2, "pe_boxhead_var_vote: head_stride %d < %d", head_stride, 5 * num_classes + 2);
    PE_CHECK_ARG(cand_max >= 1 && cand_max <= kMaxCand, "pe_boxhead_var_vote: cand_max %d not in [1,%d]", cand_max, kMaxCand);
    PE_CHECK_ARG(max_det >= 1, "pe_boxhead_var_vote: max_det %d", max_det);
    PE_CHECK_ARG(pe::finite_positive((double)sigma_t), "pe_boxhead_var_vote: sigma_t %g is not finite and > 0", (double)sigma_t);
    PE_CHECK_ARG(out_boxes != cand_boxes, "pe_boxhead_var_vote: out_boxes aliases cand_boxes (the vote reads every candidate's input box)");
    if (N == 0) return PE_OK;
    PE_ENSURE_LDS(boxhead_var_vote_kernel, kLdsBytes, "pe_boxhead_var_vote");
    VoteArgs a{};
    a.head = head; a.head_stride = head_stride; a.N = N; a.per_image = per_image; a.K = num_classes;
    a.cand_max = cand_max; a.max_det = max_det; a.cand_boxes = cand_boxes; a.cand_class = cand_class; a.cand_rows = cand_rows;
    a.cand_counts = cand_counts; a.keep = keep; a.keep_counts = keep_counts; a.sigma_t = (double)sigma_t; a.out_boxes = out_boxes;
    hipLaunchKernelGGL(boxhead_var_vote_kernel, dim3(N), dim3(kThreads), kLdsBytes, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH("pe_boxhead_var_vote");
    return PE_OK;
}
