// Variance calibration of the detectors' box heads (gfx950): one positive scale s_d per detector, variance' = s_d * variance.
//   pe_match_ground_truth      : detections -> (label, matched ground-truth index, best IoU), batched over images
//   pe_variance_stats          : the sufficient statistics of the Gaussian NLL of the matched rows' box-delta residuals
// (the scale is applied where the rows are packed: pe_proben_pack_calibrated, csrc/pack.hip)
//
// Matching is calibration.match_labels / finetune.pairwise_iou in float64, in that expression order (built with -ffp-contract=off,
// so no multiply-add is fused): area = (x2 - x1) * (y2 - y1), w = max(min(ax2, bx2) - max(ax1, bx1), 0), inter = w * h,
// union = (area_a + area_b) - inter, IoU = inter > 0 ? inter / union : 0.  Every operation is one IEEE float64 operation on both
// sides, so the IoU is the same bits.  Boxes are expected finite (a NaN coordinate never wins here; torch's max would return it).
//
// The statistics are reduced without floating-point atomics: a thread adds its rows in row order (row r belongs to thread r mod
// (blocks * 256)), the workgroup adds its 256 threads in a stride-halving tree, the second kernel adds the (at most 1 024) workgroup
// partials in the same tree.  The grid is a function of the row count alone: same input, same bits.
#include "common.h"
#define PE_REDUCE2_FLAGS_ONLY          // the flags, not the finish kernel: see the note at variance_stats_finish_kernel
#include "reduce2.h"
#include "box_residual.h"

namespace {

constexpr int kMatchThreads = 256;
constexpr int kMatchChunk = 512;          // ground-truth boxes staged in LDS at a time: 512 * (5 * 8 + 4) = 22 KiB

// A workgroup per image, a thread per detection (tiles of 256 when an image has more), the image's ground truth staged in LDS in
// chunks of kMatchChunk: every lane reads the same LDS address (broadcast).  All loop bounds are workgroup-uniform.
__global__ __launch_bounds__(kMatchThreads) void match_ground_truth_kernel(const double* det, const int32_t* det_off, const double* gt,
                                                                           const int32_t* gt_off, const int32_t* gt_cls,
                                                                           const int32_t* gt_crowd, double thresh, int num_classes,
                                                                           int32_t* out_label, int32_t* out_match, double* out_iou) {
    __shared__ double gx1[kMatchChunk], gy1[kMatchChunk], gx2[kMatchChunk], gy2[kMatchChunk], garea[kMatchChunk];
    __shared__ int32_t glive[kMatchChunk];
    const int b = blockIdx.x;
    const int d0 = det_off[b], d1 = det_off[b + 1], g0 = gt_off[b], g1 = gt_off[b + 1];
    for (int tile = d0; tile < d1; tile += kMatchThreads) {
        const int i = tile + (int)threadIdx.x;
        const bool live = i < d1;
        double ax1 = 0, ay1 = 0, ax2 = 0, ay2 = 0, area_a = 0;
        if (live) {
            ax1 = det[(size_t)i * 4]; ay1 = det[(size_t)i * 4 + 1]; ax2 = det[(size_t)i * 4 + 2]; ay2 = det[(size_t)i * 4 + 3];
            area_a = (ax2 - ax1) * (ay2 - ay1);
        }
        double best = -1.0;             // an IoU is >= 0: the first ground-truth box that takes part always replaces this
        int best_g = -1;
        for (int c0 = g0; c0 < g1; c0 += kMatchChunk) {
            const int n = min(kMatchChunk, g1 - c0);
            __syncthreads();            // the previous chunk (or tile) has been read by every thread
            for (int k = threadIdx.x; k < n; k += kMatchThreads) {
                const size_t g = (size_t)(c0 + k);
                const double x1 = gt[g * 4], y1 = gt[g * 4 + 1], x2 = gt[g * 4 + 2], y2 = gt[g * 4 + 3];
                gx1[k] = x1; gy1[k] = y1; gx2[k] = x2; gy2[k] = y2;
                garea[k] = (x2 - x1) * (y2 - y1);
                glive[k] = gt_crowd ? (gt_crowd[g] == 0) : 1;
            }
            __syncthreads();
            if (live) {
                for (int k = 0; k < n; ++k) {
                    if (!glive[k]) continue;
                    const double w = fmax(fmin(ax2, gx2[k]) - fmax(ax1, gx1[k]), 0.0);
                    const double h = fmax(fmin(ay2, gy2[k]) - fmax(ay1, gy1[k]), 0.0);
                    const double inter = w * h;
                    const double uni = area_a + garea[k] - inter;
                    const double iou = inter > 0.0 ? inter / uni : 0.0;
                    if (iou > best) { best = iou; best_g = c0 + k; }      // strict: the lowest index keeps an equal maximum
                }
            }
        }
        if (live) {
            const bool hit = best_g >= 0 && best >= thresh;
            out_label[i] = hit ? gt_cls[best_g] : num_classes;
            out_match[i] = hit ? best_g : -1;
            out_iou[i] = best_g >= 0 ? best : 0.0;
        }
    }
}

constexpr int kStatThreads = 256;
constexpr int kStatValues = 5;            // n, sum q, sum log var, coverage at 1 sigma, coverage at 2 sigma

struct StatArgs {
    const double* det;
    const int32_t* match;
    const double* gt;
    const double* var;
    long long M, G;
    double w[4];
    double s;
    double* partial;      // [blocks, 5]
    int32_t* flags;       // pe::flag_excluded (csrc/reduce2.h): excluded rows
};

__global__ __launch_bounds__(kStatThreads) void variance_stats_kernel(StatArgs a) {
    __shared__ double x[kStatThreads][kStatValues];
    double n = 0.0, sq = 0.0, sl = 0.0, c1 = 0.0, c2 = 0.0;
    const long long step = (long long)gridDim.x * kStatThreads;
    for (long long r = (long long)blockIdx.x * kStatThreads + threadIdx.x; r < a.M; r += step) {
        const int m = a.match[r];
        const double v = a.var[r];
        bool ok = m >= 0 && m < a.G && v > 0.0 && v < __builtin_huge_val();       // NaN fails v > 0; an index beyond the table is never read
        double res[4];
        if (ok) ok = pe::box_residual(a.det + r * 4, a.gt + (size_t)m * 4, a.w, res);
        if (!ok) {
            pe::flag_excluded(a.flags, r);
            continue;
        }
        const double sv = a.s * v, sv4 = 4.0 * sv;
        double q = 0.0;
        for (int c = 0; c < 4; ++c) {
            const double r2 = res[c] * res[c];
            q += r2 / v;
            c1 += r2 <= sv ? 1.0 : 0.0;
            c2 += r2 <= sv4 ? 1.0 : 0.0;
        }
        n += 1.0;
        sq += q;
        sl += log(v);
    }
    x[threadIdx.x][0] = n; x[threadIdx.x][1] = sq; x[threadIdx.x][2] = sl; x[threadIdx.x][3] = c1; x[threadIdx.x][4] = c2;
    pe::block_tree(x, kStatThreads);
    if (threadIdx.x == 0)
        for (int v = 0; v < kStatValues; ++v) a.partial[(size_t)blockIdx.x * kStatValues + v] = x[0][v];
}

// second pass, one workgroup: thread k holds workgroup k's partial (0 beyond the grid: adding it is exact), 1 024 -> 1 in the same tree
// (not pe::launch_finish of csrc/reduce2.h: its segment order would change the low bits of sum_q and sum_log_var)
__global__ __launch_bounds__(PE_VARIANCE_STATS_MAX_BLOCKS) void variance_stats_finish_kernel(const double* partial, int blocks,
                                                                                             double* out) {
    __shared__ double x[PE_VARIANCE_STATS_MAX_BLOCKS][kStatValues];
    for (int v = 0; v < kStatValues; ++v)
        x[threadIdx.x][v] = (int)threadIdx.x < blocks ? partial[(size_t)threadIdx.x * kStatValues + v] : 0.0;
    pe::block_tree(x, PE_VARIANCE_STATS_MAX_BLOCKS);
    if (threadIdx.x == 0)
        for (int v = 0; v < kStatValues; ++v) out[v] = x[0][v];
}

}  // namespace

extern "C" int pe_match_ground_truth(const double* det_boxes, const int32_t* det_offsets, const double* gt_boxes,
                                     const int32_t* gt_offsets, const int32_t* gt_classes, const int32_t* gt_crowd,
                                     int32_t num_images, double iou_thresh, int32_t num_classes, int32_t* out_labels,
                                     int32_t* out_match, double* out_iou, void* stream) {
    PE_CHECK_ARG(num_images >= 0, "pe_match_ground_truth: num_images %d", num_images);
    PE_CHECK_ARG(num_classes >= 1, "pe_match_ground_truth: num_classes %d", num_classes);
    PE_CHECK_ARG(iou_thresh == iou_thresh, "pe_match_ground_truth: iou_thresh %g", iou_thresh);
    if (num_images == 0) return PE_OK;
    PE_CHECK_ARG(det_offsets && gt_offsets, "pe_match_ground_truth: null pointer (det_offsets / gt_offsets)");
    // images without detections or without ground truth are legal, so the row pointers may belong to empty tensors: they are only
    // dereferenced inside [offsets[b], offsets[b + 1]); the outputs are per detection
    PE_CHECK_ARG(det_boxes && gt_boxes && gt_classes, "pe_match_ground_truth: null pointer (det_boxes / gt_boxes / gt_classes)");
    PE_CHECK_ARG(out_labels && out_match && out_iou, "pe_match_ground_truth: null output");
    hipLaunchKernelGGL(match_ground_truth_kernel, dim3(num_images), dim3(kMatchThreads), 0, (hipStream_t)stream, det_boxes, det_offsets,
                       gt_boxes, gt_offsets, gt_classes, gt_crowd, iou_thresh, (int)num_classes, out_labels, out_match, out_iou);
    PE_CHECK_LAUNCH("pe_match_ground_truth");
    return PE_OK;
}

extern "C" int pe_variance_stats(const double* det_boxes, const int32_t* match, const double* gt_boxes, const double* variances,
                                 int64_t num_rows, int64_t num_gt, const float* bbox_reg_weights_host, double scale, double* workspace, double* out,
                                 int32_t* out_flags, void* stream) {
    PE_CHECK_ARG(pe::finite_positive(scale), "pe_variance_stats: scale %g is not finite and > 0", scale);
    PE_CHECK_ARG(num_rows >= 0 && num_gt >= 0, "pe_variance_stats: num_rows %lld, num_gt %lld", (long long)num_rows, (long long)num_gt);
    PE_CHECK_ARG(workspace && out && out_flags, "pe_variance_stats: null pointer (workspace / out / out_flags)");
    PE_CHECK_ARG(num_rows == 0 || (det_boxes && match && variances && (gt_boxes || num_gt == 0)),
                 "pe_variance_stats: null pointer (det_boxes / match / gt_boxes / variances)");
    StatArgs a{};
    if (int rc = pe::bbox_reg_weights(bbox_reg_weights_host, a.w, "pe_variance_stats")) return rc;
    a.det = det_boxes; a.match = match; a.gt = gt_boxes; a.var = variances; a.M = num_rows; a.G = num_gt; a.s = scale;
    a.partial = workspace; a.flags = out_flags;
    // the grid is a function of num_rows alone: same input, same partition, same bits
    const int blocks = (int)std::max<long long>(1, std::min<long long>((num_rows + kStatThreads - 1) / kStatThreads,
                                                                        PE_VARIANCE_STATS_MAX_BLOCKS));
    if (int st = pe::zero_flags(out_flags, (hipStream_t)stream, "pe_variance_stats")) return st;
    hipLaunchKernelGGL(variance_stats_kernel, dim3(blocks), dim3(kStatThreads), 0, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH("pe_variance_stats");
    hipLaunchKernelGGL(variance_stats_finish_kernel, dim3(1), dim3(PE_VARIANCE_STATS_MAX_BLOCKS), 0, (hipStream_t)stream, workspace, blocks,
                       out);
    PE_CHECK_LAUNCH("pe_variance_stats (finish)");
    return PE_OK;
}
