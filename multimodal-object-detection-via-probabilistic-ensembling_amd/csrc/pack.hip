// The detectors' padded outputs -> ProbEn input rows (gfx950): one kernel, one host implementation, four entry points.
//   pe_proben_pack_detections     : PROBS        the float32 prob_score / scores widened to float64
//   pe_proben_pack_logits         : LOGITS       p = softmax(logits / T_d) in float64 (csrc/softmax_row.h), score = p[class]
//   pe_proben_pack_log_posteriors : LOGITS_LOGP  the same plus the row's K+1 log-posteriors (the input of pe_proben_fuse_batch_logp)
//   pe_proben_pack_calibrated     : whichever of the three its arguments select, with out_vars = (double)var * s_d
//   pe_proben_pack_pooled         : pe_proben_pack_calibrated plus out_source, the detector index of every written row
// Built with -ffp-contract=off like the other ProbEn code.
#include "common.h"
#include "softmax_row.h"

namespace {

enum PackRoute { PROBS, LOGITS, LOGITS_LOGP };

struct PackRows {
    const float* boxes[4];
    const int32_t* classes[4];
    const float* vars[4];
    const int32_t* counts[4];
    const float* cols[4];      // PROBS: prob_score [., K]; LOGITS, LOGITS_LOGP: class_logits [., K+1]
    const float* scores[4];    // PROBS
    double T[4];               // LOGITS, LOGITS_LOGP
    int nd, B, D, K, max_class, stride;
    int scaled;                // != 0: out_vars = (double)var * s[d]; 0: the plain conversion
    double* ob;
    double* os;
    double* op;
    double* ov;
    int32_t* oc;
    int32_t* ooff;
    int32_t* ocnt;
    int32_t* osingle;
    double* olp;               // LOGITS_LOGP: [rows, K+1] log-posteriors
    double s[4];               // read when scaled
    int32_t* osrc;             // pe_proben_pack_pooled: [rows] detector index of the row; NULL: not written
};

// One wavefront per image.  The ordered compaction: per detector the first min(counts, D) rows in chunks of 64, a row is kept when
// class <= max_class, the kept rows of a chunk land behind the `written` rows before them in lane order (ballot + prefix count), a
// detector that contributed a row is a source.  The route (a template parameter: PROBS carries no softmax code) only decides where
// a kept row's probabilities and score come from; on the logits routes the chunk's 64 rows go through the softmax 64 / G at a time.
template <PackRoute ROUTE>
__global__ __launch_bounds__(64) void proben_pack_kernel(PackRows a) {
    constexpr bool LOGP = ROUTE == LOGITS_LOGP;
    const int b = blockIdx.x, lane = threadIdx.x;
    const int k1 = a.K + 1;
    const int G = (ROUTE != PROBS && k1 <= 64) ? pe::group_width(k1) : 0;
    int written = 0, sources = 0;
    for (int d = 0; d < a.nd; ++d) {
        const int before = written;
        const int c = min(a.counts[d][b], a.D);
        const double T = a.T[d];
        for (int base = 0; base < c; base += 64) {
            const int j = base + lane;
            bool ok = false;
            int cls = 0;
            if (j < c) {
                cls = a.classes[d][(size_t)b * a.D + j];
                ok = cls <= a.max_class;
            }
            const unsigned long long m = __ballot(ok);
            const int dst_local = written + __popcll(m & pe::lanemask_lt());
            const size_t src = (size_t)b * a.D + j;
            const size_t dst = (size_t)b * a.stride + dst_local;
            if (ok) {
                for (int e = 0; e < 4; ++e) a.ob[dst * 4 + e] = (double)a.boxes[d][src * 4 + e];
                if (ROUTE == PROBS) {
                    a.os[dst] = (double)a.scores[d][src];
                    for (int k = 0; k < a.K; ++k) a.op[dst * a.K + k] = (double)a.cols[d][src * a.K + k];
                }
                const double v = (double)a.vars[d][src];
                a.ov[dst] = a.scaled ? v * a.s[d] : v;      // wave-uniform
                a.oc[dst] = cls;
                if (a.osrc) a.osrc[dst] = d;                // wave-uniform
            }
            if (ROUTE != PROBS) {
                if (G) {
                    const int rows_per_pass = 64 / G, col = lane & (G - 1);
                    const int top = min(64, c - base);
                    for (int r0 = 0; r0 < top; r0 += rows_per_pass) {          // wave-uniform trip count
                        const int r = r0 + lane / G;                             // the chunk row this lane's group holds (< 64)
                        const bool live = ((m >> r) & 1ull) != 0;
                        const int rdst = __shfl(dst_local, r);
                        const int rcls = __shfl(cls, r);
                        const float* row = a.cols[d] + ((size_t)b * a.D + base + r) * k1;
                        double lp = 0.0;
                        const double p = pe::softmax_group<LOGP>(row, live, col, k1, G, T, &lp);
                        if (live) {
                            const size_t o = (size_t)b * a.stride + rdst;
                            if (col < a.K) a.op[o * a.K + col] = p;
                            if (col == rcls) a.os[o] = p;
                            if (LOGP && col < k1) a.olp[o * k1 + col] = lp;
                        }
                    }
                    // a class outside [0, K] cannot index the row: its score is NaN rather than a neighbour's value
                    if (ok && (cls < 0 || cls >= k1)) a.os[dst] = __builtin_nan("");
                } else if (ok) {
                    const double pw = pe::softmax_serial(a.cols[d] + src * k1, k1, T, a.op + dst * a.K, a.K, cls,
                                                         LOGP ? a.olp + dst * k1 : nullptr);
                    a.os[dst] = (cls >= 0 && cls < k1) ? pw : __builtin_nan("");
                }
            }
            written += __popcll(m);
        }
        sources += written > before ? 1 : 0;
    }
    if (lane == 0) {
        a.ooff[b] = b * a.stride;
        a.ocnt[b] = written;
        if (a.osingle) a.osingle[b] = sources == 1 ? 1 : 0;
    }
}

const char* const kRouteName[] = {"pe_proben_pack_detections", "pe_proben_pack_logits", "pe_proben_pack_log_posteriors"};

// All four entry points: every argument check and the launch.  The messages carry the name of the route's own entry point, also
// when pe_proben_pack_calibrated or pe_proben_pack_pooled (the only callers with var_scales_host / out_source) selected it.
int pack_impl(PackRoute route, const float* const* det_boxes_host, const float* const* det_scores_host,
              const int32_t* const* det_classes_host, const float* const* det_probs_host, const float* const* det_logits_host,
              const float* const* det_vars_host, const int32_t* const* det_counts_host, const double* temperatures_host,
              const double* var_scales_host, int32_t num_detectors, int32_t num_images, int32_t det_stride, int32_t num_classes,
              int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores, double* out_probs, double* out_log_probs,
              double* out_vars, int32_t* out_classes, int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source,
              int32_t* out_source, void* stream) {
    const char* what = kRouteName[route];
    const bool probs = route == PROBS;
    PE_CHECK_ARG(num_detectors >= 1 && num_detectors <= 4, "%s: num_detectors %d", what, num_detectors);
    PE_CHECK_ARG(num_images >= 0 && det_stride >= 0, "%s: num_images %d, det_stride %d", what, num_images, det_stride);
    PE_CHECK_ARG(probs || num_classes >= 1, "%s: num_classes %d", what, num_classes);
    PE_CHECK_ARG(row_stride >= num_detectors * det_stride, "%s: row_stride %d < %d", what, row_stride, num_detectors * det_stride);
    PE_CHECK_ARG(det_boxes_host && det_classes_host && det_vars_host && det_counts_host &&
                     (probs ? det_scores_host && det_probs_host : det_logits_host && temperatures_host),
                 "%s: null pointer (detector tables%s)", what, probs ? "" : " / temperatures");
    PE_CHECK_ARG(out_boxes && out_scores && out_probs && out_vars && out_classes && out_offsets && out_counts, "%s: null output", what);
    PE_CHECK_ARG(route != LOGITS_LOGP || out_log_probs, "%s: null output (out_log_probs)", what);
    PackRows a{};
    for (int d = 0; d < num_detectors; ++d) {
        if (var_scales_host)
            PE_CHECK_ARG(pe::finite_positive(var_scales_host[d]), "pe_proben_pack_calibrated: variance scale %g of detector %d is not finite and > 0",
                         var_scales_host[d], d);
        if (!probs)
            PE_CHECK_ARG(pe::finite_positive(temperatures_host[d]), "%s: temperature %g of detector %d is not finite and > 0", what,
                         temperatures_host[d], d);
        a.boxes[d] = det_boxes_host[d]; a.classes[d] = det_classes_host[d]; a.vars[d] = det_vars_host[d]; a.counts[d] = det_counts_host[d];
        if (probs) { a.scores[d] = det_scores_host[d]; a.cols[d] = det_probs_host[d]; }
        else { a.cols[d] = det_logits_host[d]; a.T[d] = temperatures_host[d]; }
        a.s[d] = var_scales_host ? var_scales_host[d] : 1.0;
        PE_CHECK_ARG(a.boxes[d] && a.classes[d] && a.vars[d] && a.counts[d] && a.cols[d] && (a.scores[d] || !probs),
                     "%s: null pointer of detector %d", what, d);
    }
    if (num_images == 0) return PE_OK;
    a.scaled = var_scales_host != nullptr;
    a.nd = num_detectors; a.B = num_images; a.D = det_stride; a.K = num_classes; a.max_class = max_class;
    a.stride = row_stride; a.ob = out_boxes; a.os = out_scores; a.op = out_probs; a.ov = out_vars; a.oc = out_classes;
    a.ooff = out_offsets; a.ocnt = out_counts; a.osingle = out_single_source; a.olp = out_log_probs;
    a.osrc = out_source;
    void (*kernel)(PackRows) = probs ? proben_pack_kernel<PROBS> : route == LOGITS ? proben_pack_kernel<LOGITS> : proben_pack_kernel<LOGITS_LOGP>;
    hipLaunchKernelGGL(kernel, dim3(num_images), dim3(64), 0, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}

// pe_proben_pack_calibrated / pe_proben_pack_pooled: their own checks - which route the arguments select.  Everything else is the route's.
int pack_select(const char* what, const float* const* det_boxes_host, const float* const* det_scores_host,
                const int32_t* const* det_classes_host, const float* const* det_probs_host, const float* const* det_logits_host,
                const float* const* det_vars_host, const int32_t* const* det_counts_host, const double* temperatures_host,
                const double* var_scales_host, int32_t num_detectors, int32_t num_images, int32_t det_stride, int32_t num_classes,
                int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores, double* out_probs, double* out_log_probs,
                double* out_vars, int32_t* out_classes, int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source,
                int32_t* out_source, void* stream) {
    if (det_logits_host) {
        PE_CHECK_ARG(temperatures_host, "%s: null pointer (temperatures: the logits route needs one per detector)", what);
        PE_CHECK_ARG(!det_scores_host && !det_probs_host, "%s: both probabilities and logits given: one route at a time", what);
    } else {
        PE_CHECK_ARG(det_scores_host && det_probs_host, "%s: null pointer (neither probabilities nor logits)", what);
        PE_CHECK_ARG(!temperatures_host && !out_log_probs, "%s: temperatures / out_log_probs belong to the logits route", what);
    }
    return pack_impl(!det_logits_host ? PROBS : out_log_probs ? LOGITS_LOGP : LOGITS, det_boxes_host, det_scores_host, det_classes_host,
                     det_probs_host, det_logits_host, det_vars_host, det_counts_host, temperatures_host, var_scales_host, num_detectors,
                     num_images, det_stride, num_classes, max_class, row_stride, out_boxes, out_scores, out_probs, out_log_probs, out_vars,
                     out_classes, out_offsets, out_counts, out_single_source, out_source, stream);
}

}  // namespace

extern "C" int pe_proben_pack_detections(const float* const* det_boxes_host, const float* const* det_scores_host,
                                         const int32_t* const* det_classes_host, const float* const* det_probs_host,
                                         const float* const* det_vars_host, const int32_t* const* det_counts_host,
                                         int32_t num_detectors, int32_t num_images, int32_t det_stride,
                                         int32_t num_classes, int32_t max_class, int32_t row_stride,
                                         double* out_boxes, double* out_scores, double* out_probs, double* out_vars,
                                         int32_t* out_classes, int32_t* out_offsets, int32_t* out_counts,
                                         int32_t* out_single_source, void* stream) {
    return pack_impl(PROBS, det_boxes_host, det_scores_host, det_classes_host, det_probs_host, nullptr, det_vars_host, det_counts_host,
                     nullptr, nullptr, num_detectors, num_images, det_stride, num_classes, max_class, row_stride, out_boxes, out_scores,
                     out_probs, nullptr, out_vars, out_classes, out_offsets, out_counts, out_single_source, nullptr, stream);
}

extern "C" int pe_proben_pack_logits(const float* const* det_boxes_host, const int32_t* const* det_classes_host,
                                     const float* const* det_logits_host, const float* const* det_vars_host,
                                     const int32_t* const* det_counts_host, const double* temperatures_host,
                                     int32_t num_detectors, int32_t num_images, int32_t det_stride, int32_t num_classes,
                                     int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores,
                                     double* out_probs, double* out_vars, int32_t* out_classes, int32_t* out_offsets,
                                     int32_t* out_counts, int32_t* out_single_source, void* stream) {
    return pack_impl(LOGITS, det_boxes_host, nullptr, det_classes_host, nullptr, det_logits_host, det_vars_host, det_counts_host,
                     temperatures_host, nullptr, num_detectors, num_images, det_stride, num_classes, max_class, row_stride, out_boxes,
                     out_scores, out_probs, nullptr, out_vars, out_classes, out_offsets, out_counts, out_single_source, nullptr, stream);
}

extern "C" int pe_proben_pack_log_posteriors(const float* const* det_boxes_host, const int32_t* const* det_classes_host,
                                             const float* const* det_logits_host, const float* const* det_vars_host,
                                             const int32_t* const* det_counts_host, const double* temperatures_host,
                                             int32_t num_detectors, int32_t num_images, int32_t det_stride, int32_t num_classes,
                                             int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores,
                                             double* out_probs, double* out_log_probs, double* out_vars, int32_t* out_classes,
                                             int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source, void* stream) {
    return pack_impl(LOGITS_LOGP, det_boxes_host, nullptr, det_classes_host, nullptr, det_logits_host, det_vars_host, det_counts_host,
                     temperatures_host, nullptr, num_detectors, num_images, det_stride, num_classes, max_class, row_stride, out_boxes,
                     out_scores, out_probs, out_log_probs, out_vars, out_classes, out_offsets, out_counts, out_single_source, nullptr, stream);
}

extern "C" int pe_proben_pack_calibrated(const float* const* det_boxes_host, const float* const* det_scores_host,
                                         const int32_t* const* det_classes_host, const float* const* det_probs_host,
                                         const float* const* det_logits_host, const float* const* det_vars_host,
                                         const int32_t* const* det_counts_host, const double* temperatures_host,
                                         const double* var_scales_host, int32_t num_detectors, int32_t num_images,
                                         int32_t det_stride, int32_t num_classes, int32_t max_class, int32_t row_stride,
                                         double* out_boxes, double* out_scores, double* out_probs, double* out_log_probs,
                                         double* out_vars, int32_t* out_classes, int32_t* out_offsets, int32_t* out_counts,
                                         int32_t* out_single_source, void* stream) {
    return pack_select("pe_proben_pack_calibrated", det_boxes_host, det_scores_host, det_classes_host, det_probs_host, det_logits_host,
                       det_vars_host, det_counts_host, temperatures_host, var_scales_host, num_detectors, num_images, det_stride,
                       num_classes, max_class, row_stride, out_boxes, out_scores, out_probs, out_log_probs, out_vars, out_classes,
                       out_offsets, out_counts, out_single_source, nullptr, stream);
}

extern "C" int pe_proben_pack_pooled(const float* const* det_boxes_host, const float* const* det_scores_host,
                                     const int32_t* const* det_classes_host, const float* const* det_probs_host,
                                     const float* const* det_logits_host, const float* const* det_vars_host,
                                     const int32_t* const* det_counts_host, const double* temperatures_host,
                                     const double* var_scales_host, int32_t num_detectors, int32_t num_images, int32_t det_stride,
                                     int32_t num_classes, int32_t max_class, int32_t row_stride, double* out_boxes,
                                     double* out_scores, double* out_probs, double* out_log_probs, double* out_vars,
                                     int32_t* out_classes, int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source,
                                     int32_t* out_source, void* stream) {
    PE_CHECK_ARG(out_source, "pe_proben_pack_pooled: null output (out_source)");
    return pack_select("pe_proben_pack_pooled", det_boxes_host, det_scores_host, det_classes_host, det_probs_host, det_logits_host,
                       det_vars_host, det_counts_host, temperatures_host, var_scales_host, num_detectors, num_images, det_stride,
                       num_classes, max_class, row_stride, out_boxes, out_scores, out_probs, out_log_probs, out_vars, out_classes,
                       out_offsets, out_counts, out_single_source, out_source, stream);
}
