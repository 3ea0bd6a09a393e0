/*
 * proben_hip.h - C-ABI of libproben_hip.so: the MI355X (gfx950) implementation of the
 * RGB+thermal detection-and-fusion inference path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every entry point
 *     only ENQUEUES work on that stream: no allocation, no hidden synchronisation;
 *   - the caller allocates all outputs and scratch;
 *   - return value: 0 = ok, negative = error (PE_ERR_*); pe_last_error() returns a
 *     thread-local, human-readable message for the last failing call on this thread.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * upstream repository Jamie725/Multimodal-Object-Detection-via-Probabilistic-Ensembling).
 */
#ifndef PROBEN_HIP_H
#define PROBEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_OK 0
#define PE_ERR_INVALID_ARG (-1)
#define PE_ERR_UNSUPPORTED (-2)
#define PE_ERR_HIP (-3)

/* score_mode / box_mode of pe_proben_fuse_batch (demo/FLIR/demo_probEn.py:145-167,
 * CLI flags --score_fusion / --box_fusion in detectron2/utils/opt.py:14-17) */
#define PE_SCORE_PROBEN 0
#define PE_SCORE_AVG 1
#define PE_SCORE_MAX 2
#define PE_SCORE_PROBEN_BINARY 3 /* demo_probEn.py:24-30, the K = 1 (KAIST) form */
#define PE_SCORE_PROBEN_LOGP 4   /* pe_proben_fuse_batch_logp only: ProbEn over log-posteriors with an explicit background column */
#define PE_BOX_VAVG 0
#define PE_BOX_SAVG 1
#define PE_BOX_AVG 2
#define PE_BOX_ARGMAX 3

const char* pe_last_error(void);
int pe_version(void);

/* ---------------------------------------------------------------------------------------------
 * ProbEn late fusion, batched over images.
 * Replaces nms_bayesian + bayesian_fusion_multiclass + weighted_box_fusion + avg_bbox_fusion
 * (demo/FLIR/demo_probEn.py:20-42,73-77,92-187), called per image from `fusion`
 * (demo_probEn.py:189-196) inside apply_late_fusion_and_evaluate (demo_probEn.py:198-298).
 *
 * Rows of image b are [offsets[b], offsets[b+1]) of the flat arrays, already concatenated in
 * detector order (prepare_data, demo_probEn.py:79-90).  float64 in (the reference's NumPy math),
 * float64 boxes / float32 scores and classes out (the reference's torch.Tensor exit).
 * Output rows of image b are written at [offsets[b], offsets[b] + out_counts[b]) in pivot order.
 * out_counts[b] = -1 if the image has more than max_rows_per_image rows.
 * One 1024-thread workgroup per image; max_rows_per_image (R) sizes its LDS slab: (8 * (11 + L) + 17) bytes per row, L = num_classes + 1
 * (probEn), 2 (binary) or 0 - 160 KiB hold 1 195 rows at num_classes 3; a bound that does not fit returns PE_ERR_UNSUPPORTED.  With
 * 16 * ceil(R / 64) more bytes per row (R <= ~560 at num_classes 3) the pair tests go into two bit matrices first; the results are the same.
 * ------------------------------------------------------------------------------------------- */
int pe_proben_fuse_batch(const double* boxes,     /* [Ntot,4] xyxy */
                         const double* scores,    /* [Ntot] */
                         const double* probs,     /* [Ntot,K] */
                         const double* variances, /* [Ntot] */
                         const int32_t* classes,  /* [Ntot] */
                         const int32_t* offsets,  /* [B+1] (or [B] when row_counts is given) */
                         const int32_t* row_counts, /* optional [B]: rows of image b = row_counts[b] */
                         const int32_t* passthrough, /* optional [B]: != 0 -> copy the rows unchanged (only ONE
                                                        detector fired: demo_probEn.py:240-253) */
                         int32_t num_images, int32_t num_classes, int32_t max_rows_per_image,
                         int32_t score_mode, int32_t box_mode, double iou_thresh,
                         double frame_w, double frame_h, /* class-band shift: 640, 512 */
                         double* out_boxes,              /* [Ntot,4] */
                         float* out_scores,              /* [Ntot] */
                         float* out_classes,             /* [Ntot] */
                         int32_t* out_keep,              /* [Ntot] row index (image-local) of each pivot */
                         int32_t* out_counts,            /* [B] */
                         void* stream);

/* Detector outputs -> ProbEn input rows, on the device (replaces the JSON hop between
 * demo/FLIR/demo_FLIR_save_predictions.py:133-176 and demo_probEn.py:205-234 + prepare_data :79-90).
 * det_*[d]: DEVICE pointers of detector d's padded outputs: boxes f32 [B,D,4], scores f32 [B,D],
 * classes i32 [B,D], probs f32 [B,D,K], vars f32 [B,D], counts i32 [B]  (host arrays of pointers).
 * Rows with class > max_class are dropped (the reference keeps `classes <= 2`, :148-155).
 * Image b's rows are written at b*row_stride in detector order; out_counts[b] = rows written;
 * out_single_source[b] = 1 when exactly one detector contributed rows (-> passthrough). */
int pe_proben_pack_detections(const float* const* det_boxes_host, const float* const* det_scores_host,
                              const int32_t* const* det_classes_host, const float* const* det_probs_host,
                              const float* const* det_vars_host, const int32_t* const* det_counts_host,
                              int32_t num_detectors, int32_t num_images, int32_t det_stride,
                              int32_t num_classes, int32_t max_class, int32_t row_stride, double* out_boxes,
                              double* out_scores, double* out_probs, double* out_vars, int32_t* out_classes,
                              int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Temperature calibration of the detectors' class posteriors (csrc/calibrate.hip): one scalar T per detector,
 *   p = softmax(logits / T)  over the K + 1 columns of the box head's class_logits (background last),
 * computed per row in float64: z_k = (double)logit_k / T, m = max_k z_k, p_k = exp(z_k - m) / sum_j exp(z_j - m).
 * Nothing is clamped: a NaN / +inf logit gives a NaN row, as the float64 NumPy expression does.
 * Every entry point checks its arguments before any device work: T must be finite and > 0.
 *
 * pe_proben_pack_logits: pe_proben_pack_detections with det_logits_host[d] (f32 [B,D,K+1]) in place of the probabilities and
 *   temperatures_host[d] (host doubles, one per detector).  out_probs receives the K foreground p_k, out_scores the row's own
 *   p_class (so avg / max score fusion and the clustering order see the calibrated score; a class outside [0,K] gives NaN).
 *   Boxes, variances, classes, offsets, counts and the single-source flag are those of pe_proben_pack_detections, bit for bit.
 *   The background column is not stored: pe_proben_fuse_batch forms it as 1 - sum(p).
 * pe_calibrated_softmax: the same arithmetic over a flat f32 [num_rows, num_columns] tensor; out_probs f64 [num_rows, num_columns]
 *   holds all K + 1 columns.  A row gets the same bits here and in pe_proben_pack_logits.
 * pe_temperature_nll: for each of num_temperatures <= 64 candidates T_t (host doubles), over logits f32 [num_rows, num_columns] and
 *   labels i32 [num_rows] in [0, K] (K = background):
 *     out[2t]     = sum_i -log softmax(logits_i / T_t)[label_i]
 *     out[2t + 1] = its derivative with respect to log T_t = sum_i (z_label - sum_k p_k z_k)
 *   One read of the logits serves all candidates.  Deterministic: per-workgroup partial sums in a fixed order into
 *   workspace (f64, PE_TEMPERATURE_NLL_MAX_BLOCKS * num_temperatures * 2 values), then one fixed-order pass; no floating-point
 *   atomics, so the same input gives the same bits.  out_flags i32 [2]: [0] = rows whose label is outside [0, K] (they add nothing
 *   to the sums: the caller must treat a non-zero count as an argument error), [1] = 1 + the largest such row index.
 * ------------------------------------------------------------------------------------------- */
#define PE_TEMPERATURE_NLL_MAX_BLOCKS 1024
int pe_proben_pack_logits(const float* const* det_boxes_host, const int32_t* const* det_classes_host,
                          const float* const* det_logits_host, const float* const* det_vars_host,
                          const int32_t* const* det_counts_host, const double* temperatures_host,
                          int32_t num_detectors, int32_t num_images, int32_t det_stride, int32_t num_classes,
                          int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores,
                          double* out_probs, double* out_vars, int32_t* out_classes, int32_t* out_offsets,
                          int32_t* out_counts, int32_t* out_single_source, void* stream);
int pe_calibrated_softmax(const float* logits, int64_t num_rows, int32_t num_columns, double temperature,
                          double* out_probs, void* stream);
int pe_temperature_nll(const float* logits, const int32_t* labels, int64_t num_rows, int32_t num_columns,
                       const double* temperatures_host, int32_t num_temperatures, double* workspace,
                       double* out, int32_t* out_flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Log-posterior ProbEn (PE_SCORE_PROBEN_LOGP): the Bayes rule of bayesian_fusion_multiclass (demo/FLIR/demo_probEn.py:32-42) evaluated
 * on log-posteriors over all K + 1 columns, background included.  It departs from the reference in three places, on purpose:
 *   - :35-36 forms the background as 1 - sum(p) over float32 probabilities: 0 or a few 1e-8 of either sign on a saturated row, so its
 *     log is -inf or NaN and the whole cluster's score is NaN.  Here the background is the box head's own column,
 *     log p_k = z_k - m - log(sum_j exp(z_j - m)), z = (double)logit / T, m = max_k z_k: finite for every finite logit;
 *   - :38-40 takes exp(sum of logs) before normalising, which underflows to 0 / 0 on large clusters of confident rows.  Here the
 *     cluster's columns a_j are normalised as exp(a_j - max a) / sum_j exp(a_j - max a): the largest term is exp(0) = 1;
 *   - the reference drops the class prior of p(y | x_1..x_m) ~ prod_i p(y | x_i) / p(y)^(m-1) (uniform prior).  Here log_prior, when
 *     given, is subtracted (m - 1) times per column.
 * Where probEn is well conditioned the two agree to rounding (float64), so after the float32 exit to within 1 ulp.  Opt-in: the other
 * score modes and entry points are untouched.
 *
 * pe_proben_pack_log_posteriors: pe_proben_pack_logits plus out_log_probs f64 [rows, K + 1] (row stride K + 1, background column
 *   stored).  Every other output - out_scores (the row's calibrated p_class) and out_probs included - is pe_proben_pack_logits' bit for
 *   bit (one device function), so the clustering order and the s-avg / argmax box rules see what the temperature route sees.  max and
 *   sum of a row are the lane group's xor butterflies for K + 1 <= 64 (every lane gets the same bits), a serial column-order loop above.
 * pe_log_softmax: the same arithmetic over a flat f32 [num_rows, num_columns] tensor; a row gets the same bits here and in the pack.
 * pe_proben_fuse_batch_logp: pe_proben_fuse_batch with log_probs f64 [Ntot, K + 1] in place of probs and no score_mode; same kernel
 *   (a template instantiation), clustering (both forms), box modes, LDS budget (L = K + 1), K <= 62, out_counts = -1 and passthrough
 *   rules.  For a cluster of m > 1 rows in cluster order (matches first, pivot last):
 *     a_j = (sum_t log_probs[t][j]) - (m - 1) * log_prior[j]      (sequential sum; the prior term only when log_prior != NULL)
 *     s_j = exp(a_j - max_j a_j) / sum_j exp(a_j - max_j a_j)     (column order)
 *   fused score = max_j s_j over the K + 1 entries INCLUDING background, class = its first index, NaN wins (the rule of PE_SCORE_PROBEN).
 *   A cluster of one keeps its row's score and class.  log_prior: optional DEVICE f64 [K + 1] (NULL = uniform), log of a normalised
 *   prior; being a device pointer it cannot be checked here - entries must be finite (no NaN, no +-inf): the caller's contract
 *   (fusion.log_class_prior validates it).  -inf / NaN log_probs propagate as in NumPy (a NaN column gives a NaN score).
 * ------------------------------------------------------------------------------------------- */
int pe_proben_pack_log_posteriors(const float* const* det_boxes_host, const int32_t* const* det_classes_host,
                                  const float* const* det_logits_host, const float* const* det_vars_host,
                                  const int32_t* const* det_counts_host, const double* temperatures_host,
                                  int32_t num_detectors, int32_t num_images, int32_t det_stride, int32_t num_classes,
                                  int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores,
                                  double* out_probs, double* out_log_probs, double* out_vars, int32_t* out_classes,
                                  int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source, void* stream);
int pe_log_softmax(const float* logits, int64_t num_rows, int32_t num_columns, double temperature, double* out_log_probs,
                   void* stream);
int pe_proben_fuse_batch_logp(const double* boxes, const double* scores, const double* log_probs, /* [Ntot,K+1] */
                              const double* variances, const int32_t* classes, const int32_t* offsets,
                              const int32_t* row_counts, const int32_t* passthrough, int32_t num_images, int32_t num_classes,
                              int32_t max_rows_per_image, int32_t box_mode, double iou_thresh, double frame_w, double frame_h,
                              const double* log_prior, /* optional [K+1] */
                              double* out_boxes, float* out_scores, float* out_classes, int32_t* out_keep, int32_t* out_counts,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Variance calibration of the detectors' box heads (csrc/variance.hip): one scale s_d per detector, variance' = s_d * variance, where
 * the variance is the box head's one scalar per detection, exp(var_pred), trained by a Gaussian NLL in box-delta units
 * (training.py::bbox_gaussian_loss).  Not in the reference, which fuses the heads' variances as they come (demo/FLIR/demo_probEn.py
 * :155-160 weights each member box by 1 / variance); v-avg only sees the ratios between detectors, so this is a per-detector correction.
 *
 * pe_match_ground_truth: replaces calibration.match_labels (an image at a time on the CPU, labels only) for flat device tensors.
 *   det_boxes f64 [M,4] XYXY with det_offsets i32 [B+1], gt_boxes f64 [G,4] with gt_offsets i32 [B+1], gt_classes i32 [G], gt_crowd
 *   optional i32 [G] (!= 0: the box takes no part).  Per detection: out_labels = the class of the ground-truth box of its image with
 *   the largest IoU if that IoU >= iou_thresh, else num_classes; out_match = that box's flat index in [0, G), else -1; out_iou = the
 *   largest IoU over the boxes that took part (0 without one).  IoU as finetune.pairwise_iou, float64, unfused: the same bits.  The
 *   lowest index wins among equal maxima.  A class outside [0, num_classes] is passed on as it is (the caller folds it).  Images
 *   without detections or ground truth are legal; the ground truth of an image is walked in LDS-sized chunks, any number of boxes.
 * pe_variance_stats: over num_rows matched rows (det_boxes f64 [M,4], match i32 [M] into gt_boxes f64 [num_gt,4], variances f64 [M]),
 *   r = Box2BoxTransform.get_deltas(detection, matched ground truth) (modeling.py; weights bbox_reg_weights_host, 4 host floats, NULL
 *   = 10, 10, 5, 5) in float64 and q_i = sum_c r_ic^2 / var_i:
 *     out[0] = n rows used, out[1] = sum_i q_i, out[2] = sum_i log var_i,
 *     out[3] / out[4] = (row, coordinate) pairs with r^2 <= scale * var / r^2 <= 4 * scale * var   (counts, exact in f64).
 *   A row is excluded (adds nothing) when match < 0 (or >= num_gt: never read), a width or height of either box is not > 0, or the
 *   variance is not finite and > 0; out_flags i32 [2]: [0] = excluded rows, [1] = 1 + the largest excluded row index, as
 *   pe_temperature_nll reports bad labels.  Deterministic like pe_temperature_nll: per-workgroup partials in a fixed order into
 *   workspace (f64, PE_VARIANCE_STATS_MAX_BLOCKS * 5 values), then one fixed-order pass; no floating-point atomics.
 *   The fit is closed: s_hat = out[1] / (4 n), NLL(s) = 0.5 (4 n log s + 4 out[2] + out[1] / s).
 * pe_proben_pack_calibrated: pe_proben_pack_detections (det_scores_host + det_probs_host given, det_logits_host, temperatures_host
 *   and out_log_probs NULL), pe_proben_pack_logits (det_logits_host + temperatures_host given, scores / probs NULL) or
 *   pe_proben_pack_log_posteriors (the latter with out_log_probs) behind one signature, plus var_scales_host (optional host doubles,
 *   one per detector, finite and > 0): out_vars = (double)var_f32 * s_d, one float64 multiply where the variance is written (one
 *   launch, the route's own kernel).  Every other output is the bits of the entry point it stands for; with var_scales_host NULL (the
 *   plain conversion, no multiply) or all 1.0 so is out_vars.
 * ------------------------------------------------------------------------------------------- */
#define PE_VARIANCE_STATS_MAX_BLOCKS 1024
int pe_match_ground_truth(const double* det_boxes, const int32_t* det_offsets, const double* gt_boxes, const int32_t* gt_offsets,
                          const int32_t* gt_classes, const int32_t* gt_crowd /* optional */, int32_t num_images, double iou_thresh,
                          int32_t num_classes, int32_t* out_labels, int32_t* out_match, double* out_iou, void* stream);
int pe_variance_stats(const double* det_boxes, const int32_t* match, const double* gt_boxes, const double* variances,
                      int64_t num_rows, int64_t num_gt, const float* bbox_reg_weights_host /* optional [4] */, double scale,
                      double* workspace, double* out /* [5] */, int32_t* out_flags /* [2] */, void* stream);
int pe_proben_pack_calibrated(const float* const* det_boxes_host, const float* const* det_scores_host,
                              const int32_t* const* det_classes_host, const float* const* det_probs_host,
                              const float* const* det_logits_host, const float* const* det_vars_host,
                              const int32_t* const* det_counts_host, const double* temperatures_host,
                              const double* var_scales_host /* optional */, int32_t num_detectors, int32_t num_images,
                              int32_t det_stride, int32_t num_classes, int32_t max_class, int32_t row_stride, double* out_boxes,
                              double* out_scores, double* out_probs, double* out_log_probs /* optional */, double* out_vars,
                              int32_t* out_classes, int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reliability statistics of a score (csrc/reliability.hip): what a reliability diagram, the expected and the maximum calibration error
 * (ECE, MCE) and the Brier score are made of, for the rows a calibration was NOT fitted on.  Not in the reference.
 *
 * Bins: num_bins = B in [1, PE_RELIABILITY_MAX_BINS] bins of equal width on [0, 1]; a row with confidence conf falls into
 *   bin = min((int)(conf * B), B - 1)  (one float64 multiply), so conf == 1.0 lies in the last bin.
 * Outputs: out_counts i64 [B, 2]: [b][0] = rows in the bin, [b][1] = correct rows (both exact); out_sums f64 [B, 2]: [b][0] = sum of
 *   conf, [b][1] = sum of the Brier term d * d, d = conf - (correct ? 1.0 : 0.0) (two IEEE operations, no contraction).
 *   ECE = sum_b (n_b / N) |correct_b / n_b - sum conf_b / n_b|, MCE = the largest of those gaps, Brier = sum_b sum term_b / N
 *   (calibration.summarise_reliability).
 * pe_reliability_logits: logits f32 [num_rows, num_columns] (K + 1 columns, background last), labels i32 [num_rows] in [0, K].
 *   p = softmax(logits / temperature) as in pe_calibrated_softmax: the same row arithmetic (csrc/softmax_row.h), the same bits.
 *   classes i32 [num_rows] given: conf = p[classes[i]], correct = (labels[i] == classes[i]) - the detection's own score, the one
 *   pe_proben_pack_logits writes to out_scores.  classes NULL (top label): conf = max_k p_k over all K + 1 columns, the predicted class
 *   is the FIRST index that attains it, correct = (that index == labels[i]).
 *   A row is excluded - it adds nothing - when its label or its class is outside [0, K] or its conf is NaN (a NaN or +inf logit).
 * pe_reliability_scores: conf f64 [num_rows], correct i32 [num_rows] (non-zero = correct): the same bins, outputs and flags for scores
 *   that do not come from a softmax (the fused detections).  A conf that is NaN or outside [0, 1] excludes the row.
 * out_flags i32 [2], as pe_temperature_nll's: [0] = excluded rows, [1] = 1 + the largest excluded row index.
 * Deterministic like pe_temperature_nll and pe_variance_stats - no floating-point atomics, the same input gives the same bits:
 *   min(ceil(num_rows / 256), PE_RELIABILITY_MAX_BLOCKS) workgroups of 4 wavefronts, a function of num_rows alone.  Wavefront v of the
 *   grid takes row groups v, v + (4 * workgroups), ... (a group = the 64 / G rows of calibrated_softmax_kernel's lane groups for
 *   K + 1 <= 64, G the power of two >= K + 1; 64 rows otherwise) and adds their rows in ascending row order into its own table of B
 *   bins; a workgroup adds its 4 tables in wavefront order into its 4 * num_bins slots of the workspace; a second kernel
 *   adds the workgroups in the one order that csrc/reduce2.h states.
 *   workspace: PE_RELIABILITY_MAX_BLOCKS * num_bins * 4 eight-byte values.
 * Arguments are checked before any device work (temperature finite and > 0, num_bins, num_columns >= 2, num_rows >= 0, null
 * pointers).  num_rows == 0 reads nothing: the outputs that are given are zeroed and no pointer is required.
 * ------------------------------------------------------------------------------------------- */
#define PE_RELIABILITY_MAX_BINS 64
#define PE_RELIABILITY_MAX_BLOCKS 1024
int pe_reliability_logits(const float* logits, const int32_t* labels, const int32_t* classes /* optional */, int64_t num_rows,
                          int32_t num_columns, double temperature, int32_t num_bins, double* workspace, int64_t* out_counts,
                          double* out_sums, int32_t* out_flags, void* stream);
int pe_reliability_scores(const double* conf, const int32_t* correct, int64_t num_rows, int32_t num_bins, double* workspace,
                          int64_t* out_counts, double* out_sums, int32_t* out_flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pooling weights of log-posterior ProbEn: the logarithmic opinion pool, one exponent w_d >= 0 per detector INSIDE the fusion.  ProbEn's
 * product assumes detectors that are conditionally independent given the class; detectors that share evidence (two that look at the
 * same thermal frame, several rows of one detector in a cluster) count it twice and the fused score is over-confident although every
 * detector is calibrated on its own.  Not in the reference.  For a cluster of m > 1 rows in cluster order (matches first, pivot last),
 * d(t) the detector row t came from:
 *     a_j = (sum_t w_d(t) * log_probs[t][j]) - (W - 1) * log_prior[j],   W = sum_t w_d(t)   (both sums sequential, in that order; the
 *                                                                                            prior term only when log_prior != NULL)
 *     s_j = exp(a_j - max_j a_j) / sum_j exp(a_j - max_j a_j)                               (column order)
 * With every w = 1 this is PE_SCORE_PROBEN_LOGP bit for bit (1.0 * x is x, W is the integer m); with sum w = 1 over a cluster it is a
 * weighted geometric mean.  Unlike a temperature, w leaves the row's own score alone: the clustering order, clusters of one and s-avg.
 *
 * pe_proben_fuse_batch_pooled: pe_proben_fuse_batch_logp plus row_source i32 [Ntot] (the detector index of each row), pool_weights
 *   DEVICE f64 [num_detectors], num_detectors in [1, PE_POOL_MAX_DETECTORS], and the optional output out_cluster i32 [Ntot].  Same
 *   kernel (a template instantiation), clustering (both forms), box modes, score / class rule (maximum over the K + 1 columns, first
 *   index, NaN wins), K <= 62, out_counts = -1 and passthrough rules; a cluster of one keeps its row's score and class, whatever the
 *   weights.  The weight is staged in LDS beside the row: 8 more bytes per row than pe_proben_fuse_batch_logp in the LDS budget.
 *   pool_weights is a device pointer and cannot be checked here: entries must be finite and >= 0, not all 0 - the caller's contract
 *   (fusion.pool_weight_tensor validates it).  A row whose source is outside [0, num_detectors) takes a NaN weight (a NaN score for its
 *   cluster); 0 * -inf is NaN as in NumPy.
 *   out_cluster[offsets[b] + r], r an input row of image b: the output row k of the cluster the row ended in, as pivot or as member;
 *   -1 when the row left the pool without joining one (a NaN IoU); r on a passthrough image; untouched when out_counts[b] is -1.
 * pe_proben_pack_pooled: pe_proben_pack_calibrated plus out_source i32 [num_images * row_stride] (required): the detector index d
 *   of every written row, stored where the row is stored, in the one walk.  Every other output is pe_proben_pack_calibrated's bits.
 * pe_pool_nll: the objective of the weights' fit.  log_probs f64 [num_rows, num_columns] (K + 1 columns in [2, 64]), row_source i32
 *   [num_rows]; the clusters in CSR form, member_rows i32 [num_members] (row indices) and cluster_offsets i32 [num_clusters + 1];
 *   labels i32 [num_clusters] in [0, K]; log_prior optional DEVICE f64 [K + 1]; weights_host: num_candidates <= 64 candidate vectors,
 *   host doubles [num_candidates, num_detectors], each finite and >= 0 (checked; the array is free again on return).  Per candidate c,
 *   out f64 [num_candidates, 1 + num_detectors]:
 *     out[c][0]     = sum over clusters of -log s_label(w_c)
 *     out[c][1 + d] = its derivative in w_d = sum over clusters of  sum_j s_j G_dj - G_d,label,
 *     G_dj = S_dj - n_d lp_j,  S_dj = the sum of log_probs[t][j] over the cluster's rows of detector d (member order), n_d their
 *     number, lp the log prior (0 when NULL); a_j is evaluated as (sum_d w_d G_dj) + lp_j, d ascending - the same value as the fusion's
 *     member-order sum up to rounding.  The NLL is convex in w (a is linear in w).
 *   Lane = candidate, wavefront = cluster: a wavefront reads its cluster's rows once (lane = column) into the table G in LDS and the 64
 *   candidates work from it.  A cluster is excluded - it adds nothing - when it has fewer than 2 rows (the product does not fuse
 *   those), its label is outside [0, K], one of its rows has a source outside [0, num_detectors), or its offsets / one of its row
 *   indices point outside the arrays; out_flags i32 [2]: [0] = excluded clusters, [1] = 1 + the largest excluded cluster index.
 *   Deterministic like pe_temperature_nll: min(ceil(num_clusters / 4), PE_POOL_NLL_MAX_BLOCKS) workgroups, a function of num_clusters
 *   alone, per-workgroup partials in a fixed order, one fixed-order finishing pass, no floating-point atomics.
 *   workspace: f64, num_candidates * (num_detectors + PE_POOL_NLL_MAX_BLOCKS * (1 + num_detectors)) values.
 * Arguments are checked before any device work.
 * ------------------------------------------------------------------------------------------- */
#define PE_POOL_MAX_DETECTORS 8
#define PE_POOL_NLL_MAX_BLOCKS 1024
int pe_proben_fuse_batch_pooled(const double* boxes, const double* scores, const double* log_probs, /* [Ntot,K+1] */
                                const double* variances, const int32_t* classes, const int32_t* row_source, /* [Ntot] */
                                const int32_t* offsets, const int32_t* row_counts, const int32_t* passthrough, int32_t num_images,
                                int32_t num_classes, int32_t max_rows_per_image, int32_t box_mode, double iou_thresh, double frame_w,
                                double frame_h, const double* log_prior, /* optional [K+1] */
                                const double* pool_weights,              /* DEVICE [num_detectors] */
                                int32_t num_detectors, double* out_boxes, float* out_scores, float* out_classes, int32_t* out_keep,
                                int32_t* out_counts, int32_t* out_cluster /* optional [Ntot] */, void* stream);
int pe_proben_pack_pooled(const float* const* det_boxes_host, const float* const* det_scores_host,
                          const int32_t* const* det_classes_host, const float* const* det_probs_host,
                          const float* const* det_logits_host, const float* const* det_vars_host,
                          const int32_t* const* det_counts_host, const double* temperatures_host,
                          const double* var_scales_host /* optional */, int32_t num_detectors, int32_t num_images,
                          int32_t det_stride, int32_t num_classes, int32_t max_class, int32_t row_stride, double* out_boxes,
                          double* out_scores, double* out_probs, double* out_log_probs /* optional */, double* out_vars,
                          int32_t* out_classes, int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source,
                          int32_t* out_source, void* stream);
int pe_pool_nll(const double* log_probs, const int32_t* row_source, int64_t num_rows, int32_t num_columns,
                const int32_t* member_rows, int64_t num_members, const int32_t* cluster_offsets, const int32_t* labels,
                int32_t num_clusters, const double* log_prior /* optional */, const double* weights_host, int32_t num_candidates,
                int32_t num_detectors, double* workspace, double* out, int32_t* out_flags /* [2] */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The fused detection as a full prediction: what phase 4 of the fusion kernel forms and pe_proben_fuse_batch_logp / _pooled drop.  Not in
 * the reference.
 * pe_proben_fuse_batch_posterior: the arguments of pe_proben_fuse_batch_pooled - row_source and pool_weights may be NULL TOGETHER, which is
 *   the unpooled rule of pe_proben_fuse_batch_logp (num_detectors is then not looked at) - and three more outputs, indexed like out_scores
 *   (image b's fused rows are [offsets[b], offsets[b] + out_counts[b])).  Same kernel (a template instantiation); out_boxes, out_scores,
 *   out_classes, out_keep, out_counts and out_cluster (optional, with or without weights) are the bits of the entry point it stands for.
 *   out_log_posterior f64 [Ntot, K + 1]: for a cluster of m >= 2 rows lq_j = (a_j - top) - log(tot), a_j the cluster's summed column (member
 *     order, prior and pool weights included), top = max_j a_j, tot = sum_j exp(a_j - top) in column order - the quantities the score is made
 *     of, so exp(lq_class) is the fused score up to rounding.  A cluster of one row and a passed-through row: the row's input log_probs, copied.
 *   out_vars f64 [Ntot]: the variance of the fused box under the independence its box rule assumes, sum_t lambda_t^2 var_t with lambda_t the
 *     weight the rule gives member t.  v-avg: 1.0 / wsum, wsum the box fusion's own sequential sum of 1 / var_t (= 1 / sum 1 / var);
 *     s-avg: lambda_t = s_t / sum s; avg: lambda_t = 1 / m - both summed sequentially in cluster order (matches in sorted order, pivot last)
 *     as (lambda_t * lambda_t) * var_t; argmax: the chosen member's variance.  A cluster of one and a passed-through row: the row's own.
 *   out_members i32 [Ntot]: the rows in the cluster; 1 for a cluster of one and for a passed-through row.
 *   Every element of a live fused row is written exactly once, by the thread that owns the cluster (the row, on passthrough); nothing is
 *   written for an image with out_counts -1 or beyond out_counts[b] (fusion.fuse_batch pre-fills NaN / NaN / 0).  No atomics.
 *   Checked before any device work, on top of every check of pe_proben_fuse_batch_pooled: row_source and pool_weights both NULL or both
 *   set; the three new pointers non-NULL.
 * ------------------------------------------------------------------------------------------- */
int pe_proben_fuse_batch_posterior(const double* boxes, const double* scores, const double* log_probs, /* [Ntot,K+1] */
                                   const double* variances, const int32_t* classes, const int32_t* row_source, /* [Ntot] or NULL */
                                   const int32_t* offsets, const int32_t* row_counts, const int32_t* passthrough, int32_t num_images,
                                   int32_t num_classes, int32_t max_rows_per_image, int32_t box_mode, double iou_thresh, double frame_w,
                                   double frame_h, const double* log_prior, /* optional [K+1] */
                                   const double* pool_weights,              /* DEVICE [num_detectors] or NULL */
                                   int32_t num_detectors, double* out_boxes, float* out_scores, float* out_classes, int32_t* out_keep,
                                   int32_t* out_counts, int32_t* out_cluster /* optional [Ntot] */,
                                   double* out_log_posterior /* [Ntot,K+1] */, double* out_vars /* [Ntot] */,
                                   int32_t* out_members /* [Ntot] */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Presence evidence for log-posterior ProbEn: WHICH detectors produced a row of a cluster is an observation about the class that the
 * product of posteriors never uses (each posterior is conditioned on "this detector produced a row").  Not in the reference.  With D
 * detectors, D <= PE_PRESENCE_MAX_DETECTORS, a cluster's pattern is P = OR over its rows of (1 << row_source[row]), in [1, 2^D), and
 *     a_j = (the a_j of pe_proben_fuse_batch_logp / _pooled, prior and pool weights included) + presence[P * (K + 1) + j]
 * - the addition last, once per column -, then the max-subtracted softmax and the score / class rule as before (maximum over the K + 1
 * columns, first index, NaN wins).  presence is a table of float64 log-evidence [2^D][K + 1] (row 0 unused), indexed by the pattern and
 * not a miss probability per detector: detectors that share a frame do not fire independently given the class.
 * pe_proben_fuse_batch_presence: the arguments of pe_proben_fuse_batch_posterior with row_source REQUIRED, pool_weights optional (NULL =
 *   the unpooled rule) and out_log_posterior / out_vars / out_members optional TOGETHER (all NULL = a score-only run); presence DEVICE f64
 *   [(1 << num_detectors) * (K + 1)], every entry finite (a device pointer, not checked here: calibration.presence_table validates it);
 *   num_detectors in [1, PE_PRESENCE_MAX_DETECTORS] (it also sizes pool_weights); out_pattern optional i32 [Ntot], indexed like
 *   out_scores: the fused row's pattern, written once by the thread that owns the cluster (the row, on passthrough).  Same kernel (a
 *   template instantiation), clustering (both forms), box modes, K <= 62 and out_counts = -1 rules.
 *   A cluster of ONE row is fused: a_j = log_probs[row][j] + presence[1 << source][j] - no pool weight and no prior, which is what those
 *   rules give a lone row -, its score the normalised maximum, its class the argmax over all K + 1 columns (a lone row whose largest
 *   column becomes background leaves as a background row), out_log_posterior normalised; box, keep and variance stay the row's own.
 *   A passthrough image is rescored, not clustered: each row is such a cluster of one, output row = input row, keep = r, count = n; rows
 *   of one detector are never merged with each other there.
 *   Nothing before the fusion phase reads the table: the row's own scores decide the clustering order, s-avg's weights and argmax's box,
 *   so the clusters at a zero table are the clusters at every table.  At a zero table every output of a cluster of m >= 2 rows equals
 *   pe_proben_fuse_batch_logp / _pooled / _posterior (x + 0.0 is x); lone and passthrough rows are normalised and differ from the copied
 *   score by rounding.
 *   A row whose source is outside [0, num_detectors) makes every column of its cluster NaN (a NaN score, class 0 by the NaN rule) and adds
 *   no bit to out_pattern (0 for a lone such row).
 *   The row's detector index is staged in LDS beside the row: 4 more bytes per row in the LDS budget.
 * pe_bias_nll: the objective of the table's fit.  One row b of the table is a bias-only softmax regression over the clusters of its
 *   pattern, convex in b: base f64 [num_clusters, num_columns] (the fused log-posterior at a zero table), labels i32 [num_clusters] in
 *   [0, K]; candidates_host: num_candidates <= 64 candidate rows, host doubles [num_candidates, num_columns], each finite (checked; the
 *   array is free again on return).  Per candidate c, out f64 [num_candidates, 1 + num_columns]:
 *     out[c][0]     = sum over clusters of -log softmax(base + b_c)[label] = log(tot) - (a_label - top),
 *     out[c][1 + j] = its derivative in b_j = sum over clusters of e_j / tot - [label == j],
 *     a_j = base_j + b_j, top = max_j a_j, e_j = exp(a_j - top), tot = sum_j e_j in column order.
 *   Lane = candidate, wavefront = cluster; a lane's candidate and accumulators live in registers, so num_columns <=
 *   PE_BIAS_NLL_MAX_COLUMNS (FLIR has 4, KAIST 2); more returns PE_ERR_UNSUPPORTED.  A cluster is excluded - it adds nothing - when its
 *   label is outside [0, K] or its base holds a non-finite entry; out_flags i32 [2]: [0] = excluded clusters, [1] = 1 + the largest
 *   excluded index.  num_clusters == 0 is valid: zeros, no kernel.  Deterministic like pe_pool_nll: min(ceil(num_clusters / 4),
 *   PE_BIAS_NLL_MAX_BLOCKS) workgroups, a function of num_clusters alone, per-workgroup partials [workgroup][candidate][1 + num_columns]
 *   in a fixed order, the fixed-order finishing pass, no floating-point atomics.
 *   workspace: f64, num_candidates * (num_columns + PE_BIAS_NLL_MAX_BLOCKS * (1 + num_columns)) values.
 * Arguments are checked before any device work.
 * ------------------------------------------------------------------------------------------- */
#define PE_PRESENCE_MAX_DETECTORS 4
#define PE_BIAS_NLL_MAX_COLUMNS 16
#define PE_BIAS_NLL_MAX_BLOCKS 1024
int pe_proben_fuse_batch_presence(const double* boxes, const double* scores, const double* log_probs, /* [Ntot,K+1] */
                                  const double* variances, const int32_t* classes, const int32_t* row_source, /* [Ntot] */
                                  const int32_t* offsets, const int32_t* row_counts, const int32_t* passthrough, int32_t num_images,
                                  int32_t num_classes, int32_t max_rows_per_image, int32_t box_mode, double iou_thresh, double frame_w,
                                  double frame_h, const double* log_prior, /* optional [K+1] */
                                  const double* pool_weights,              /* DEVICE [num_detectors] or NULL */
                                  const double* presence,                  /* DEVICE [(1 << num_detectors) * (K+1)] */
                                  int32_t num_detectors, double* out_boxes, float* out_scores, float* out_classes, int32_t* out_keep,
                                  int32_t* out_counts, int32_t* out_cluster /* optional [Ntot] */,
                                  double* out_log_posterior /* [Ntot,K+1] */, double* out_vars /* [Ntot] */,
                                  int32_t* out_members /* [Ntot]; the three NULL together = score only */,
                                  int32_t* out_pattern /* optional [Ntot] */, void* stream);
int pe_bias_nll(const double* base, const int32_t* labels, int32_t num_clusters, int32_t num_columns, const double* candidates_host,
                int32_t num_candidates, double* workspace, double* out, int32_t* out_flags /* [2] */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Correlated box fusion, box_fusion "c-avg" (csrc/boxcorr.hip).  Not a box_mode of the fusion kernel: a second
 * launch after a "v-avg" fusion that wrote out_cluster.
 * pe_box_gls_batch: for every fused row k < counts[b] of image b whose cluster (the input rows with cluster == k) has two or more rows,
 *   out_boxes[offsets[b] + k] and, when given, out_vars[offsets[b] + k] are OVERWRITTEN with the generalised-least-squares mean of the
 *   members' boxes and its variance 1 / (1' C^-1 1), C_tu = R_tu sqrt(var_t var_u), R = the members' correlation under `correlation`
 *   (DEVICE, row-major [num_detectors * num_detectors], symmetric: entry [a][b] between rows of detectors a != b, [d][d] between two rows
 *   of detector d, in [0, 1); positive semidefinite - the caller's to check).  boxes / variances / row_source / cluster are the
 *   fusion's inputs and its out_cluster, offsets / row_counts its layout, counts its out_counts.  Nothing else is written: not for an
 *   image with counts <= 0, not beyond counts[b], not for a cluster of one row.  A member whose source is outside [0, num_detectors)
 *   makes its cluster's box and variance NaN, and so does a cluster whose R is not positive definite (several rows of one detector
 *   under an off-diagonal entry the diagonal cannot carry: no distribution has those correlations).  A workgroup per image, rows staged in LDS 1 024 at a time (48 KiB), so the capacity is the
 *   fusion's: max_rows_per_image in [1, 2048].  num_detectors in [1, PE_BOX_CORR_MAX_DETECTORS].
 * pe_box_pair_stats: the statistics of the correlation's fit over clusters in CSR form (member_rows [num_members] into the packed rows,
 *   cluster_offsets [num_clusters + 1], cluster_match [num_clusters] = the cluster's ground-truth box or -1: the cluster adds nothing).
 *   With z_t = get_deltas(row t, ground truth) / sqrt(var_t) (bbox_reg_weights as pe_variance_stats), out holds 28 eight-byte values:
 *   int64 N_ab for the 10 detector pairs a <= b in the order 00 01 02 03 11 12 13 22 23 33 (unordered member pairs t < u of one cluster),
 *   int64 M_d [4] (member rows), then f64 S_ab [10] = sum over those pairs of sum_c z_tc z_uc and f64 Q_d [4] = sum_c z_tc^2.  A member
 *   with a degenerate box (its own or the ground truth's), a variance that is not finite and > 0 or a source outside [0, num_detectors)
 *   takes no part and is counted in out_flags ([2]: how many, 1 + the last such member index).  No floating-point atomics; the grid,
 *   min(ceil(num_clusters / 256), PE_BOX_PAIR_MAX_BLOCKS) workgroups, is a function of num_clusters alone: same input, same bits.
 *   workspace: f64, 6 * num_members + (num_members + 1) / 2 + 28 * PE_BOX_PAIR_MAX_BLOCKS values.  num_clusters == 0: zeros, no kernel.
 * Arguments are checked before any device work.
 * ------------------------------------------------------------------------------------------- */
#define PE_BOX_CORR_MAX_DETECTORS PE_PRESENCE_MAX_DETECTORS
#define PE_BOX_PAIR_MAX_BLOCKS 1024
int pe_box_gls_batch(const double* boxes, const double* variances, const int32_t* row_source, const int32_t* cluster,
                     const int32_t* offsets, const int32_t* row_counts /* optional */, const int32_t* counts, int32_t num_images,
                     int32_t max_rows_per_image, const double* correlation, int32_t num_detectors, double* out_boxes /* in/out */,
                     double* out_vars /* optional, in/out */, void* stream);
int pe_box_pair_stats(const double* boxes, const double* variances, const int32_t* row_source, int64_t num_rows,
                      const int32_t* member_rows, int64_t num_members, const int32_t* cluster_offsets, const int32_t* cluster_match,
                      int32_t num_clusters, const double* gt_boxes, int64_t num_gt, int32_t num_detectors,
                      const float* bbox_reg_weights_host /* [4] or NULL = 10, 10, 5, 5 */, double* workspace, double* out /* [28] */,
                      int32_t* out_flags /* [2] */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused convolution / GEMM: NHWC fp16 activations, [Cout][KH][KW][Cin] fp16 weights, fp32 accumulate
 * on MFMA, epilogue = + bias[Cout] (fp32) + residual + ReLU, fp16 (or fp32) NHWC output.
 * Replaces, per layer, detectron2.layers.Conv2d.forward (layers/wrappers.py:62-98) + FrozenBatchNorm2d
 * (layers/batch_norm.py:45-65; folded into weight/bias by the caller) + relu_ + the residual add of
 * BottleneckBlock.forward (modeling/backbone/resnet.py:205-221) + the nearest-2x top-down add of
 * FPN.forward (modeling/backbone/fpn.py:129-137); with H = W = 1 it is the nn.Linear of
 * FastRCNNConvFCHead / FastRCNNOutputLayers (roi_heads/box_head.py:73-81, fast_rcnn.py:531-545).
 *   kernel 1: 1x1, stride 1|2, no padding, Cin % 64 == 0
 *   kernel 3: 3x3, stride 1, padding 1, Cin % 64 == 0
 *   kernel 7: the stem, 7x7 stride 2 padding 3 over an NHWC4 input; weight packed [Cout][8][8][4]
 *             (kh 0..6 real + 1 zero row, kw 0..6 real + 1 zero column, 4 channels)
 *   residual_mode 0: none; 1: residual has the output's shape; 2: residual is [N,res_h,res_w,Cout]
 *             and is read at (oh/2, ow/2) (nearest-2x upsample).
 *   out_f32 != 0: fp32 output, only channels [0, cout_store) are written, row stride out_stride.
 * Kernels behind it (all with the same fp32 summation order per output - K ascending, zero-initialised accumulators, then + bias,
 * + residual, ReLU - so which one takes a launch never shows in a result, and the choice looks at channel counts / stride only, never at
 * the batch): csrc/conv1x1_ring.hip (persistent loader / consumer kernel: 1x1 with a bias, fp16 output, Cout % 256 == 0, tensors < 2 GiB;
 * residual-free from Cin 512 at stride 1 / 256 at stride 2, with a residual from Cin 128), csrc/conv_igemm2.hip (every other 1x1 and 3x3),
 * csrc/conv_igemm.hip (the unfused stem).
 * ------------------------------------------------------------------------------------------- */
int pe_conv2d_nhwc_f16(const void* input, const void* weight, const float* bias, const void* residual,
                       void* output, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                       int32_t kernel, int32_t stride, int32_t relu, int32_t residual_mode,
                       int32_t res_h, int32_t res_w, int32_t out_f32, int32_t cout_store,
                       int32_t out_stride, void* stream);
/* (kernel-selection knobs for A/B measurements are not part of this ABI: csrc/test_hooks.h) */

/* ---------------------------------------------------------------------------------------------
 * "Weights-direct" 3x3 convolution (csrc/conv_wd.h): same reference rows as pe_conv2d_nhwc_f16 with kernel 3
 * (layers/wrappers.py:62-98 + folded FrozenBatchNorm2d layers/batch_norm.py:45-65 + relu_; the 3x3 convolutions of
 * backbone/resnet.py:205-221, backbone/fpn.py:127-137 and proposal_generator/rpn.py:74-85).
 * The weights are packed ONCE into MFMA-fragment order (pe_conv_wd_pack_weights) and streamed L2 -> VGPR; only the
 * pixels go through LDS.  Supported: stride 1 / pad 1, Cin % 64 == 0, Cout % 256 == 0, W % 32 == 0 with W | 128 or
 * 128 | W, input < 2 GiB; everything else -> pe_conv2d_nhwc_f16.  Epilogue: + bias (required) + ReLU, fp16 NHWC
 * output with row stride out_stride (0 = Cout).
 * ------------------------------------------------------------------------------------------- */
int pe_conv_wd_supported(int32_t kernel, int32_t stride, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
/* ... and the batch: 1 where pe_conv3x3_wd_f16 (tail_cout 0), pe_conv3x3_wd_rpn_head_f16 (Cout 256, tail_cout 0) or
 * pe_bottleneck_tail_wd_f16 (Cout 256) takes the launch - the geometry rule above, input and tail output < 2 GiB.  The entry
 * points make their size checks through it; a caller that wants to fall back to pe_conv2d_nhwc_f16 asks it first. */
int pe_conv_wd_launch_supported(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t tail_cout);
/* Two kernel generations stand behind pe_conv3x3_wd_f16, pe_conv3x3_wd_rpn_head_f16 and pe_bottleneck_tail_wd_f16: two waves per SIMD,
 * one tile per workgroup (csrc/conv_wd.h), and one wave per SIMD with 256 accumulators in the AGPRs and PERSISTENT workgroups
 * (csrc/conv_wd9.h: the pure 3x3 and the fused RPN head at image widths 64 / 128 / 256 from 128 tiles of 256 pixels on - the same
 * bits as the two-wave kernels, so the size rule may look at the batch).  pe_bottleneck_tail_wd_f16 always runs on csrc/conv_wd.h.
 * A persistent kernel occupies every CU it runs on for its whole duration; the ones that ship (csrc/conv_wd9.h, csrc/conv1x1_ring.hip)
 * measured best at one workgroup per CU under one, two and three concurrent detector streams (profiles/r04_pipeline_ab_2.txt,
 * r05_pipeline_ab_ring.txt), so there is nothing for a caller to tune (round 4-5's `pe_conv_wd_set_concurrent_streams` hint, a
 * validated no-op since its kernel left the library, was removed from the ABI in round 6). */
/* weight: [Cout][3][3][Cin] fp16 (the layout pe_conv2d_nhwc_f16 takes); packed: Cout*9*Cin halfs */
int pe_conv_wd_pack_weights(const void* weight, void* packed, int32_t Cout, int32_t Cin, int32_t kernel, void* stream);
int pe_conv3x3_wd_f16(const void* input, const void* packed_weight, const float* bias, void* output, int32_t N,
                      int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t relu, int32_t out_stride, void* stream);
/* StandardRPNHead.forward for one level in ONE launch (proposal_generator/rpn.py:74-85): t = relu(conv3x3(x)) with 256
 * output channels never leaves the chip; head_out[m][0..15] = head_bias16 + head_weight[rows <= 16][256] * t[m]  (fp32 rows of
 * 16: 3 objectness logits, 12 anchor deltas, 1 pad - the layout pe_rpn_select_topk reads).  head_weight is packed once with
 * pe_conv_wd_pack_head ([rows][256] fp16 in, 16 KiB out); geometry rule of pe_conv_wd_supported with Cout = 256. */
/* The second half of BottleneckBlock.forward in ONE launch (modeling/backbone/resnet.py:207-221): conv2 3x3 (Cin -> 256,
 * folded BN) + ReLU -> conv3 1x1 (256 -> tail_cout, folded BN) + shortcut + ReLU.  The 256-channel intermediate stays on the
 * chip (LDS) and the stand-alone, latency-bound 1x1 launch disappears.  tail weight [tail_cout][256] fp16 is packed once with
 * pe_conv_wd_pack_tail (same size out); residual (optional) and output are [N,H,W,tail_cout] fp16; tail_cout % 256 == 0;
 * geometry rule of pe_conv_wd_supported with Cout = 256. */
int pe_conv_wd_pack_tail(const void* weight, void* packed, int32_t tail_cout, int32_t C, void* stream);
int pe_bottleneck_tail_wd_f16(const void* input, const void* packed_weight3x3, const float* bias3x3, const void* packed_tail,
                              const float* tail_bias, const void* residual, void* output, int32_t N, int32_t H, int32_t W,
                              int32_t Cin, int32_t tail_cout, void* stream);
/* A 64-channel-wide stride-1 BottleneckBlock from its 3x3 on, plus the next block's first convolution, in ONE launch (res2:
 * modeling/backbone/resnet.py:107-221 with bottleneck_channels = 64, out_channels = 256; build_resnet_backbone :558-572):
 *     t2 = relu(conv2_3x3(t1) + bias2);  out = relu(conv3(t2) + bias3 + shortcut);  [t1_next = relu(conv1_next(out) + bias1n)]
 * t1 [N,H,W,64] fp16 is relu(conv1(x)) of this block.  shortcut_src: the block input x [N,H,W,256] (identity shortcut), or -
 * has_shortcut_conv - the input s [N,H,W,64] of the first block's shortcut convolution (64 -> 256, folded BN, bias_sc).
 * out [N,H,W,256] fp16; t1_next [N,H,W,64] fp16 when has_next.  Any H, W; tensors < 2 GiB.  The intermediate t2, the shortcut
 * convolution's output and the re-read of `out` by the next conv1 never touch HBM.
 * pe_bneck64_pack: w2 [64][3][3][64], w3 [256][64], wsc [256][64] or NULL, w1n [64][256] or NULL (fp16, the layouts
 * pe_conv2d_nhwc_f16 takes) -> one fragment-ordered stream of pe_bneck64_packed_bytes(wsc != NULL, w1n != NULL) bytes. */
size_t pe_bneck64_packed_bytes(int32_t has_shortcut_conv, int32_t has_next);
int pe_bneck64_supported(int32_t N, int32_t H, int32_t W);   /* 1 where pe_bneck64_f16 takes the size (its own check) */
int pe_bneck64_pack(const void* w2, const void* w3, const void* wsc, const void* w1n, void* packed, void* stream);
int pe_bneck64_f16(const void* t1, const void* shortcut_src, const void* packed, const float* bias2, const float* bias3,
                   const float* bias_sc, const float* bias1n, void* out, void* t1_next, int32_t N, int32_t H, int32_t W,
                   int32_t has_shortcut_conv, int32_t has_next, void* stream);
/* The last convolution of an identity BottleneckBlock and the first of the NEXT block in ONE launch (res3:
 * modeling/backbone/resnet.py:205-221 - `out = self.conv3(out)`, `out += shortcut`, `relu_` - followed by the next block's
 * `out = self.conv1(x)`, `relu_` of the same rows):
 *     out = relu(conv3(t2) + bias3 + residual);  t1_next = relu(conv1_next(out) + bias1_next)
 * t2 [N,H,W,Cin] fp16 is the block's 3x3 output, residual [N,H,W,Cout] fp16 its input; w3 [Cout][Cin], w1_next [Cnext][Cout]
 * fp16 and the fp32 biases in the layouts pe_conv2d_nhwc_f16 takes (BN folded).  out [N,H,W,Cout] and t1_next [N,H,W,Cnext]
 * fp16 are both written, with the bits of the two pe_conv2d_nhwc_f16 launches it replaces; the re-read of `out` by the next
 * conv1 never touches HBM.  One instantiation: Cin = 128, Cout = 512, Cnext = 128.  Any N, H, W; tensors < 2 GiB; out and
 * t1_next must not overlap t2, residual or each other.  pe_conv1x1_pair_supported: 1 where the launch takes these channel
 * counts and N * H * W = pixels (the check pe_conv1x1_pair_f16 itself makes). */
int pe_conv1x1_pair_supported(int32_t Cin, int32_t Cout, int32_t Cnext, int64_t pixels);
int pe_conv1x1_pair_f16(const void* t2, const void* w3, const float* bias3, const void* residual, const void* w1_next,
                        const float* bias1_next, void* out, void* t1_next, int32_t N, int32_t H, int32_t W, int32_t Cin,
                        int32_t Cout, int32_t Cnext, void* stream);
int pe_conv_wd_pack_head(const void* head_weight, void* packed, int32_t rows, int32_t C, void* stream);
int pe_conv3x3_wd_rpn_head_f16(const void* input, const void* packed_weight, const float* bias, const void* packed_head,
                               const float* head_bias16, float* head_out, int32_t N, int32_t H, int32_t W, int32_t Cin,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Front-end layout kernels.
 * pe_preprocess_pack: one image -> normalised, zero-padded NHWC4 fp16 (optionally bilinear-resized first).
 *   Replaces GeneralizedRCNN.preprocess_image (modeling/meta_arch/rcnn.py:269-286), ImageList.from_tensors
 *   (structures/image_list.py:51-102) and, when dst size != src size, ResizeTransform.apply_image
 *   (data/transforms/transform.py:81-98; half-pixel bilinear, uint8 sources rounded back to integers: this is the
 *   stand-in for the cv2.resize branch of the 4- / 6-channel inputs, parity unpinned; 3-channel uint8 images use
 *   pe_preprocess_pack_pil_u8 below, which is Pillow-exact).
 *   src_kind 0: HWC uint8, 1: HWC float32, 2: CHW float32.  Source channels [ch0, ch0+nch) -> output
 *   channels 0..nch-1 (flip_rgb reverses the first three); mean/std are HOST arrays of length nch.
 * pe_maxpool3x3s2_nhwc: F.max_pool2d(x, 3, 2, 1) of BasicStem.forward (modeling/backbone/resnet.py:383).
 * pe_subsample2_nhwc:   LastLevelMaxPool (modeling/backbone/fpn.py:166-178) = x[:, ::2, ::2].
 * ------------------------------------------------------------------------------------------- */
int pe_preprocess_pack(const void* src, int32_t src_kind, int32_t src_h, int32_t src_w, int32_t src_c,
                       int32_t ch0, int32_t nch, int32_t flip_rgb, int32_t dst_h, int32_t dst_w,
                       int32_t pad_h, int32_t pad_w, const float* mean_host, const float* std_host,
                       void* dst, void* stream);
/* Same for num_images equally sized images stored back to back (src [N,...], dst [N,pad_h,pad_w,4]): one launch. */
int pe_preprocess_pack_batch(const void* src, int32_t num_images, int32_t src_kind, int32_t src_h, int32_t src_w,
                             int32_t src_c, int32_t ch0, int32_t nch, int32_t flip_rgb, int32_t dst_h, int32_t dst_w,
                             int32_t pad_h, int32_t pad_w, const float* mean_host, const float* std_host, void* dst,
                             void* stream);
/* The same with Pillow's EXACT bilinear resampler for uint8 sources [N,src_h,src_w,src_c] - the reference resizes
 * 3-channel images with Image.fromarray(img.astype(uint8)).resize((w, h), BILINEAR) (data/transforms/transform.py:92-97):
 * horizontal pass rounded to uint8, then vertical pass, 22-bit fixed-point weights.  xtab [dst_w, 2 + xk] /
 * ytab [dst_h, 2 + yk] DEVICE int32 tables (first tap, tap count, weights) of libImaging/Resample.c
 * precompute_coeffs + normalize_coeffs_8bpc (host helper: proben_amd.data.pil_bilinear_tables). */
int pe_preprocess_pack_pil_u8(const void* src, int32_t num_images, int32_t src_h, int32_t src_w, int32_t src_c,
                              int32_t ch0, int32_t nch, int32_t flip_rgb, int32_t dst_h, int32_t dst_w, int32_t pad_h,
                              int32_t pad_w, const float* mean_host, const float* std_host, const int32_t* xtab,
                              int32_t xk, const int32_t* ytab, int32_t yk, void* dst, void* stream);
/* pe_fusion_input_pack: the FLIR early / middle fusion input (demo/FLIR/demo_FLIR_save_predictions.py:98-121) built on the
 * device from the uint8 frames, one launch per output group.  thermal [N,th_h,th_w,3] and rgb [N,rgb_h,rgb_w,3] are DEVICE
 * uint8 BGR batches (data.read_image).  The RGB frame is resized to the thermal size with OpenCV's 8-bit INTER_LINEAR rule
 * (proben_amd.data.cv2_linear_resize_u8; the identity when the sizes agree), stacked as B,G,R,T0,T1,T2, and channels
 * [ch0, ch0+nch) of that stack go through the float INTER_LINEAR resize of pe_preprocess_pack (src_kind 1) to dst_h x dst_w,
 * normalise and zero-pad to pad_h x pad_w (multiples of pad_multiple, less than one multiple above the resized size).
 * Bit for bit the output of the host build + float32 upload + pe_preprocess_pack_batch.  rgb may be null when ch0 >= 3;
 * mean/std are HOST arrays of length nch. */
int pe_fusion_input_pack(const void* thermal, const void* rgb, int32_t num_images, int32_t th_h, int32_t th_w, int32_t rgb_h,
                         int32_t rgb_w, int32_t ch0, int32_t nch, int32_t dst_h, int32_t dst_w, int32_t pad_h, int32_t pad_w,
                         int32_t pad_multiple, const float* mean_host, const float* std_host, void* dst, void* stream);
int pe_maxpool3x3s2_nhwc(const void* in, void* out, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int pe_subsample2_nhwc(const void* in, void* out, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* Fused BasicStem.forward (modeling/backbone/resnet.py:375-384): conv 7x7 / 2 / pad 3 with the frozen BN folded
 * + ReLU + max_pool2d(3, 2, 1) in one pass: x [N,H,W,4] fp16 (H, W multiples of 4) -> out [N,H/4,W/4,64] fp16.
 * w_packed [64,7,8,4] fp16 where tap t multiplies input column 2*c - 4 + t (tap 0 is zero); bias fp32 [64]. */
int pe_stem_conv7x7_maxpool_f16(const void* x, const void* w_packed, const float* bias, void* out, int32_t N,
                                int32_t H, int32_t W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched class-aware greedy NMS (float32).  Replaces detectron2.layers.batched_nms
 * (layers/nms.py:20-37) -> torchvision.ops.boxes.batched_nms / nms (torchvision 0.13.0), call sites
 * proposal_generator/rpn_outputs.py:147, roi_heads/fast_rcnn.py:130, demo/FLIR/demo_probEn.py:64.
 *   boxes [B,n_max,4], scores [B,n_max], idxs [B,n_max] (class / level id, may be NULL; any int32 - ids in [0, 2^18) get
 *   the per-class fast path: tiles of the suppression matrix between different classes are never computed),
 *   counts [B] rows used per image (NULL = n_max), valid [B,n_max] optional row mask.
 *   mode 0: coordinate trick (boxes + idx*(max+1)), mode 1: suppress only within equal idx ("vanilla").
 *   Mode 0 is evaluated per class while every live coordinate of the image is >= 0 (then the bands cannot meet); an image
 *   with a negative coordinate is compared all-pairs on the shifted boxes, so a box reaching below -1 suppresses - and is
 *   suppressed by - the neighbouring class exactly as torchvision's trick does.
 *   out_keep [B,max_out] input-row indices in score-descending order (ties: lower index first),
 *   out_counts [B].  scratch: pe_nms_scratch_bytes(B, n_max) bytes of device memory.
 *   Non-finite inputs (csrc/nms.hip and oracle/nms.py state the rule in full): NaN scores come first, whatever their sign or
 *   payload, ties by index, then +Inf down to -Inf.  A row with a NaN coordinate has a NaN IoU with everything: it is kept and
 *   suppresses nothing.  Mode 0's max is a NaN-propagating maximum over the rows that take part: with a NaN or +Inf
 *   coordinate among them every shifted box is NaN and every row is kept.  Rows masked out or beyond counts never take part.
 * ------------------------------------------------------------------------------------------- */
#define PE_NMS_TRICK 0
#define PE_NMS_CLASS 1
size_t pe_nms_scratch_bytes(int32_t B, int32_t n_max);
int pe_nms_batched(const float* boxes, const float* scores, const int32_t* idxs, const int32_t* counts,
                   const uint8_t* valid, int32_t B, int32_t n_max, float iou_thresh, int32_t mode,
                   int32_t max_out, int32_t* out_keep, int32_t* out_counts, void* scratch,
                   size_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RPN proposal selection: per (image, level) top-k of the objectness logits, decode of the survivors
 * against analytically generated anchors, finite / clip-to-unpadded-size / non-empty flags.
 * Replaces DefaultAnchorGenerator (modeling/anchor_generator.py:43-56,130-199), RPNOutputs.predict_proposals
 * / predict_objectness_logits (proposal_generator/rpn_outputs.py:409-452), Box2BoxTransform.apply_deltas
 * (box_regression.py:73-110) and find_top_rpn_proposals' selection half (rpn_outputs.py:100-145).
 *   level_heads_host[l]: DEVICE pointer to the fused RPN head output of level l, fp32 [N*H*W, head_stride]
 *     (columns 0..2 objectness for anchors a=0..2, columns 3+4a..6+4a the deltas of anchor a); head_stride >= 16,
 *     a multiple of 4, pointers 16-byte aligned (the logits of a cell are fetched as one 16-byte load, once, into LDS);
 *   level_hw_host [L,2], level_stride_host [L], cell_anchors_host [L,3,4] are HOST arrays;
 *   image_hw [N,2] device int32 (h,w) of the unpadded resized images;
 *   outputs per image: cand_per_image = sum_l min(pre_nms_topk, H*W*3) rows, level-major, each level
 *   sorted by logit descending (ties: anchor index ascending).
 * pe_gather_boxes: rows keep[n, :counts[n]] of boxes/scores -> dense [N,max_out,...], zero padded.
 * ------------------------------------------------------------------------------------------- */
int pe_rpn_select_topk(const float* const* level_heads_host, const int32_t* level_hw_host,
                       const int32_t* level_stride_host, const float* cell_anchors_host,
                       int32_t num_levels, int32_t N, int32_t head_stride, int32_t pre_nms_topk,
                       const int32_t* image_hw, float scale_clamp, float* cand_boxes, float* cand_scores,
                       int32_t* cand_level, uint8_t* cand_valid, int32_t cand_per_image, void* scratch,
                       size_t scratch_bytes, void* stream);
/* Optional scratch for pe_rpn_select_topk: with >= this many bytes, levels larger than 16384 anchors are selected in
 * two exact stages (per-slice top-k on many CUs, then a merge) instead of one workgroup per (image, level). */
size_t pe_rpn_scratch_bytes(const int32_t* level_hw_host, int32_t num_levels, int32_t N);
int pe_gather_boxes(const float* boxes, const float* scores, const int32_t* keep, const int32_t* counts,
                    int32_t N, int32_t n_in, int32_t max_out, float* out_boxes, float* out_scores,
                    void* stream);

/* Stand-alone forms of two steps the detector kernels carry fused, because the reference exposes them as Python API:
 * pe_box2box_apply_deltas: Box2BoxTransform.apply_deltas (modeling/box_regression.py:73-110): deltas [N, 4k] and boxes
 *   [N,4] -> [N, 4k]; weights_host = (wx, wy, ww, wh); dw / dh are clamped to scale_clamp before exp.
 * pe_grid_anchors: DefaultAnchorGenerator.grid_anchors for ONE level (modeling/anchor_generator.py:43-56,120-146):
 *   cell_anchors [A,4] + shifts (x * stride, y * stride) (+ offset * stride) -> [H*W*A, 4] in (y, x, anchor) order. */
int pe_box2box_apply_deltas(const float* deltas, const float* boxes, int32_t N, int32_t k, const float* weights_host,
                            float scale_clamp, float* out, void* stream);
int pe_grid_anchors(const float* cell_anchors, int32_t num_cell_anchors, int32_t H, int32_t W, int32_t stride,
                    float offset, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused SGD-with-momentum step over flat fp32 buffers (training half).  Replaces the per-parameter loop of the
 * torch.optim.SGD that solver/build.py:93-133 builds (momentum, per-group lr / weight decay, dampening 0, no Nesterov) behind
 * DefaultTrainer (engine/defaults.py:250-262):  d = grad * grad_scale + weight_decay * p;  buf = first_step ? d : momentum * buf + d;
 * p -= lr * buf;  fp16_shadow (optional, [n] halfs) = (half)p in the same pass.  grad_scale folds DDP's 1 / world_size and the
 * inverse loss scale.  All pointers 16-byte aligned (shadow 8): one call per parameter group of a flat buffer.
 * ------------------------------------------------------------------------------------------- */
int pe_sgd_momentum_f32(float* params, const float* grads, float* momentum_buf, void* fp16_shadow, int64_t n, float lr,
                        float momentum, float weight_decay, float grad_scale, int32_t first_step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ROIAlign forward over NHWC feature maps.  Replaces roi_align_forward of detectron2._C
 * (layers/csrc/ROIAlign/ROIAlign.h:54-84, ROIAlign_cuda.cu:12-139,310-366; same arithmetic as
 * ROIAlign_cpu.cpp:22-218) and, with num_levels == 4, ROIPooler.forward + assign_boxes_to_levels
 * (modeling/poolers.py:13-44,180-235) in one launch.
 *   feats_host[l]: DEVICE pointers, feature l is [N, H_l, W_l, C]; dtype 0 = fp16, 1 = fp32 (in and out);
 *   rois: [R,5] (batch,x1,y1,x2,y2) when rois_have_batch_index, else boxes [N, per_image, 4] with
 *         counts[n] live rows per image (dead rows produce zeros);
 *   output [R, pooled_h, pooled_w, C]; out_level (optional) [R] assigned level or -1.
 * ------------------------------------------------------------------------------------------- */
int pe_roi_align_nhwc(const void* const* feats_host, const int32_t* feat_hw_host, const float* scales_host,
                      int32_t num_levels, int32_t N, int32_t C, int32_t dtype, const float* rois,
                      int32_t rois_have_batch_index, int32_t num_rois, int32_t per_image,
                      const int32_t* counts, int32_t pooled_h, int32_t pooled_w, int32_t sampling_ratio,
                      int32_t aligned, void* output, int32_t* out_level, void* stream);

/* The same, boxes form only ([N, per_image, 4] + counts), with the PROCESSING order chosen by the library: one workgroup per
 * image first sorts its proposals by (FPN level, Morton code of the box centre) into order_workspace ([N * per_image] int32,
 * per_image <= 2048, else the order is left as given), and the ROIAlign workgroups walk that order, one contiguous stretch per
 * XCD.  Outputs land where pe_roi_align_nhwc puts them, bit for bit; only the feature traffic changes (proposals arrive in RPN
 * score order, scattered over the pyramid).  This is what ROIPooler's per-level nonzero/index_put grouping
 * (modeling/poolers.py:219-233) does for locality in the reference, without its four device synchronisations. */
int pe_roi_align_nhwc_sorted(const void* const* feats_host, const int32_t* feat_hw_host, const float* scales_host,
                             int32_t num_levels, int32_t N, int32_t C, int32_t dtype, const float* boxes, int32_t per_image,
                             const int32_t* counts, int32_t pooled_h, int32_t pooled_w, int32_t sampling_ratio,
                             int32_t aligned, void* output, int32_t* out_level, int32_t* order_workspace, void* stream);

/* ROIAlign backward (training half).  Replaces roi_align_backward of detectron2._C
 * (layers/csrc/ROIAlign/ROIAlign.h:86-115, ROIAlign_cuda.cu:141-306,369-420; same arithmetic as ROIAlign_cpu.cpp:221-394)
 * behind _ROIAlign.backward (layers/roi_align.py:26-42) and, with num_levels == 4, the backward of ROIPooler's per-level
 * scatter.  Arguments as pe_roi_align_nhwc; grad_output [R, pooled_h, pooled_w, C] (dtype 0 = fp16, 1 = fp32);
 * grad_feats_host[l]: DEVICE pointers to fp32 [N, H_l, W_l, C] gradients that are ACCUMULATED into (the caller zeroes
 * them); rows beyond counts[n] contribute nothing.  fp32 atomic adds: the summation order over overlapping ROIs is not
 * defined (as in the reference's CUDA kernel). */
int pe_roi_align_backward_nhwc(const void* grad_output, int32_t dtype, const int32_t* feat_hw_host, const float* scales_host,
                               int32_t num_levels, int32_t N, int32_t C, const float* rois, int32_t rois_have_batch_index,
                               int32_t num_rois, int32_t per_image, const int32_t* counts, int32_t pooled_h,
                               int32_t pooled_w, int32_t sampling_ratio, int32_t aligned, float* const* grad_feats_host,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * Box-head post-processing.  Replaces FastRCNNOutputs.inference / fast_rcnn_inference_single_image
 * (modeling/roi_heads/fast_rcnn.py:43-147,345-360,417-452) and detector_postprocess
 * (modeling/postprocessing.py:8-38).  head: fp32 [N*per_image, head_stride] with columns
 * [0,K] logits, [K+1,5K] deltas (class-major), 5K+1 log-variance.
 *   pe_boxhead_candidates: softmax, decode (weights reg_weights_host[4]), finite mask, clip to image_hw,
 *     score > thresh -> candidates in (row, class) order: boxes, scores, class, (filtered row, original row).
 *     At most cand_max candidates per image are kept (proposal-row order); cand_total (optional, may be NULL) receives
 *     the uncapped number so a caller can detect - and refuse - an overflow instead of losing detections silently.
 *   (caller runs pe_nms_batched over the candidates, class-aware, max_out = max_det)
 *   pe_boxhead_finalize: gathers the kept candidates' fields (incl. the reference's Q3/Q4 index quirks;
 *     fix_vars != 0 pairs each detection with its own proposal's variance), rescales to out_hw, clips,
 *     drops empty boxes.
 * ------------------------------------------------------------------------------------------- */
int pe_boxhead_candidates(const float* head, int32_t head_stride, int32_t N, int32_t per_image,
                          int32_t num_classes, const int32_t* prop_counts, const float* proposals,
                          const int32_t* image_hw, const float* reg_weights_host, float scale_clamp,
                          float score_thresh, int32_t cand_max, float* cand_boxes, float* cand_scores,
                          int32_t* cand_class, int32_t* cand_rows, int32_t* cand_counts, int32_t* cand_total,
                          float* probs, void* stream);
int pe_boxhead_finalize(const float* head, int32_t head_stride, int32_t N, int32_t per_image,
                        int32_t num_classes, int32_t cand_max, int32_t max_det, int32_t fix_vars,
                        const float* probs, const float* cand_boxes, const float* cand_scores,
                        const int32_t* cand_class, const int32_t* cand_rows, const int32_t* keep,
                        const int32_t* keep_counts, const int32_t* image_hw, const int32_t* out_hw,
                        float* det_boxes, float* det_scores, int32_t* det_classes, float* det_logits,
                        float* det_probs, float* det_vars, int32_t* det_rows, int32_t* det_counts,
                        void* stream);

/* Variance voting (He, Zhu, Wang, Savvides, Zhang: "Bounding Box Regression with Uncertainty for Accurate Object Detection",
 * CVPR 2019, section 3.3), opt-in, one launch between pe_nms_batched and pe_boxhead_finalize.  In the reference's flow this is the
 * point of fast_rcnn_inference_single_image (modeling/roi_heads/fast_rcnn.py:43-147) right after batched_nms, where boxes[keep] is
 * gathered; the reference itself does not vote.  DESIGN.md section 31 states the rule:
 *   var_i = exp(head[n*per_image + orow_i, 5K+1]) (float32 as pe_boxhead_finalize computes it, then float64; always the candidate's
 *   OWN proposal row - quirk Q3 / fix_vars only choose the variance finalize REPORTS).  For a kept candidate b the voters are the
 *   candidates i of the image with class_i == class_b, IoU(b, i) > 0 (finetune.pairwise_iou's float64 expression) and var_i finite
 *   and > 0;  p_i = exp(-(1 - IoU(b, i))^2 / sigma_t),  w_i = p_i / var_i,  b'[c] = sum_i w_i box_i[c] / sum_i w_i, rounded once
 *   to float32.  A kept box that is no voter of itself (variance NaN, 0 or inf, or a box without area) keeps its bits.
 * out_boxes [N, cand_max, 4] (must not alias cand_boxes): rows [0, cand_counts[n]) of every image are written completely - a
 * candidate that is not kept gets its input row, a kept one its voted box - and nothing else is touched; pe_boxhead_finalize then
 * takes out_boxes in place of cand_boxes.  keep [N, max_det] / keep_counts [N] as pe_nms_batched leaves them; a keep id outside
 * [0, cand_counts[n]) is skipped.  Scores, classes, row ids, counts and the variances finalize reports are not changed by voting.
 * One workgroup per image, candidates staged in LDS in tiles of PE_VAR_VOTE_TILE, a wavefront per kept box, float64 sums in a
 * fixed order without atomics: image n's rows do not depend on N, on the other images or on the run.
 * Checked before any device work: null pointers, num_classes in [1, 80], head_stride >= 5K + 2, cand_max in [1, 16384],
 * max_det >= 1, sigma_t finite and > 0, out_boxes != cand_boxes; N == 0 returns PE_OK. */
#define PE_VAR_VOTE_TILE 4096
int pe_boxhead_var_vote(const float* head, int32_t head_stride, int32_t N, int32_t per_image, int32_t num_classes,
                        int32_t cand_max, int32_t max_det, const float* cand_boxes, const int32_t* cand_class,
                        const int32_t* cand_rows, const int32_t* cand_counts, const int32_t* keep,
                        const int32_t* keep_counts, float sigma_t, float* out_boxes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Native COCO bbox evaluator (HOST code, multithreaded; no GPU involved).  Replaces COCOeval.evaluate /
 * computeIoU / evaluateImg / accumulate of the reference's vendored pycocotools
 * (detectron2/pycocotools/cocoeval.py:85-191, 236-421, Params :500-536) and pycocotools 2.0.4 `_mask.iou`
 * (bbIou) for iouType "bbox"; caller: FLIR_evaluation.py:496-563 (_evaluate_predictions_on_coco).
 *   Ground truth rows (annotation order): gt_img / gt_cat = DENSE indices into the sorted image-id / category-id
 *   lists, gt_box [n_gt,4] xywh float64, gt_area, gt_crowd (uint8), gt_id (annotation ids; an id of 0 counts
 *   as "unmatched", like the reference).  Detection rows (result order; detection id = row + 1, area = w*h):
 *   dt_img, dt_cat, dt_box [n_dt,4] xywh, dt_score.
 *   iou_thrs [T], rec_thrs [R], max_dets [M] ascending, area_rng [A,2].  num_threads <= 0: hardware concurrency (<= 32).
 *   Out: precision [T,R,K,A,M] and recall [T,K,A,M] float64, -1 where the reference leaves -1.
 * ------------------------------------------------------------------------------------------- */
int pe_cocoeval_bbox(const int32_t* gt_img, const int32_t* gt_cat, const double* gt_box, const double* gt_area,
                     const uint8_t* gt_crowd, const int64_t* gt_id, int64_t n_gt, const int32_t* dt_img,
                     const int32_t* dt_cat, const double* dt_box, const double* dt_score, int64_t n_dt,
                     int32_t n_imgs, int32_t n_cats, const double* iou_thrs, int32_t T, const double* rec_thrs,
                     int32_t R, const int32_t* max_dets, int32_t M, const double* area_rng, int32_t A,
                     int32_t num_threads, double* precision, double* recall);

/* ---------------------------------------------------------------------------------------------
 * Paired bootstrap of the COCO statistics over images.  Replaces running COCOeval.accumulate
 * (detectron2/pycocotools/cocoeval.py:315-421) once per resampled dataset: matching is per image and does not change
 * under resampling, so it is exported once by the host evaluator and only accumulate runs per replicate, on the GPU.
 *
 * pe_cocoeval_bbox_matches (HOST code, every pointer a host pointer): the arguments of pe_cocoeval_bbox up to num_threads,
 *   with T <= PE_AP_BOOTSTRAP_MAX_T and max_dets[M-1] <= 256 (PE_ERR_UNSUPPORTED otherwise).  Caller-sized outputs:
 *   list_off [K+1]: category k owns entries [list_off[k], list_off[k+1]) - per image its top max_dets[M-1] detections, images in
 *     order, stably sorted by descending score (NaN last): what accumulate sorts for maxDet = max_dets[M-1], the same for every area range;
 *   list_img, list_rank [n_dt]: the entry's dense image index and its rank inside its image (the list of a smaller maxDet is the
 *     sub-sequence rank < maxDet);
 *   list_flags [A][n_dt] (row stride n_dt): bit t = matched at iou_thrs[t], bit 16 + t = ignored at iou_thrs[t], for area range a;
 *   npig [K][A][n_imgs]: the image's non-ignored ground truths.
 *
 * pe_ap_bootstrap (device pointers): the lists above (list_stride = the row stride of list_flags, >= list_off[K]); mult u8 [B][I],
 *   replicate b holds image i mult[b][i] times (0 - 255; the caller checks the range before it narrows to u8); rec_thrs f64 [R]
 *   ascending; cells i32 [C][3] = (category, area range, maxDet).  Per (replicate, cell, threshold), with w_j = mult[img_j] when
 *   rank_j < maxDet and 0 otherwise:  NP = sum_i mult_i npig_i,  TP_j / FP_j = running sums of w_j tp_j / w_j fp_j  (tp = matched and not
 *   ignored, fp = neither),  rc_j = TP_j / NP,  pr_j = TP_j / (FP_j + TP_j + 2^-52) made non-increasing from the right,
 *   q[r] = pr[first j with rc_j >= rec_thrs[r]] or 0.
 *   Out: psum f64 [B][C][T] = q[0] + q[1] + ... in that order; recall f64 [B][C][T] = rc_last (0 for an empty list); valid i32 [B][C]
 *   = 1, or 0 when NP = 0 (psum 0, recall and precision -1, like the reference's untouched cells), or -1 when the cell's triple or its
 *   list bounds are out of range; precision f64 [B][C][T][R] = q, optional (NULL: not written).
 *   Counts are int32 (list_stride * 255 must fit) and NP int64: the same bytes whatever B and C are.  One workgroup per
 *   (replicate, cell), one wavefront per threshold; I <= PE_AP_BOOTSTRAP_MAX_IMAGES, T <= PE_AP_BOOTSTRAP_MAX_T,
 *   R <= PE_AP_BOOTSTRAP_MAX_R, else PE_ERR_UNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
#define PE_AP_BOOTSTRAP_MAX_T 16
#define PE_AP_BOOTSTRAP_MAX_R 128
#define PE_AP_BOOTSTRAP_MAX_IMAGES 32768
int pe_cocoeval_bbox_matches(const int32_t* gt_img, const int32_t* gt_cat, const double* gt_box, const double* gt_area,
                             const uint8_t* gt_crowd, const int64_t* gt_id, int64_t n_gt, const int32_t* dt_img,
                             const int32_t* dt_cat, const double* dt_box, const double* dt_score, int64_t n_dt,
                             int32_t n_imgs, int32_t n_cats, const double* iou_thrs, int32_t T, const double* rec_thrs,
                             int32_t R, const int32_t* max_dets, int32_t M, const double* area_rng, int32_t A,
                             int32_t num_threads, int64_t* list_off, int32_t* list_img, uint8_t* list_rank,
                             uint32_t* list_flags, int32_t* npig);
int pe_ap_bootstrap(const int64_t* list_off, const int32_t* list_img, const uint8_t* list_rank, const uint32_t* list_flags,
                    int64_t list_stride, const int32_t* npig, const uint8_t* mult, int32_t B, int32_t I, int32_t K, int32_t A,
                    int32_t T, const double* rec_thrs, int32_t R, const int32_t* cells, int32_t C, double* psum,
                    double* recall, int32_t* valid, double* precision, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Paired bootstrap of the KAIST log-average miss rate over images.  Replaces running the accumulate of
 * evalKAIST/evaluation_script.py - the evaluator behind demo/KAIST/demo_LAMR_KAIST.py:85,145 (KAISTPedEval.accumulate) - once per
 * resampled dataset: the per-image matching is exported once on the host (lamr_bootstrap.export_lamr_matches) and only accumulate runs
 * per replicate, on the GPU.
 *
 * pe_lamr_bootstrap (device pointers): list_img i32 [n_list], the dense image index of every entry of the evaluator's list (all
 *   images, stably sorted by descending score); list_flags u8 [n_list], bit 0 = matched, bit 1 = ignored; npig i32 [I], the image's
 *   non-ignored ground truths; mult u8 [B][I], replicate b holds image i mult[b][i] times; fppi_thrs f64 [R]; cells i32 [C][2] =
 *   (lo, hi), the image-index range [lo, hi) the cell is evaluated over.  Per (replicate, cell), with w_j = mult[img_j] when
 *   lo <= img_j < hi and entry j is not ignored and 0 otherwise (an image index outside [0, I) weighs 0):
 *     N = sum_{lo<=i<hi} mult_i,  NP = sum_{lo<=i<hi} mult_i npig_i,  F_j = sum_{j'<j} w_j' [not matched],
 *     tp_at[r] = sum_j w_j [matched] [(double)F_j / (double)N <= fppi_thrs[r]],
 *     and tp_at[r] = TP_tot when there is a weighted entry and the first one's first copy (F = 1 for an unmatched entry, 0 for a matched
 *     one) is not below fppi_thrs[r]: the evaluator's index -1 reads the last operating point.
 *   Out: tp_at i64 [B][C][R]; totals i64 [B][C][4] = N, NP, TP_tot, FP_tot; valid i32 [B][C] = 1, or 0 when NP = 0 (tp_at 0: the
 *   evaluator leaves such a cell at -1), or -1 when the cell is not a range inside [0, I] (tp_at and totals 0).
 *   Counts are int32 inside (n_list * 255 must fit) and int64 outside: the same bytes whatever B and C are.  One workgroup per
 *   replicate, one wavefront per cell; C <= PE_LAMR_BOOTSTRAP_MAX_CELLS, R <= PE_LAMR_BOOTSTRAP_MAX_R,
 *   I <= PE_AP_BOOTSTRAP_MAX_IMAGES, n_list <= (2^31 - 1) / 255, B * C < 2^31, else PE_ERR_UNSUPPORTED.  B = 0 or C = 0: PE_OK, nothing
 *   is done; n_list = 0 with NULL lists is legal.
 * ------------------------------------------------------------------------------------------- */
#define PE_LAMR_BOOTSTRAP_MAX_CELLS 16
#define PE_LAMR_BOOTSTRAP_MAX_R 16
int pe_lamr_bootstrap(const int32_t* list_img, const uint8_t* list_flags, int64_t n_list, const int32_t* npig, const uint8_t* mult,
                      int32_t B, int32_t I, const double* fppi_thrs, int32_t R, const int32_t* cells, int32_t C, int64_t* tp_at,
                      int64_t* totals, int32_t* valid, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weighted boxes fusion, batched over images: R. Solovyev, W. Wang, T. Gabruseva, "Weighted boxes fusion: Ensembling
 * boxes from different object detection models", Image and Vision Computing 107 (2021), section 3.  Not in the reference - its
 * weighted_box_fusion (demo/FLIR/demo_probEn.py:73-77) is the score-weighted average of a ProbEn cluster's boxes, PE_BOX_SAVG here, and
 * is not this method.  The late-fusion baseline ProbEn is compared against, on the same rows.
 *
 * pe_wbf_fuse_batch: rows of image b are [offsets[b], offsets[b+1]) (or offsets[b] + [0, row_counts[b])) of the flat arrays, in detector
 *   order; row_source i32 [Ntot] the detector index of each row; det_weights DEVICE f64 [num_detectors] (u: finite, >= 0, not all 0 - a
 *   device pointer, so the caller's contract; options.FusionOptions validates it).  float64, every operation rounded on its own, in
 *   this order:
 *     U = u[0] + u[1] + ...;  s = score * u[source]
 *     a row is skipped - counted in out_skipped[b], out_cluster = -1 - when source is outside [0, num_detectors), class is outside
 *     [0, num_classes), a coordinate or s is not finite, !(s > 0), or s < skip_thresh (s == skip_thresh is kept)
 *     the kept rows are visited by s descending, ties by original index descending; classes are independent; a cluster holds S, X[4], n
 *     and the fused box F[k] = X[k] / S; a visited row with box b is tested against every cluster of its class, in creation order:
 *       w = fmax(0, fmin(F.x2, b.x2) - fmax(F.x1, b.x1)), h likewise, inter = w * h
 *       iou = inter / ((F.x2 - F.x1) * (F.y2 - F.y1) + (b.x2 - b.x1) * (b.y2 - b.y1) - inter)
 *     the first maximum of iou (a NaN never wins) > iou_thresh (strict): the row joins that cluster, S += s, X[k] += s * b[k], n += 1,
 *     F[k] = X[k] / S; else it opens a new cluster from zeros by the same update
 *     conf = ((S / (double)n) * fmin((double)n, U)) / U
 *   Output rows of image b, at [offsets[b], offsets[b] + out_counts[b]): the clusters by conf descending, ties by class ascending, then
 *   creation order (a NaN conf first).  out_boxes = F, out_scores = (float)conf, out_classes = (float)class, out_members = n;
 *   out_cluster[offsets[b] + r] = the output row (image-local) of the cluster input row r ended in.  No passthrough split: an image
 *   on which one detector fired is fused like any other (a lone row ends at s * min(1, U) / U).  out_counts[b] = -1 and
 *   out_skipped[b] = 0, nothing else written, if the image has more than max_rows_per_image rows.
 *   One 1024-thread workgroup per image, a wavefront per class (class mod 16), a lane per cluster; 164 bytes of LDS per row at every
 *   num_classes: 160 KiB hold PE_WBF_MAX_ROWS rows per image.  max_rows_per_image above it, num_detectors above PE_WBF_MAX_DETECTORS
 *   and num_images above PE_WBF_MAX_IMAGES (a launch's thread count must stay below 2^32) return PE_ERR_UNSUPPORTED with the capacity
 *   in the message; num_images = 0 returns PE_OK.  Arguments are checked before any device work.  No floating-point atomics: the
 *   results of an image depend on its own rows only.
 * ------------------------------------------------------------------------------------------- */
#define PE_WBF_MAX_DETECTORS 8
#define PE_WBF_MAX_ROWS 996
#define PE_WBF_MAX_IMAGES 4194303
int pe_wbf_fuse_batch(const double* boxes,        /* [Ntot,4] xyxy */
                      const double* scores,       /* [Ntot] */
                      const int32_t* classes,     /* [Ntot] */
                      const int32_t* row_source,  /* [Ntot] */
                      const int32_t* offsets,     /* [B+1] (or [B] when row_counts is given) */
                      const int32_t* row_counts,  /* optional [B] */
                      int32_t num_images, int32_t num_classes, int32_t max_rows_per_image,
                      const double* det_weights,  /* DEVICE [num_detectors] */
                      int32_t num_detectors, double iou_thresh, double skip_thresh,
                      double* out_boxes,          /* [Ntot,4] */
                      float* out_scores,          /* [Ntot] */
                      float* out_classes,         /* [Ntot] */
                      int32_t* out_counts,        /* [B] */
                      int32_t* out_cluster,       /* [Ntot] */
                      int32_t* out_members,       /* [Ntot] */
                      int32_t* out_skipped,       /* [B] */
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * Probability-based Detection Quality: D. Hall et al., "Probabilistic object detection: definition and evaluation",
 * WACV 2020, for box ground truth and one scalar box variance per detection.  Not in the reference, and restated from the paper: the
 * rule below is the specification, tests/pdq_ref.py restates it in NumPy.
 *
 * pe_pdq_pair_quality: detections of image b are rows [det_offsets[b], det_offsets[b+1]) of det_boxes f64 [M,4] XYXY, det_vars f64 [M]
 *   (box-delta units, already scaled) and det_log_probs f64 [M, K+1]; its ground truths are [gt_offsets[b], gt_offsets[b+1]) of gt_boxes
 *   f64 [G,4], gt_classes i32 [G], gt_crowd i32 [G]; image_hw i32 [B,2] = (H, W); pair_offsets i64 [B+1], pair_offsets[b+1] -
 *   pair_offsets[b] = G_b * M_b; pair (g, d) of image b is at pair_offsets[b] + g_local * M_b + d_local.  float64, built without fused
 *   multiply-adds.  With (wx, wy, ww, wh) = bbox_reg_weights_host (null: 10, 10, 5, 5, as pe_variance_stats), eps = 1e-14,
 *   Phi(z) = 0.5 erfc(-z / sqrt 2), Phic(z) = 0.5 erfc(z / sqrt 2):
 *     sx = sqrt(var) * (x2 - x1) * sqrt(1 / wx^2 + 1 / (4 ww^2)), sy likewise with y, wy, wh
 *     column u: a = (u + 0.5 - x1) / sx, b = (x2 - u - 0.5) / sx, px[u] = Phi(a) Phi(b), qx[u] = Phic(a) + Phi(a) Phic(b);
 *       sx == 0: px[u] = 1 where x1 <= u + 0.5 <= x2 else 0, qx = 1 - px; rows v the same: py, qy
 *     P(v, u) = px[u] py[v], Q(v, u) = qx[u] + px[u] qy[v]
 *     a ground truth's pixels S_g: x1g <= u + 0.5 < x2g, y1g <= v + 0.5 < y2g inside the image, n_g of them
 *     FG = (1 / n_g) sum over S_g of log max(P, eps);  BG = (1 / n_g) sum over {P > tau} \ S_g (inside the image) of log max(Q, eps)
 *     (log max(P, eps) is evaluated as log1p(-Q) where P > 0.5 and log max(Q, eps) as log1p(-P) where Q > 0.5)
 *     Q_S = exp(FG + BG), Q_L = exp(det_log_probs[d][class_g]), q = sqrt(Q_S * Q_L)
 *   out_q, out_fg = exp(FG), out_bg = exp(BG), out_label = Q_L: f64 [num_pairs].
 *   A ground truth is ignored - out_gt_live i32 [G] = 0, counted in out_flags[2], out_flags[3] = 1 + the index of one of them - when
 *   gt_crowd is set, n_g == 0, a coordinate is not finite or its class is outside [0, K); a detection is excluded - counted in
 *   out_flags[0], out_flags[1] = 1 + the index of one - when a coordinate is not finite, its width or height is not > 0, or its variance is
 *   negative or not finite.  The four outputs are 0 for every pair of an ignored ground truth or an excluded detection.
 *   max_width_plus_height sizes the tables in LDS (16 bytes per column and per row): above PE_PDQ_MAX_TABLE it is refused; an image with
 *   H < 1, W < 1 or W + H above it has its detections excluded and its ground truths ignored.  Offsets are device memory: an image whose
 *   offsets would leave the arrays is left unwritten.  One 256-thread workgroup per detection (the four tables once, then the sum over
 *   {P > tau}, then per ground truth the sums over its own rectangle) and ceil(G / 256) more for out_gt_live.  No floating-point
 *   atomics: the same input gives the same bits.  Arguments are checked before any device work.
 *
 * pe_pdq_assign (HOST pointers, no device work): per image the one-to-one assignment of the ground truths with gt_live != 0 to the
 *   detections with det_take != 0 (null: all) that maximises the sum of q, by the O(n^3) Hungarian algorithm on the block in either
 *   orientation; a q that is not > 0 counts as 0.  out_match i32 [G] = the detection's row index, or -1 (not live, unassigned, or
 *   assigned at q = 0).  The offsets must start at 0, rise, and end at the counts; pair_offsets must span G_b * M_b per image.
 * ------------------------------------------------------------------------------------------- */
#define PE_PDQ_MAX_TABLE 4096
int pe_pdq_pair_quality(const double* det_boxes, const double* det_vars, const double* det_log_probs, const int32_t* det_offsets,
                        const double* gt_boxes, const int32_t* gt_classes, const int32_t* gt_crowd, const int32_t* gt_offsets,
                        const int32_t* image_hw, const int64_t* pair_offsets, int32_t num_images, int32_t num_classes, int32_t num_dets,
                        int32_t num_gt, int64_t num_pairs, int32_t max_width_plus_height, const float* bbox_reg_weights_host, double tau,
                        double* out_q, double* out_fg, double* out_bg, double* out_label, int32_t* out_gt_live, int32_t* out_flags,
                        void* stream);
int pe_pdq_assign(const double* q_host, const int32_t* gt_live_host, const int32_t* det_take_host, const int32_t* det_offsets_host,
                  const int32_t* gt_offsets_host, const int64_t* pair_offsets_host, int32_t num_images, int32_t num_dets, int32_t num_gt,
                  int64_t num_pairs, int32_t* out_match_host);

/* ---------------------------------------------------------------------------------------------
 * TIDE error typing: D. Bolya, S. Foley, J. Hays, J. Hoffman, "TIDE: A General Toolbox for Identifying Object Detection
 * Errors", ECCV 2020, for this project's evaluator.  Not in the reference, and restated from the paper: the rule below is the
 * specification, tests/tide_ref.py restates it in NumPy.
 *
 * pe_tide_classify: the detections of image b are rows [det_offsets[b], det_offsets[b+1]) of det_boxes f64 [M,4] XYWH and det_cats
 *   i32 [M] (device), in the caller's total order (descending score, NaN last, ties by category, then by the evaluator's rank); its
 *   ground truths are rows [gt_offsets[b], gt_offsets[b+1]) of gt_boxes f64 [G,4] XYWH, gt_cats i32 [G], gt_crowd u8 [G] (device), in
 *   annotation order.  det_offsets_host / gt_offsets_host i32 [num_images + 1] are HOST arrays: they are checked (start at 0, rise,
 *   end at num_dets / num_gt, the limits below) before any device work, then copied into offsets_ws, DEVICE i32 [2 (num_images + 1)],
 *   on the stream.  0 <= t_b < t_f <= 1.  float64, every operation rounded on its own.
 *   A. base matching = cocoeval.py:236-313 at one threshold with every non-crowd ground truth counted (area range "all"), category
 *      by category, detections in order: among the unmatched non-crowd ground truths of the detection's category with
 *      inter / (a_d + a_g - inter) >= min(t_f, 1 - 1e-10) the largest, the LATER one on a tie; if there is none, the same among its
 *      crowd ground truths with inter / a_d (a crowd box may be matched repeatedly).  The quotient is used unguarded; the evaluator's
 *      comparison lets a NaN through and then every later candidate, which is kept: with a NaN among a group's candidates the group's
 *      last candidate is taken.
 *   B. every unmatched detection is typed on iou = inter > 0 ? inter / (a_d + a_g - inter) : 0 against the image's non-crowd ground
 *      truths: own / other = the largest iou (>= 0) over those of its category / of the other categories, the LOWEST index on a tie,
 *      0 with partner -1 if there is none.  First hit: Loc t_b <= own < t_f (partner own's); Cls other >= t_f (other's); Dupe
 *      own >= t_f (own's); Bkg other < t_b; Both otherwise.
 *   C. a non-crowd ground truth is missed when A left it unmatched and it is the partner of no Loc and of no Cls error.
 *   D. two independent walks in the total order, over the Loc errors and over the Cls errors: an error claims its partner if A left
 *      the partner unmatched and no earlier error of the same walk claimed it.
 *   Out, i32: out_match [M] the image-local ground-truth index of A or -1; out_type [M] PE_TIDE_TP (matched), PE_TIDE_IGNORED (matched
 *   to a crowd box) or the error type; out_partner [M] image-local, -1 for matched, Bkg and Both; out_claim [M] 0 / 1;
 *   out_gt [G] bits: 1 matched in A, 2 partner of a Loc error, 4 partner of a Cls error, 8 missed.
 *   One 256-thread workgroup per image, ground truths in LDS (47 KiB): an image with more than PE_TIDE_MAX_GT ground truths or
 *   PE_TIDE_MAX_DETS detections (100 per category at PE_TIDE_MAX_CLASSES categories), or num_classes above PE_TIDE_MAX_CLASSES,
 *   returns PE_ERR_UNSUPPORTED before anything is launched; num_images = 0 returns PE_OK.  Nothing is shared between workgroups and
 *   there are no floating-point atomics: an image's output does not depend on the rest of the launch.
 * ------------------------------------------------------------------------------------------- */
#define PE_TIDE_MAX_DETS 8000
#define PE_TIDE_MAX_GT 1024
#define PE_TIDE_MAX_CLASSES 80
#define PE_TIDE_TP 0
#define PE_TIDE_CLS 1
#define PE_TIDE_LOC 2
#define PE_TIDE_BOTH 3
#define PE_TIDE_DUPE 4
#define PE_TIDE_BKG 5
#define PE_TIDE_IGNORED 6
int pe_tide_classify(const double* det_boxes, const int32_t* det_cats, const int32_t* det_offsets_host, const double* gt_boxes,
                     const int32_t* gt_cats, const uint8_t* gt_crowd, const int32_t* gt_offsets_host, int32_t num_images,
                     int32_t num_classes, int32_t num_dets, int32_t num_gt, double t_f, double t_b, int32_t* offsets_ws,
                     int32_t* out_match, int32_t* out_type, int32_t* out_partner, int32_t* out_claim, int32_t* out_gt, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PROBEN_HIP_H */