// Temperature calibration of the detectors' class posteriors (gfx950).
//   pe_proben_pack_logits   : pe_proben_pack_detections with p = softmax(logits / T_d) in float64 in place of the float32 prob_score
//   pe_calibrated_softmax   : the same row arithmetic over a flat [M, K+1] tensor (all K+1 columns stored)
//   pe_proben_pack_log_posteriors / pe_log_softmax : the two above with log p_k = z_k - m - log(sum_j e_j) stored for all K+1 columns
//                             (the input of the log-posterior fusion, pe_proben_fuse_batch_logp in csrc/proben.hip)
//   pe_temperature_nll      : sum_i -log softmax(logits_i / T)[label_i] and d/d(log T), for up to 64 candidate T in one launch
//
// Row arithmetic (one definition, softmax_group / softmax_serial, shared by the first two entry points so a row gets the same bits
// from either): z_k = (double)logit_k / T, m = max_k z_k, e_k = exp(z_k - m), p_k = e_k / sum_j e_j.  For K+1 <= 64 a row is held
// by a power-of-two group of lanes, one column per lane, and max and sum are xor-butterflies over the group: every lane of the group
// ends with the same bits (a + b == b + a at every level), the logits of the group's rows are read coalesced and 64 / G rows are
// in flight per wavefront.  Above 64 columns a lane walks its row serially.  Nothing is clamped: a NaN or +inf logit (or a row of
// -inf) gives NaN probabilities like the float64 NumPy expression.  Built with -ffp-contract=off like the other ProbEn code.
// The log-posterior (LOGP instantiations) reuses z, m and the sum s of the same call: log p_k = (z_k - m) - log(s), finite for every
// finite logit (s is in [1, K+1]), where log(p_k) is -inf once p_k underflows and log(1 - sum p) is NaN on a saturated row.
#include "common.h"

namespace {

constexpr double kNegInf = -__builtin_huge_val();

__host__ __device__ __forceinline__ int group_width(int k1) {   // smallest power of two >= k1 (k1 <= 64)
    int g = 1;
    while (g < k1) g <<= 1;
    return g;
}

// One column of one row per lane; `row` = the row's K+1 logits (ignored when !live), col = lane % G.  Every lane of the wavefront
// calls this (the shuffles are wave-wide).  Returns p_col (0 on the padding lanes col >= k1); LOGP: *lp = log p_col.
template <bool LOGP = false>
__device__ __forceinline__ double softmax_group(const float* row, bool live, int col, int k1, int G, double T, double* lp = nullptr) {
    const bool real = live && col < k1;
    const double z = real ? (double)row[col] / T : kNegInf;
    double m = z;
    for (int o = G >> 1; o > 0; o >>= 1) {
        const double v = __shfl_xor(m, o);
        m = (v > m || v != v) ? v : m;          // NaN wins, like np.max
    }
    const double e = real ? exp(z - m) : 0.0;
    double s = e;
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (LOGP) *lp = (z - m) - log(s);
    return e / s;
}

// K+1 > 64: the lane owns the row.  Sum in column order; out[k] for k < n_store, returns p_want (want < 0: nothing).
// out_lp (optional): log p_k for all k1 columns.
__device__ __forceinline__ double softmax_serial(const float* row, int k1, double T, double* out, int n_store, int want,
                                                 double* out_lp = nullptr) {
    double m = kNegInf;
    for (int k = 0; k < k1; ++k) {
        const double z = (double)row[k] / T;
        m = (z > m || z != z) ? z : m;
    }
    double s = 0.0;
    for (int k = 0; k < k1; ++k) s += exp((double)row[k] / T - m);
    double pw = 0.0;
    for (int k = 0; k < k1; ++k) {
        const double p = exp((double)row[k] / T - m) / s;
        if (k < n_store) out[k] = p;
        if (k == want) pw = p;
    }
    if (out_lp) {
        const double ls = log(s);
        for (int k = 0; k < k1; ++k) out_lp[k] = ((double)row[k] / T - m) - ls;
    }
    return pw;
}

struct PackLogitsArgs {
    const float* boxes[4];
    const int32_t* classes[4];
    const float* logits[4];
    const float* vars[4];
    const int32_t* counts[4];
    double T[4];
    int nd, B, D, K, max_class, stride;
    double* ob;
    double* os;
    double* op;
    double* ov;
    int32_t* oc;
    int32_t* ooff;
    int32_t* ocnt;
    int32_t* osingle;
    double* olp;     // LOGP: [rows, K+1] log-posteriors
};

// one wavefront per image: the ordered compaction of proben_pack_kernel (csrc/proben.hip), then the chunk's 64 rows go through the
// softmax 64 / G at a time.  LOGP (pe_proben_pack_log_posteriors) stores the row's K+1 log-posteriors next to everything else.
// (proben_scale_vars_kernel, csrc/variance.hip, repeats this compaction to rewrite out_vars: keep the row order of the two in step)
template <bool LOGP>
__global__ __launch_bounds__(64) void proben_pack_logits_kernel(PackLogitsArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int k1 = a.K + 1;
    const int G = k1 <= 64 ? group_width(k1) : 0;
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
                a.ov[dst] = (double)a.vars[d][src];
                a.oc[dst] = cls;
            }
            if (G) {
                const int rows_per_pass = 64 / G, col = lane & (G - 1);
                const int top = min(64, c - base);
                for (int r0 = 0; r0 < top; r0 += rows_per_pass) {          // wave-uniform trip count
                    const int r = r0 + lane / G;                             // the chunk row this lane's group holds (< 64)
                    const bool live = ((m >> r) & 1ull) != 0;
                    const int rdst = __shfl(dst_local, r);
                    const int rcls = __shfl(cls, r);
                    const float* row = a.logits[d] + ((size_t)b * a.D + base + r) * k1;
                    double lp = 0.0;
                    const double p = softmax_group<LOGP>(row, live, col, k1, G, T, &lp);
                    if (live) {
                        const size_t o = (size_t)b * a.stride + rdst;
                        if (col < a.K) a.op[o * a.K + col] = p;
                        if (col == rcls) a.os[o] = p;
                        if (LOGP && col < k1) a.olp[o * k1 + col] = lp;
                    }
                }
            } else if (ok) {
                // a class outside [0, K] cannot index the row: its score is NaN rather than a neighbour's value
                const double pw = softmax_serial(a.logits[d] + src * k1, k1, T, a.op + dst * a.K, a.K, cls, LOGP ? a.olp + dst * k1 : nullptr);
                a.os[dst] = (cls >= 0 && cls < k1) ? pw : __builtin_nan("");
            }
            if (G && ok && (cls < 0 || cls >= k1)) a.os[dst] = __builtin_nan("");
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

// flat [M, k1] -> [M, k1]; 256 threads, grid-stride over row groups.  LOGP (pe_log_softmax): out = log p.
template <bool LOGP>
__global__ __launch_bounds__(256) void calibrated_softmax_kernel(const float* logits, long long M, int k1, double T, double* out) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (long long)gridDim.x * 4;
    if (k1 <= 64) {
        const int G = group_width(k1), rpp = 64 / G, col = lane & (G - 1);
        for (long long r0 = wave * rpp; r0 < M; r0 += waves * rpp) {      // wave-uniform
            const long long r = r0 + lane / G;
            const bool live = r < M;
            double lp = 0.0;
            const double p = softmax_group<LOGP>(logits + r * k1, live, col, k1, G, T, &lp);
            if (live && col < k1) out[r * k1 + col] = LOGP ? lp : p;
        }
    } else if (LOGP) {
        for (long long r = wave * 64 + lane; r < M; r += waves * 64) softmax_serial(logits + r * k1, k1, T, nullptr, 0, -1, out + r * k1);
    } else {
        for (long long r = wave * 64 + lane; r < M; r += waves * 64) softmax_serial(logits + r * k1, k1, T, out + r * k1, k1, -1);
    }
}

constexpr int kNllThreads = 256, kNllWaves = kNllThreads / 64;

struct NllArgs {
    const float* logits;
    const int32_t* labels;
    long long M;
    int k1, n_t;
    double T[64];
    double* partial;     // [blocks, n_t, 2]
    int32_t* flags;      // [0] rows with a label outside [0, K], [1] 1 + the largest such row index (saturating)
};

// Lane = candidate temperature, wavefront = row: the 64 lanes read the same logits (one cache line, broadcast) and each keeps its own
// two sums.  Wave w of block g takes rows g * kNllWaves + w, + gridDim.x * kNllWaves, ...: a fixed order for a fixed (M, grid).
__global__ __launch_bounds__(kNllThreads) void temperature_nll_kernel(NllArgs a) {
    __shared__ double part[kNllWaves][64][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const double T = a.T[lane < a.n_t ? lane : 0];
    double nll = 0.0, dnll = 0.0;
    const long long step = (long long)gridDim.x * kNllWaves;
    for (long long r = (long long)blockIdx.x * kNllWaves + w; r < a.M; r += step) {
        const int y = a.labels[r];
        if (y < 0 || y >= a.k1) {
            if (lane == 0) {
                atomicAdd(&a.flags[0], 1);
                atomicMax(&a.flags[1], (int)min(r + 1, (long long)0x7fffffff));
            }
            continue;
        }
        const float* row = a.logits + r * a.k1;
        double m = kNegInf;
        for (int k = 0; k < a.k1; ++k) {
            const double z = (double)row[k] / T;
            m = (z > m || z != z) ? z : m;
        }
        double s = 0.0, sz = 0.0;
        for (int k = 0; k < a.k1; ++k) {
            const double z = (double)row[k] / T;
            const double e = exp(z - m);
            s += e;
            sz += e * (z - m);
        }
        const double zy = (double)row[y] / T - m;
        nll += log(s) - zy;           // -log softmax(z)[y]
        dnll += zy - sz / s;          // d/d(log T): z_y - sum_k p_k z_k (the shift by m cancels)
    }
    part[w][lane][0] = nll;
    part[w][lane][1] = dnll;
    __syncthreads();
    if (threadIdx.x < a.n_t) {
        double s0 = part[0][lane][0], s1 = part[0][lane][1];
        for (int v = 1; v < kNllWaves; ++v) { s0 += part[v][lane][0]; s1 += part[v][lane][1]; }
        double* o = a.partial + ((size_t)blockIdx.x * a.n_t + lane) * 2;
        o[0] = s0;
        o[1] = s1;
    }
}

// second pass, one workgroup: segment g of the 16 adds its share of the blocks in block order, then candidate t adds the 16 segment
// sums in segment order - fixed for a fixed block count
constexpr int kFinishSegments = 16;

__global__ __launch_bounds__(64 * kFinishSegments) void temperature_nll_finish_kernel(const double* partial, int blocks, int n_t, double* out) {
    __shared__ double seg[kFinishSegments][64][2];
    const int t = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int per = (blocks + kFinishSegments - 1) / kFinishSegments;
    double s0 = 0.0, s1 = 0.0;
    if (t < n_t) {
        const int end = min(blocks, (g + 1) * per);
        for (int k = g * per; k < end; ++k) {
            s0 += partial[((size_t)k * n_t + t) * 2];
            s1 += partial[((size_t)k * n_t + t) * 2 + 1];
        }
    }
    seg[g][t][0] = s0;
    seg[g][t][1] = s1;
    __syncthreads();
    if (g == 0 && t < n_t) {
        s0 = seg[0][t][0];
        s1 = seg[0][t][1];
        for (int k = 1; k < kFinishSegments; ++k) { s0 += seg[k][t][0]; s1 += seg[k][t][1]; }
        out[t * 2] = s0;
        out[t * 2 + 1] = s1;
    }
}

bool good_temperature(double t) { return t == t && t > 0.0 && t < __builtin_huge_val(); }

// pe_proben_pack_logits / pe_proben_pack_log_posteriors: one body, `what` words the messages, logp selects the kernel
int pack_logits_impl(const char* what, const float* const* det_boxes_host, const int32_t* const* det_classes_host,
                     const float* const* det_logits_host, const float* const* det_vars_host, const int32_t* const* det_counts_host,
                     const double* temperatures_host, int32_t num_detectors, int32_t num_images, int32_t det_stride,
                     int32_t num_classes, int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores,
                     double* out_probs, double* out_vars, int32_t* out_classes, int32_t* out_offsets, int32_t* out_counts,
                     int32_t* out_single_source, double* out_log_probs, bool logp, void* stream) {
    PE_CHECK_ARG(num_detectors >= 1 && num_detectors <= 4, "%s: num_detectors %d", what, num_detectors);
    PE_CHECK_ARG(num_images >= 0 && det_stride >= 0, "%s: num_images %d, det_stride %d", what, num_images, det_stride);
    PE_CHECK_ARG(num_classes >= 1, "%s: num_classes %d", what, num_classes);
    PE_CHECK_ARG(row_stride >= num_detectors * det_stride, "%s: row_stride %d < %d", what, row_stride, num_detectors * det_stride);
    PE_CHECK_ARG(det_boxes_host && det_classes_host && det_logits_host && det_vars_host && det_counts_host && temperatures_host,
                 "%s: null pointer (detector tables / temperatures)", what);
    PE_CHECK_ARG(out_boxes && out_scores && out_probs && out_vars && out_classes && out_offsets && out_counts, "%s: null output", what);
    PE_CHECK_ARG(!logp || out_log_probs, "%s: null output (out_log_probs)", what);
    PackLogitsArgs a{};
    for (int d = 0; d < num_detectors; ++d) {
        PE_CHECK_ARG(good_temperature(temperatures_host[d]), "%s: temperature %g of detector %d is not finite and > 0", what,
                     temperatures_host[d], d);
        a.boxes[d] = det_boxes_host[d]; a.classes[d] = det_classes_host[d]; a.logits[d] = det_logits_host[d];
        a.vars[d] = det_vars_host[d]; a.counts[d] = det_counts_host[d]; a.T[d] = temperatures_host[d];
        PE_CHECK_ARG(a.boxes[d] && a.classes[d] && a.logits[d] && a.vars[d] && a.counts[d], "%s: null pointer of detector %d", what, d);
    }
    if (num_images == 0) return PE_OK;
    a.nd = num_detectors; a.B = num_images; a.D = det_stride; a.K = num_classes; a.max_class = max_class;
    a.stride = row_stride; a.ob = out_boxes; a.os = out_scores; a.op = out_probs; a.ov = out_vars; a.oc = out_classes;
    a.ooff = out_offsets; a.ocnt = out_counts; a.osingle = out_single_source; a.olp = out_log_probs;
    if (logp)
        hipLaunchKernelGGL(proben_pack_logits_kernel<true>, dim3(num_images), dim3(64), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(proben_pack_logits_kernel<false>, dim3(num_images), dim3(64), 0, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}

int flat_softmax_impl(const char* what, const float* logits, int64_t num_rows, int32_t num_columns, double temperature, double* out,
                      bool logp, void* stream) {
    PE_CHECK_ARG(good_temperature(temperature), "%s: temperature %g is not finite and > 0", what, temperature);
    PE_CHECK_ARG(num_rows >= 0, "%s: num_rows %lld", what, (long long)num_rows);
    PE_CHECK_ARG(num_columns >= 2, "%s: num_columns %d (K + 1) < 2", what, num_columns);
    if (num_rows == 0) return PE_OK;
    PE_CHECK_ARG(logits && out, "%s: null pointer", what);
    const int rows_per_wave = num_columns <= 64 ? 64 / group_width(num_columns) : 64;
    const long long waves = (num_rows + rows_per_wave - 1) / rows_per_wave;
    const int blocks = (int)std::min<long long>((waves + 3) / 4, 4096);
    if (logp)
        hipLaunchKernelGGL(calibrated_softmax_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, (long long)num_rows,
                           (int)num_columns, temperature, out);
    else
        hipLaunchKernelGGL(calibrated_softmax_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logits, (long long)num_rows,
                           (int)num_columns, temperature, out);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}

}  // namespace

extern "C" int pe_proben_pack_logits(const float* const* det_boxes_host, const int32_t* const* det_classes_host,
                                     const float* const* det_logits_host, const float* const* det_vars_host,
                                     const int32_t* const* det_counts_host, const double* temperatures_host,
                                     int32_t num_detectors, int32_t num_images, int32_t det_stride, int32_t num_classes,
                                     int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores,
                                     double* out_probs, double* out_vars, int32_t* out_classes, int32_t* out_offsets,
                                     int32_t* out_counts, int32_t* out_single_source, void* stream) {
    return pack_logits_impl("pe_proben_pack_logits", det_boxes_host, det_classes_host, det_logits_host, det_vars_host, det_counts_host,
                            temperatures_host, num_detectors, num_images, det_stride, num_classes, max_class, row_stride, out_boxes,
                            out_scores, out_probs, out_vars, out_classes, out_offsets, out_counts, out_single_source, nullptr, false,
                            stream);
}

extern "C" int pe_proben_pack_log_posteriors(const float* const* det_boxes_host, const int32_t* const* det_classes_host,
                                             const float* const* det_logits_host, const float* const* det_vars_host,
                                             const int32_t* const* det_counts_host, const double* temperatures_host,
                                             int32_t num_detectors, int32_t num_images, int32_t det_stride, int32_t num_classes,
                                             int32_t max_class, int32_t row_stride, double* out_boxes, double* out_scores,
                                             double* out_probs, double* out_log_probs, double* out_vars, int32_t* out_classes,
                                             int32_t* out_offsets, int32_t* out_counts, int32_t* out_single_source, void* stream) {
    return pack_logits_impl("pe_proben_pack_log_posteriors", det_boxes_host, det_classes_host, det_logits_host, det_vars_host,
                            det_counts_host, temperatures_host, num_detectors, num_images, det_stride, num_classes, max_class,
                            row_stride, out_boxes, out_scores, out_probs, out_vars, out_classes, out_offsets, out_counts,
                            out_single_source, out_log_probs, true, stream);
}

extern "C" int pe_calibrated_softmax(const float* logits, int64_t num_rows, int32_t num_columns, double temperature,
                                     double* out_probs, void* stream) {
    return flat_softmax_impl("pe_calibrated_softmax", logits, num_rows, num_columns, temperature, out_probs, false, stream);
}

extern "C" int pe_log_softmax(const float* logits, int64_t num_rows, int32_t num_columns, double temperature, double* out_log_probs,
                              void* stream) {
    return flat_softmax_impl("pe_log_softmax", logits, num_rows, num_columns, temperature, out_log_probs, true, stream);
}

extern "C" int pe_temperature_nll(const float* logits, const int32_t* labels, int64_t num_rows, int32_t num_columns,
                                  const double* temperatures_host, int32_t num_temperatures, double* workspace,
                                  double* out, int32_t* out_flags, void* stream) {
    PE_CHECK_ARG(num_temperatures >= 1 && num_temperatures <= 64, "pe_temperature_nll: num_temperatures %d not in [1,64]",
                 num_temperatures);
    PE_CHECK_ARG(temperatures_host, "pe_temperature_nll: null pointer (temperatures)");
    for (int t = 0; t < num_temperatures; ++t)
        PE_CHECK_ARG(good_temperature(temperatures_host[t]), "pe_temperature_nll: temperature %g (candidate %d) is not finite and > 0",
                     temperatures_host[t], t);
    PE_CHECK_ARG(num_rows >= 0, "pe_temperature_nll: num_rows %lld", (long long)num_rows);
    PE_CHECK_ARG(num_columns >= 2, "pe_temperature_nll: num_columns %d (K + 1) < 2", num_columns);
    PE_CHECK_ARG(workspace && out && out_flags, "pe_temperature_nll: null pointer (workspace / out / out_flags)");
    PE_CHECK_ARG(num_rows == 0 || (logits && labels), "pe_temperature_nll: null pointer (logits / labels)");
    NllArgs a{};
    a.logits = logits; a.labels = labels; a.M = num_rows; a.k1 = num_columns; a.n_t = num_temperatures;
    for (int t = 0; t < num_temperatures; ++t) a.T[t] = temperatures_host[t];
    a.partial = workspace; a.flags = out_flags;
    // the grid is a function of num_rows alone: same input, same partition, same bits
    const int blocks = (int)std::max<long long>(1, std::min<long long>((num_rows + kNllWaves - 1) / kNllWaves,
                                                                        PE_TEMPERATURE_NLL_MAX_BLOCKS));
    if (hipMemsetAsync(out_flags, 0, 2 * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
        pe::set_error("pe_temperature_nll: hipMemsetAsync of the flags failed");
        return PE_ERR_HIP;
    }
    hipLaunchKernelGGL(temperature_nll_kernel, dim3(blocks), dim3(kNllThreads), 0, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH("pe_temperature_nll");
    hipLaunchKernelGGL(temperature_nll_finish_kernel, dim3(1), dim3(64 * kFinishSegments), 0, (hipStream_t)stream, workspace, blocks,
                       (int)num_temperatures, out);
    PE_CHECK_LAUNCH("pe_temperature_nll (finish)");
    return PE_OK;
}
