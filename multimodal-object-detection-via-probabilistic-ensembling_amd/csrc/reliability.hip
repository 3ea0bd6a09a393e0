// Reliability statistics of a calibrated score (gfx950): per confidence bin the rows, the correct rows, the sum of the confidences
// and the sum of the Brier terms - what a reliability diagram, ECE, MCE and the Brier score are made of (calibration.py sums them up).
//   pe_reliability_logits : conf from softmax(logits / T) (csrc/softmax_row.h: a row carries the bits pe_calibrated_softmax gives it),
//                           the detection's own class when `classes` is given, the top label otherwise
//   pe_reliability_scores : conf and correct given (the fused detections, whose score comes from the fuse kernel)
// Both are reliability_kernel<Source>: the source says which lane owns which row and what its (conf, correct) is; binning and the
// reduction are one piece of code.  Built with -ffp-contract=off: the Brier term d * d is two IEEE operations, as in NumPy.
//
// Summation order (no floating-point atomics anywhere; the same input gives the same bits):
//   1. The per-wavefront table lives in registers: lane b of a wavefront holds bin b (num_bins <= 64 = the wavefront).  Wavefront v of
//      the grid (v = 4 * workgroup + wave) takes row groups v, v + waves, ... in that order; inside a group the owner lanes take turns in
//      lane order, which is row order: the row's (bin, conf, term) is broadcast and the one lane whose index is the bin adds it.
//      So a wavefront adds its rows in ascending row order.
//   2. A workgroup adds its 4 wavefronts in wavefront order (LDS) into its 4 B slots of the workspace: [counts B x 2 | sums B x 2] =
//      per bin (rows, correct) as int64, then per bin (sum conf, sum term).
//   3. pe::launch_finish (csrc/reduce2.h) adds the workgroups: the order is stated there.
// The grid is min(ceil(num_rows / 256), PE_RELIABILITY_MAX_BLOCKS), a function of num_rows alone.  Counts are integers: exact in any order.
#include "common.h"
#include "reduce2.h"
#include "softmax_row.h"

namespace {

constexpr int kRelThreads = 256, kRelWaves = kRelThreads / 64;
constexpr int kRelRowsPerBlock = 256;          // sizes the grid only: which rows a wavefront takes is the source's row grouping

enum RowState { kNoRow = 0, kRowUsed = 1, kRowExcluded = 2 };

// conf from the logits.  K + 1 <= 64: the row-to-lane-group mapping of calibrated_softmax_kernel (a group of G lanes per row, 64 / G rows
// per wavefront), the group's first lane owns the row.  Above: a lane per row.
struct LogitsSource {
    const float* logits;
    const int32_t* labels;
    const int32_t* classes;     // NULL: top label
    int k1;
    double T;
    static constexpr const char* kInputs = "logits / labels";

    __device__ int rows_per_group() const { return k1 <= 64 ? 64 / pe::group_width(k1) : 64; }

    // the serial row of pe::softmax_serial, expression for expression (z, m, s and p as there), for the one thing it has no output
    // for: the largest p_k and the first index that attains it.  Bit-equal p: tests/test_reliability_gpu.py holds K + 1 = 65 to
    // pe_calibrated_softmax's output.
    __device__ double serial_top(const float* row, int* index) const {
        double m = pe::kNegInf;
        for (int k = 0; k < k1; ++k) {
            const double z = (double)row[k] / T;
            m = (z > m || z != z) ? z : m;
        }
        double s = 0.0;
        for (int k = 0; k < k1; ++k) s += exp((double)row[k] / T - m);
        double best = exp((double)row[0] / T - m) / s;
        int bi = 0;
        for (int k = 1; k < k1; ++k) {
            const double p = exp((double)row[k] / T - m) / s;
            if (p > best || p != p) { best = p; bi = k; }      // strict: the first index keeps an equal maximum; NaN wins (the row is excluded)
        }
        *index = bi;
        return best;
    }

    // every lane of the wavefront calls this (the group path shuffles wave-wide)
    __device__ int fetch(long long r0, long long M, int lane, long long* row_index, double* conf, int* correct) const {
        if (k1 <= 64) {
            const int G = pe::group_width(k1), col = lane & (G - 1);
            const long long r = r0 + lane / G;
            const bool live = r < M;
            const double p = pe::softmax_group<false>(logits + r * k1, live, col, k1, G, T);
            const int y = live ? labels[r] : 0;
            const int c = (live && classes) ? classes[r] : 0;
            const bool ids_ok = y >= 0 && y < k1 && c >= 0 && c < k1;
            double cf;
            int pred;
            if (classes) {
                cf = __shfl(p, (lane - col) + (ids_ok ? c : 0));      // the group's lane that holds column c
                pred = c;
            } else {
                cf = p;                                               // padding lanes hold 0 (NaN on a NaN row) under an index >= K + 1
                pred = col;
                for (int o = G >> 1; o > 0; o >>= 1) {
                    const double v = __shfl_xor(cf, o);
                    const int vi = __shfl_xor(pred, o);
                    if (v > cf || v != v || (v == cf && vi < pred)) { cf = v; pred = vi; }      // the first index keeps an equal maximum
                }
            }
            *row_index = r;
            *conf = cf;
            *correct = pred == y;
            if (!live || col != 0) return kNoRow;
            return (ids_ok && cf == cf) ? kRowUsed : kRowExcluded;
        }
        const long long r = r0 + lane;
        *row_index = r;
        if (r >= M) return kNoRow;
        const int y = labels[r];
        const int c = classes ? classes[r] : 0;
        if (y < 0 || y >= k1 || c < 0 || c >= k1) return kRowExcluded;
        int pred = c;
        const double cf = classes ? pe::softmax_serial(logits + r * k1, k1, T, nullptr, 0, c) : serial_top(logits + r * k1, &pred);
        *conf = cf;
        *correct = pred == y;
        return cf == cf ? kRowUsed : kRowExcluded;
    }
};

struct ScoresSource {
    const double* conf;
    const int32_t* correct;
    static constexpr const char* kInputs = "conf / correct";

    __device__ int rows_per_group() const { return 64; }

    __device__ int fetch(long long r0, long long M, int lane, long long* row_index, double* cf, int* ok) const {
        const long long r = r0 + lane;
        *row_index = r;
        if (r >= M) return kNoRow;
        const double c = conf[r];
        *cf = c;
        *ok = correct[r] != 0;
        return (c >= 0.0 && c <= 1.0) ? kRowUsed : kRowExcluded;          // NaN fails both
    }
};

template <class Source>
__global__ __launch_bounds__(kRelThreads) void reliability_kernel(Source src, long long M, int B, double* workspace, int32_t* flags) {
    __shared__ long long wave_counts[kRelWaves][64][2];
    __shared__ double wave_sums[kRelWaves][64][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rpg = src.rows_per_group();
    const long long wave = (long long)blockIdx.x * kRelWaves + w, waves = (long long)gridDim.x * kRelWaves;
    long long n = 0, n_correct = 0;        // this lane's bin
    double sum_conf = 0.0, sum_term = 0.0;
    for (long long r0 = wave * rpg; r0 < M; r0 += waves * rpg) {          // wave-uniform
        long long r = 0;
        double conf = 0.0;
        int correct = 0;
        const int state = src.fetch(r0, M, lane, &r, &conf, &correct);
        if (state == kRowExcluded) pe::flag_excluded(flags, r);
        const bool used = state == kRowUsed;
        const double d = conf - (correct ? 1.0 : 0.0);
        const double term = d * d;
        const int bin = used ? min((int)(conf * (double)B), B - 1) : 0;
        const int key = bin * 2 + (correct ? 1 : 0);
        // the owner lanes take turns in lane order = row order; every lane sees the row, the lane whose index is its bin adds it
        for (unsigned long long todo = __ballot(used); todo; todo &= todo - 1) {
            const int from = __ffsll((long long)todo) - 1;
            const int k = __shfl(key, from);
            const double c = __shfl(conf, from);
            const double t = __shfl(term, from);
            if (lane == (k >> 1)) {
                n += 1;
                n_correct += k & 1;
                sum_conf += c;
                sum_term += t;
            }
        }
    }
    wave_counts[w][lane][0] = n;
    wave_counts[w][lane][1] = n_correct;
    wave_sums[w][lane][0] = sum_conf;
    wave_sums[w][lane][1] = sum_term;
    __syncthreads();
    if ((int)threadIdx.x < B) {
        long long c0 = wave_counts[0][lane][0], c1 = wave_counts[0][lane][1];
        double s0 = wave_sums[0][lane][0], s1 = wave_sums[0][lane][1];
        for (int v = 1; v < kRelWaves; ++v) {
            c0 += wave_counts[v][lane][0]; c1 += wave_counts[v][lane][1];
            s0 += wave_sums[v][lane][0]; s1 += wave_sums[v][lane][1];
        }
        double* o = workspace + (size_t)blockIdx.x * B * 4 + lane * 2;
        reinterpret_cast<long long*>(o)[0] = c0;
        reinterpret_cast<long long*>(o)[1] = c1;
        o[2 * B] = s0;
        o[2 * B + 1] = s1;
    }
}

// the checks the two entry points share (after their own), the zeroing and the two launches
template <class Source>
int reliability_impl(const char* what, const Source& src, bool data_ok, int64_t num_rows, int32_t num_bins, double* workspace,
                     int64_t* out_counts, double* out_sums, int32_t* out_flags, void* stream) {
    PE_CHECK_ARG(num_bins >= 1 && num_bins <= PE_RELIABILITY_MAX_BINS, "%s: num_bins %d not in [1,%d]", what, num_bins,
                 PE_RELIABILITY_MAX_BINS);
    PE_CHECK_ARG(num_rows >= 0, "%s: num_rows %lld", what, (long long)num_rows);
    hipStream_t st = (hipStream_t)stream;
    if (num_rows == 0) {      // nothing to read: the outputs that are given are zeroed
        if ((out_counts && hipMemsetAsync(out_counts, 0, (size_t)num_bins * 2 * sizeof(int64_t), st) != hipSuccess) ||
            (out_sums && hipMemsetAsync(out_sums, 0, (size_t)num_bins * 2 * sizeof(double), st) != hipSuccess) ||
            (out_flags && hipMemsetAsync(out_flags, 0, 2 * sizeof(int32_t), st) != hipSuccess)) {
            pe::set_error("%s: hipMemsetAsync of the outputs failed", what);
            return PE_ERR_HIP;
        }
        return PE_OK;
    }
    PE_CHECK_ARG(data_ok, "%s: null pointer (%s)", what, Source::kInputs);
    PE_CHECK_ARG(workspace && out_counts && out_sums && out_flags, "%s: null pointer (workspace / out_counts / out_sums / out_flags)", what);
    // the grid is a function of num_rows alone: same input, same partition, same bits
    const int blocks = (int)std::min<long long>((num_rows + kRelRowsPerBlock - 1) / kRelRowsPerBlock, PE_RELIABILITY_MAX_BLOCKS);
    if (int rc = pe::zero_flags(out_flags, st, what)) return rc;
    hipLaunchKernelGGL(reliability_kernel<Source>, dim3(blocks), dim3(kRelThreads), 0, st, src, (long long)num_rows, (int)num_bins,
                       workspace, out_flags);
    PE_CHECK_LAUNCH(what);
    return pe::launch_finish(workspace, blocks, 4 * num_bins, 2 * num_bins, reinterpret_cast<long long*>(out_counts), out_sums, st, what);
}

}  // namespace

extern "C" int pe_reliability_logits(const float* logits, const int32_t* labels, const int32_t* classes, int64_t num_rows,
                                     int32_t num_columns, double temperature, int32_t num_bins, double* workspace, int64_t* out_counts,
                                     double* out_sums, int32_t* out_flags, void* stream) {
    PE_CHECK_ARG(pe::finite_positive(temperature), "pe_reliability_logits: temperature %g is not finite and > 0", temperature);
    PE_CHECK_ARG(num_columns >= 2, "pe_reliability_logits: num_columns %d (K + 1) < 2", num_columns);
    const LogitsSource src{logits, labels, classes, (int)num_columns, temperature};
    return reliability_impl("pe_reliability_logits", src, logits && labels, num_rows, num_bins, workspace, out_counts, out_sums, out_flags,
                            stream);
}

extern "C" int pe_reliability_scores(const double* conf, const int32_t* correct, int64_t num_rows, int32_t num_bins, double* workspace,
                                     int64_t* out_counts, double* out_sums, int32_t* out_flags, void* stream) {
    const ScoresSource src{conf, correct};
    return reliability_impl("pe_reliability_scores", src, conf && correct, num_rows, num_bins, workspace, out_counts, out_sums, out_flags,
                            stream);
}
