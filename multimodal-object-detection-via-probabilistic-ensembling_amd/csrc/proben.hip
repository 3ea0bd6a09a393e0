// ProbEn late fusion for gfx950: ONE WORKGROUP PER IMAGE (one wavefront in rounds 1-4), whole per-image state in LDS.
//
// Replaces the reference's per-image NumPy loop (demo/FLIR/demo_probEn.py:92-187 nms_bayesian,
// :32-42 bayesian_fusion_multiclass, :24-30 bayesian_fusion, :73-77 weighted_box_fusion,
// :20-22 avg_bbox_fusion).  float64 throughout (the reference's NumPy dtype); compiled with
// -ffp-contract=off so IoU decisions round exactly like the reference's separate mul/add/div.
//
// Kernel shape: the greedy clustering is sequential in the pivot (<= N pivots per image) but its IoU tests are not - they
// use the rows' own geometry -, so parallelism comes from (a) the pair tests as ballots into bit matrices by all waves and a
// register-resident walk over them (or, when the matrices do not fit, 64 lanes scoring the pivot against 64 candidates per step),
// (b) per-row ranks / logs / geometry a thread per row, (c) the fusion formulas AFTER the clustering, a thread per cluster,
// (d) one workgroup per image, any number of images per launch.  Per image the HBM
// traffic is N*(4+1+K+1)*8 + N*4 bytes in and M*(32+4+4+4) bytes out; everything else stays in LDS.
#include "common.h"

namespace {

// First what every entry point passes, in the order the five C signatures share (a wrapper lists exactly these, max_rows as 0: it is
// fuse_impl's to set); then, defaulted to "absent", what only some pass: a wrapper assigns those it has by name.
struct ProbenArgs {
    const double *boxes = nullptr, *scores = nullptr, *probs = nullptr, *vars = nullptr;
    const int32_t *classes = nullptr, *offsets = nullptr, *row_counts = nullptr, *passthrough = nullptr;
    int32_t B = 0, K = 0, max_rows = 0, score_mode = 0, box_mode = 0;
    double thr = 0.0, fw = 0.0, fh = 0.0;
    double* out_boxes = nullptr;
    float *out_scores = nullptr, *out_classes = nullptr;
    int32_t *out_keep = nullptr, *out_counts = nullptr;
    const double* log_prior = nullptr;      // LOGP only: optional [K+1] log class prior (NULL = uniform)
    const int32_t* row_source = nullptr;    // POOL only: [Ntot] detector index of each row
    const double* pool_weights = nullptr;   // POOL only: [num_detectors] fusion exponents
    int32_t num_detectors = 0;              // POOL only
    int32_t* out_cluster = nullptr;         // POOL / POST, optional: [Ntot] output row of the cluster each input row ended in
    double* out_log_posterior = nullptr;    // POST only: [Ntot, K+1] the fused rows' normalised log-posterior
    double* out_vars = nullptr;             // POST only: [Ntot] the fused boxes' variance
    int32_t* out_members = nullptr;         // POST only: [Ntot] rows in the cluster
    const double* presence = nullptr;       // PRES only: [(1 << num_detectors) * (K+1)] log-evidence of each presence pattern (row 0 unused)
    int32_t* out_pattern = nullptr;         // PRES only, optional: [Ntot] the fused rows' presence pattern
};

// The dynamic LDS of one image, stated once: every array in order, for max_rows R (even, so that every array starts 8-byte aligned), L
// log-probability columns and the mode's optional arrays.  The kernel walks it with typed pointers into its LDS (LdsPointers), fuse_impl
// with byte counts (LdsBytes) for the size of either clustering form and the capacity it prints: the same statement gives both.  All
// arrays are indexed by SORTED position unless noted.
struct LdsPointers {
    template <typename T> using at = T*;
    unsigned char* next;
    template <typename T> __device__ T* take(size_t count) { T* p = reinterpret_cast<T*>(next); next = reinterpret_cast<unsigned char*>(p + count); return p; }
};
struct LdsBytes {
    template <typename T> using at = size_t;
    size_t next;
    template <typename T> size_t take(size_t count) { const size_t p = next; next += count * sizeof(T); return p; }
};
template <typename Cursor>
struct FuseLayout {
    template <typename T> using at = typename Cursor::template at<T>;
    at<unsigned long long> mbits, kbits;          // BITS: match [R][W] (then the clusters' member bits) and kill [R][W], W = 64-row words
    at<double> gx1, gy1, gx2, gy2, gar, gsc;      // [R]: class-band shifted corners, legacy "+1" area, score
    at<double> glog, gob, ginv, gw;               // [L][R] log-probabilities, [4][R] original coordinates, [R] 1 / variance, POOL: [R] weight
    at<int> ord, gcls, gsrc;                      // [R]: sorted position -> original row, class id, PRES: detector index (-1 = bad)
    at<unsigned short> members, cl_piv, cl_beg, cl_cnt;   // [R]: all clusters' matches back to back; per cluster pivot, first member, matches
    at<unsigned char> alive;                      // [R], sequential form only (the bit-matrix form leaves it unused)
    __host__ __device__ FuseLayout(Cursor c, int R, int L, bool pool, bool pres, bool bits) {
        const size_t matrix = bits ? (size_t)R * ((R + 63) >> 6) : 0;
        mbits = c.template take<unsigned long long>(matrix); kbits = c.template take<unsigned long long>(matrix);
        gx1 = c.template take<double>(R); gy1 = c.template take<double>(R); gx2 = c.template take<double>(R); gy2 = c.template take<double>(R);
        gar = c.template take<double>(R); gsc = c.template take<double>(R); glog = c.template take<double>((size_t)L * R);
        gob = c.template take<double>(4 * (size_t)R); ginv = c.template take<double>(R); gw = c.template take<double>(pool ? R : 0);
        ord = c.template take<int>(R); gcls = c.template take<int>(R); gsrc = c.template take<int>(pres ? R : 0);
        members = c.template take<unsigned short>(R); cl_piv = c.template take<unsigned short>(R);
        cl_beg = c.template take<unsigned short>(R); cl_cnt = c.template take<unsigned short>(R);
        alive = c.template take<unsigned char>(R);
    }
};
// The bytes of dynamic LDS at max_rows R (the last array and 16 bytes of slack), and what one more row costs in the sequential form
// (which is linear in R).
inline size_t fuse_lds_bytes(int R, int L, bool pool, bool pres, bool bits) { return FuseLayout<LdsBytes>(LdsBytes{0}, R, L, pool, pres, bits).alive + R + 16; }
inline size_t fuse_row_bytes(int L, bool pool, bool pres) { return (fuse_lds_bytes(2, L, pool, pres, false) - fuse_lds_bytes(0, L, pool, pres, false)) / 2; }
constexpr size_t kFuseLdsLimit = 160 * 1024;
constexpr size_t kFuseLdsStatic = 512;          // the kernels' static __shared__ scratch (ncl_s, reductions)

// Sort rule shared with oracle/proben.py: NaN first, score descending, ties by ORIGINAL index
// descending (== reversed stable ascending argsort, the reference's `argsort()[::-1]`).
__device__ __forceinline__ bool precedes(double sa, int ia, double sb, int ib) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return na;
    if (!na && sa != sb) return sa > sb;
    return ia > ib;
}

// One 1024-thread workgroup per image (one per CU; a step has 32 of them).  The rows' original boxes, 1 / variance and class ids
// are copied into LDS (by sorted position) next to the geometry: nothing after the second phase touches global memory (PE_SCORE_MAX
// excepted).  Phases: 1 rank sort (a thread per row), 2 geometry + logs (a thread per row), 3 clustering, 4 fusion (a thread per
// cluster).  Clustering, BITS form: (a) all 16 waves fill two bit matrices over the sorted rows, match[p][q] = IoU > thr and
// kill[p][q] = !(IoU <= thr) for q > p (a ballot per 64 candidates - the IoU tests use the rows' own geometry, never a fused box,
// so they do not depend on the order the pivots are visited in); (b) wave 0 walks the rows in order with the alive set in registers
// (lane w = rows 64w .. 64w+63): a live row becomes a pivot, its cluster = match row & alive, alive &= ~kill row - four rows'
// matrix lines are fetched per LDS round trip.  The sequential form (below, when the matrices do not fit the LDS) computes the
// IoUs inside the walk: ~1 500 cycles per row against ~100; with the rank sort on one wave that was 0.26 ms per step at the END
// of the step, where nothing overlaps it (profiles/r05_proben_phases.txt).
// LOGP (pe_proben_fuse_batch_logp, PE_SCORE_PROBEN_LOGP): a.probs holds the rows' K+1 LOG-posteriors, background column included.  Phase 2
// copies them into glog instead of taking logs of p and of 1 - sum(p), phase 4 normalises the cluster's summed columns with a
// max-subtracted log-sum-exp.  A template parameter, not a run-time branch: the four other score modes compile to what they were.
// POOL (pe_proben_fuse_batch_pooled, LOGP only): the logarithmic opinion pool.  Phase 2 stages the weight of the row's detector in gw
// beside glog (a source outside [0, num_detectors) stages NaN), phase 4 multiplies each member's log-posterior by it before the same
// sequential sum and takes the prior (W - 1) times, W the sequential sum of the members' weights.  1.0 * x is x and W is then the
// integer m, so weights of 1.0 give the LOGP bits.  out_cluster goes through LDS (the clustering's dead geometry array gx1) so that
// every input row is written once, by the thread that owns it.
// POST (pe_proben_fuse_batch_posterior, LOGP only, with or without POOL): the fused row keeps what phase 4 forms and used to drop.
// out_log_posterior[j] = (a_j - top) - log(tot), the K + 1 columns walked once more; out_vars = sum_t lambda_t^2 var_t, lambda_t the
// weight the box rule gives member t (v-avg: 1 / wsum with the box fusion's own wsum); out_members = m.  The rows' variances are
// staged (by sorted position) in the clustering's dead geometry array gy1 between phases 3 and 4, so phase 4 reads no more global
// memory than it did; a cluster of one and a passed-through row copy their input log-posterior and variance.  Every element is
// written once, by the thread that owns the cluster (or the row).  A template parameter: the other instantiations compile to what
// they were.
// PRES (pe_proben_fuse_batch_presence, LOGP only, with or without POOL / POST): presence evidence.  Phase 2 stages the row's detector
// index in gsrc (by sorted position, -1 for a source outside [0, num_detectors): 4 more bytes of LDS per row).  Phase 4 forms the
// cluster's pattern P = OR of (1 << source) over the members in cluster order and adds presence[P * (K + 1) + j], read from global
// memory like the prior, to a_j last, inside column(j); a member with a bad source makes every column NaN.  A cluster of ONE row is
// fused too: a_j = lp_j + presence[P][j] (no weight, no prior: what the pooled and the prior rule give a lone row today), score and
// class by the same rule over the K + 1 columns, out_log_posterior normalised; box, keep and variance stay the row's own.  A passthrough
// image is rescored the same way, a thread per row, each row a cluster of one: rows of one detector are never merged there.  Nothing
// before phase 4 reads the table, so the clusters at a zero table are the clusters at every table.  A template parameter: the other
// instantiations compile to what they were.
constexpr int kFuseThreads = 1024;

// np.max / np.argmax over value(0 .. n - 1): the first maximum in order; a NaN wins and ends the scan (so the first NaN).
struct FirstMax { int index; double value; };
template <typename Value>
__device__ __forceinline__ FirstMax first_max(Value value, int n) {
    FirstMax best{0, value(0)};
    bool bnan = best.value != best.value;
    for (int i = 1; i < n; ++i) {
        const double v = value(i);
        if (!bnan && (v != v || v > best.value)) { best.value = v; best.index = i; bnan = v != v; }
    }
    return best;
}

// The pair test every discrete decision of the clustering hangs on: IoU of a pivot and a candidate from the class-band shifted corners
// with the legacy "+1" widths and areas; match = IoU > thr joins the pivot's cluster, kill = !(IoU <= thr) leaves the pool (matched or NaN).
struct RowGeometry { double x1, y1, x2, y2, area; };
struct PairTest { bool match, kill; };
__device__ __forceinline__ PairTest pair_test(const RowGeometry& p, const RowGeometry& q, double thr) {
    const double w = fmax(0.0, fmin(p.x2, q.x2) - fmax(p.x1, q.x1) + 1.0);
    const double h = fmax(0.0, fmin(p.y2, q.y2) - fmax(p.y1, q.y1) + 1.0);
    const double inter = w * h;
    const double ovr = inter / (p.area + q.area - inter);
    return {ovr > thr, !(ovr <= thr)};
}

// A row's detector index where it is valid, else -1: what poisons the row's cluster in the pooled and the presence rule.
__device__ __forceinline__ int checked_source(int src, int num_detectors) { return (src >= 0 && src < num_detectors) ? src : -1; }

// The score / class rule of the log-posterior fusion over L columns a_j = column(j): NaN-wins maximum, max-subtracted sum, first maximum
// / first NaN of the normalised columns; lq (optional) takes the normalised log-posterior (a_j - top) - log(tot).  Phase 4 calls it for
// a cluster, the presence rule also for its clusters of one row (phase 4 and the passthrough branch).  In the presence kernels phase 4
// runs its own copy, so the rule is written twice: there a third inlined call made the pooled + posterior + presence instantiation 2 to
// 5 % slower (profiles/fuse_refactor.txt section 4).  The copy computes the same values by the same sums, subtractions and divisions
// in the same order; its maximum loop keeps the LAST NaN of the columns where first_max keeps the first, which only the payload of a
// NaN result could show (the kernel's own NaNs all carry one payload).
template <typename Column>
__device__ __forceinline__ void logp_rule(Column column, int L, double* lq, double& out_score, double& out_class) {
    const double top = first_max(column, L).value;          // NaN wins, like np.max
    double tot = 0.0;
    for (int j = 0; j < L; ++j) tot += exp(column(j) - top);
    const FirstMax best = first_max([&](int j) { return exp(column(j) - top) / tot; }, L);
    out_score = best.value;
    out_class = (double)best.index;
    if (lq) {
        const double ltot = log(tot);
        for (int j = 0; j < L; ++j) lq[j] = (column(j) - top) - ltot;
    }
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int l) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, l), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}

template <bool BITS, bool LOGP, bool POOL, bool POST, bool PRES>
__global__ __launch_bounds__(kFuseThreads) void proben_fuse_kernel(ProbenArgs a) {
    static_assert(LOGP || !POST, "the posterior output belongs to the log-posterior rule");
    static_assert(LOGP || !PRES, "presence evidence belongs to the log-posterior rule");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int ncl_s;
    const int img = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int beg = a.offsets[img];
    const int n = a.row_counts ? a.row_counts[img] : a.offsets[img + 1] - beg;
    if (n > a.max_rows || n < 0) {
        if (tid == 0) a.out_counts[img] = -1;
        return;
    }
    if (a.passthrough && a.passthrough[img]) {  // exactly one detector fired: rows pass through unchanged
        for (int r = tid; r < n; r += kFuseThreads) {
            const size_t o = (size_t)beg + r;
            for (int e = 0; e < 4; ++e) a.out_boxes[o * 4 + e] = a.boxes[o * 4 + e];
            if (PRES) {      // rescored as a cluster of one: a_j = lp_j + presence[1 << source][j]
                const int k1 = a.K + 1;
                const int src = checked_source(a.row_source[o], a.num_detectors);
                const bool ok = src >= 0;
                const int pat = ok ? 1 << src : 0;
                const double* lp = a.probs + o * k1;
                const double* prow = a.presence + (size_t)pat * k1;
                double sc, cl;
                logp_rule([&](int j) { return lp[j] + (ok ? prow[j] : __builtin_nan("")); }, k1, POST ? a.out_log_posterior + o * k1 : nullptr, sc, cl);
                a.out_scores[o] = (float)sc;
                a.out_classes[o] = (float)cl;
                if (a.out_pattern) a.out_pattern[o] = pat;
            } else {
                a.out_scores[o] = (float)a.scores[o];
                a.out_classes[o] = (float)a.classes[o];
            }
            a.out_keep[o] = r;
            if ((POOL || POST || PRES) && a.out_cluster) a.out_cluster[o] = r;
            if (POST) {
                if (!PRES)
                    for (int j = 0; j <= a.K; ++j) a.out_log_posterior[o * (a.K + 1) + j] = a.probs[o * (a.K + 1) + j];
                a.out_vars[o] = a.vars[o];
                a.out_members[o] = 1;
            }
        }
        if (tid == 0) a.out_counts[img] = n;
        return;
    }
    const int R = a.max_rows;
    const int K = a.K;
    const int W = (R + 63) >> 6;   // 64-row words per matrix line
    // columns of log-probabilities kept per row (0 when the score mode does not need them)
    const int L = (LOGP || a.score_mode == PE_SCORE_PROBEN) ? K + 1 : (a.score_mode == PE_SCORE_PROBEN_BINARY ? 2 : 0);
    const FuseLayout<LdsPointers> lay(LdsPointers{smem}, R, L, POOL, PRES, BITS);
    unsigned long long *mbits = lay.mbits, *kbits = lay.kbits;
    double *gx1 = lay.gx1, *gy1 = lay.gy1, *gx2 = lay.gx2, *gy2 = lay.gy2, *gar = lay.gar, *gsc = lay.gsc, *glog = lay.glog, *gob = lay.gob;
    double *ginv = lay.ginv, *gw = lay.gw;
    int *ord = lay.ord, *gcls = lay.gcls, *gsrc = lay.gsrc;
    unsigned short *members = lay.members, *cl_piv = lay.cl_piv, *cl_beg = lay.cl_beg, *cl_cnt = lay.cl_cnt;
    unsigned char* alive = lay.alive;
    auto geometry = [&](int p) { return RowGeometry{gx1[p], gy1[p], gx2[p], gy2[p], gar[p]}; };

    // ---- 1. rank sort by score (scores staged through gar, indexed by ORIGINAL row) ----
    for (int r = tid; r < n; r += kFuseThreads) gar[r] = a.scores[beg + r];
    __syncthreads();
    for (int r = tid; r < n; r += kFuseThreads) {
        const double s = gar[r];
        int rank = 0;
#pragma unroll 8
        for (int q = 0; q < n; ++q) rank += precedes(gar[q], q, s, r) ? 1 : 0;
        ord[rank] = r;
        gsc[rank] = s;
    }
    __syncthreads();
    // ---- 2. per-row geometry (class-band shifted, legacy "+1" area) and log-probabilities ----
    for (int p = tid; p < n; p += kFuseThreads) {
        const int r = ord[p];
        const double c = (double)a.classes[beg + r];
        const double* b = a.boxes + (size_t)(beg + r) * 4;
        const double x1 = b[0] + c * a.fw, y1 = b[1] + c * a.fh;
        const double x2 = b[2] + c * a.fw, y2 = b[3] + c * a.fh;
        gx1[p] = x1; gy1[p] = y1; gx2[p] = x2; gy2[p] = y2;
        gar[p] = (x2 - x1 + 1.0) * (y2 - y1 + 1.0);
        if (!BITS) alive[p] = 1;
        gob[p] = b[0]; gob[R + p] = b[1]; gob[2 * (size_t)R + p] = b[2]; gob[3 * (size_t)R + p] = b[3];
        gcls[p] = a.classes[beg + r];
        if (a.box_mode == PE_BOX_VAVG) ginv[p] = 1.0 / a.vars[beg + r];
        if (POOL) {
            const int src = checked_source(a.row_source[beg + r], a.num_detectors);
            gw[p] = src >= 0 ? a.pool_weights[src] : __builtin_nan("");
        }
        if (PRES) gsrc[p] = checked_source(a.row_source[beg + r], a.num_detectors);
        if (LOGP) {
            const double* lp = a.probs + (size_t)(beg + r) * (K + 1);
            for (int j = 0; j <= K; ++j) glog[(size_t)j * R + p] = lp[j];
        } else if (a.score_mode == PE_SCORE_PROBEN) {
            const double* pr = a.probs + (size_t)(beg + r) * K;
            double sum = 0.0;
            for (int j = 0; j < K; ++j) {
                const double pj = pr[j];
                sum += pj;
                glog[(size_t)j * R + p] = log(pj);
            }
            glog[(size_t)K * R + p] = log(1.0 - sum);
        } else if (a.score_mode == PE_SCORE_PROBEN_BINARY) {
            const double s = gsc[p];
            glog[p] = log(s);
            glog[(size_t)R + p] = log(1.0 - s);
        }
    }
    __syncthreads();

    // ---- 3. greedy clustering: only the membership is recorded ----
    if (BITS) {
        // (a) the pair tests: one (row, 64 candidates) item per wave step
        const int Wn = (n + 63) >> 6;
        for (int item = wave; item < n * Wn; item += kFuseThreads / 64) {
            const int p = item / Wn, c = item - p * Wn;
            unsigned long long m = 0, kl = 0;
            if (c >= (p >> 6)) {
                const int q = c * 64 + lane;
                PairTest t{false, false};
                if (q > p && q < n) t = pair_test(geometry(p), geometry(q), a.thr);
                m = __ballot(t.match);
                kl = __ballot(t.kill);
            }
            if (lane == 0) { mbits[(size_t)p * W + c] = m; kbits[(size_t)p * W + c] = kl; }
        }
        __syncthreads();
        // (b) the walk
        if (wave == 0) {
            unsigned long long live = 0;       // lane w: rows 64w .. 64w + 63
            if (lane < Wn) live = (n - lane * 64 >= 64) ? ~0ull : ((1ull << (n - lane * 64)) - 1ull);
            int ncl = 0, cursor = 0;
            for (int p0 = 0; p0 < n; p0 += 4) {
                unsigned long long mrow[4], krow[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const bool ok = p0 + u < n && lane < Wn;
                    mrow[u] = ok ? mbits[(size_t)(p0 + u) * W + lane] : 0ull;
                    krow[u] = ok ? kbits[(size_t)(p0 + u) * W + lane] : 0ull;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int p = p0 + u;
                    if (p >= n) break;
                    if (!((readlane64(live, p >> 6) >> (p & 63)) & 1ull)) continue;   // wave-uniform
                    const unsigned long long mem = mrow[u] & live;
                    live &= ~krow[u];
                    int cnt = 0;
                    for (int w = 0; w < Wn; ++w) cnt += __popcll(readlane64(mem, w));
                    if (lane < Wn) mbits[(size_t)p * W + lane] = mem;       // the line now holds the cluster's members
                    if (lane == 0) { cl_piv[ncl] = (unsigned short)p; cl_beg[ncl] = (unsigned short)cursor; cl_cnt[ncl] = (unsigned short)cnt; }
                    cursor += cnt;
                    ++ncl;
                }
            }
            if (lane == 0) ncl_s = ncl;
        }
    } else if (wave == 0) {
        // sequential in the pivot, 64 candidates per step, IoUs computed on the way
        int ncl = 0, cursor = 0;
        for (int pos = 0; pos < n; ++pos) {
            if (!alive[pos]) continue;  // wave-uniform (LDS broadcast)
            const RowGeometry pivot = geometry(pos);
            int cnt = 0;
            for (int base = pos + 1; base < n; base += 64) {
                const int q = base + lane;
                bool match = false;
                if (q < n && alive[q]) {
                    const PairTest t = pair_test(pivot, geometry(q), a.thr);
                    match = t.match;
                    if (t.kill) alive[q] = 0;
                }
                const unsigned long long mask = __ballot(match);
                if (match) members[cursor + cnt + __popcll(mask & pe::lanemask_lt())] = (unsigned short)q;
                cnt += __popcll(mask);
            }
            if (lane == 0) { cl_piv[ncl] = (unsigned short)pos; cl_beg[ncl] = (unsigned short)cursor; cl_cnt[ncl] = (unsigned short)cnt; }
            cursor += cnt;
            ++ncl;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // alive[] is re-read by other lanes of this wave
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) ncl_s = ncl;
    }
    __syncthreads();
    const int ncl = ncl_s;
    int* rcl = reinterpret_cast<int*>(gx1);      // POOL + out_cluster: sorted position -> output row of its cluster (gx1 is dead now)
    double* gvar = gy1;                          // POST: sorted position -> the row's variance (gy1 is dead now)
    const bool want_cluster = (POOL || POST || PRES) && a.out_cluster;      // block-uniform
    if (want_cluster)
        for (int p = tid; p < n; p += kFuseThreads) rcl[p] = -1;
    if (POST)
        for (int p = tid; p < n; p += kFuseThreads) gvar[p] = a.vars[beg + ord[p]];
    if (want_cluster || POST) __syncthreads();
    // ---- 4. fusion: one lane per cluster (cluster = matches in sorted order + the pivot LAST), output row = cluster index.
    // The per-cluster arithmetic is the sequence the reference runs per pivot (sums over the members in cluster order, the
    // normaliser summed over the columns in column order, first-maximum / first-NaN rules); it used to sit inside the pivot loop
    // with 4 (+4) of the 64 lanes working and every latency of its dependent chains exposed ~100 times per image. ----
    for (int k = tid; k < ncl; k += kFuseThreads) {
        const int pos = cl_piv[k], cnt = cl_cnt[k];
        unsigned short* mem = members + cl_beg[k];
        if (BITS) {     // the member bits in ascending (= sorted) order; this thread's own stretch of the list
            int i = 0;
            for (int w = pos >> 6; w < ((n + 63) >> 6); ++w)
                for (unsigned long long bits = mbits[(size_t)pos * W + w]; bits; bits &= bits - 1ull) mem[i++] = (unsigned short)(w * 64 + __builtin_ctzll(bits));
        }
        const int m = cnt + 1;
        const int piv_row = ord[pos];
        if (want_cluster) {
            for (int t = 0; t < cnt; ++t) rcl[mem[t]] = k;
            rcl[pos] = k;
        }
        auto at = [&](int t) { return t < cnt ? (int)mem[t] : pos; };
        auto coord = [&](int c4, int p) { return gob[(size_t)c4 * R + p]; };
        double out_score = gsc[pos];
        double out_class = (double)gcls[pos];
        double out_coord[4];
        const size_t o = (size_t)beg + k;
        double out_var = POST ? gvar[pos] : 0.0;
        int pat = 0;                                 // PRES: the cluster's presence pattern, its table row (NULL: a member's source is bad)
        const double* prow = nullptr;
        if (PRES) {
            bool ok = true;
            for (int t = 0; t < m; ++t) {
                const int src = gsrc[at(t)];
                ok = ok && src >= 0;
                pat |= src >= 0 ? 1 << src : 0;
            }
            if (ok) prow = a.presence + (size_t)pat * L;
            if (a.out_pattern) a.out_pattern[o] = pat;
        }
        if (cnt == 0) {
            for (int c4 = 0; c4 < 4; ++c4) out_coord[c4] = coord(c4, pos);
            if (PRES) {          // a cluster of one is fused: a_j = lp_j + presence[P][j]
                logp_rule([&](int j) { return glog[(size_t)j * R + pos] + (prow ? prow[j] : __builtin_nan("")); }, L,
                          POST ? a.out_log_posterior + o * L : nullptr, out_score, out_class);
            } else if (POST)
                for (int j = 0; j < L; ++j) a.out_log_posterior[o * L + j] = glog[(size_t)j * R + pos];
        } else {
            // ---------- score fusion ----------
            if (LOGP) {
                // a_j = sum over the members (cluster order) of log p_j, less (m - 1) log prior_j; s = softmax(a) with the maximum
                // subtracted first, so the largest term is exp(0) and nothing under- or overflows before the division.  np.max /
                // np.argmax over the K+1 entries INCLUDING background, NaN wins, first index - logp_rule() above.
                // POOL: a_j = sum of w log p_j, less (W - 1) log prior_j, W = the members' weights summed in the same order
                double wsum = 0.0;
                if (POOL) for (int t = 0; t < m; ++t) wsum += gw[at(t)];
                auto column = [&](int j) {
                    double acc = 0.0;
                    const double* col = glog + (size_t)j * R;
                    for (int t = 0; t < m; ++t) acc += POOL ? gw[at(t)] * col[at(t)] : col[at(t)];
                    if (a.log_prior) acc -= (POOL ? wsum - 1.0 : (double)(m - 1)) * a.log_prior[j];
                    if (PRES) acc += prow ? prow[j] : __builtin_nan("");      // last: the presence evidence of the cluster's pattern
                    return acc;
                };
                if (!PRES) {
                    logp_rule(column, L, POST ? a.out_log_posterior + o * L : nullptr, out_score, out_class);
                } else {        // the presence kernels' copy of the rule: see logp_rule
                    double top = column(0);
                    for (int j = 1; j < L; ++j) {
                        const double v = column(j);
                        top = (v > top || v != v) ? v : top;          // NaN wins, like np.max
                    }
                    double tot = 0.0;
                    for (int j = 0; j < L; ++j) tot += exp(column(j) - top);
                    double best = exp(column(0) - top) / tot;
                    int bi = 0;
                    bool bnan = best != best;
                    for (int j = 1; j < L; ++j) {
                        const double v = exp(column(j) - top) / tot;
                        if (!bnan && (v != v || v > best)) { best = v; bi = j; bnan = v != v; }
                    }
                    out_score = best;
                    out_class = (double)bi;
                    if (POST) {
                        const double ltot = log(tot);
                        for (int j = 0; j < L; ++j) a.out_log_posterior[o * L + j] = (column(j) - top) - ltot;
                    }
                }
            } else if (L > 0) {
                auto column = [&](int j) {       // exp of the cluster's summed log-probability of column j
                    double acc = 0.0;
                    const double* col = glog + (size_t)j * R;
                    for (int t = 0; t < m; ++t) acc += col[at(t)];
                    return exp(acc);
                };
                double tot = 0.0;
                for (int j = 0; j < L; ++j) tot += column(j);
                if (a.score_mode == PE_SCORE_PROBEN) {
                    // np.max / np.argmax over the K+1 entries INCLUDING background
                    const FirstMax best = first_max([&](int j) { return column(j) / tot; }, L);
                    out_score = best.value;
                    out_class = (double)best.index;
                } else {
                    out_score = column(0) / tot;
                }
            } else if (a.score_mode == PE_SCORE_AVG) {
                double acc = 0.0;
                for (int t = 0; t < m; ++t) acc += gsc[at(t)];
                out_score = acc / (double)m;
            } else {  // PE_SCORE_MAX: max over the whole [m,K] probability matrix
                double best = -INFINITY;
                bool bnan = false;
                for (int t = 0; t < m; ++t) {
                    const int r = ord[at(t)];
                    for (int j = 0; j < K; ++j) {
                        const double v = a.probs[(size_t)(beg + r) * K + j];
                        if (v != v) bnan = true;
                        best = v > best ? v : best;
                    }
                }
                out_score = bnan ? NAN : best;
            }
            // ---------- box fusion ----------
            if (a.box_mode == PE_BOX_VAVG || a.box_mode == PE_BOX_SAVG) {
                auto weight = [&](int p) { return (a.box_mode == PE_BOX_VAVG) ? ginv[p] : gsc[p]; };
                double wsum = 0.0;
                for (int t = 0; t < m; ++t) wsum += weight(at(t));
                for (int c4 = 0; c4 < 4; ++c4) {
                    double acc = 0.0;
                    for (int t = 0; t < m; ++t) {
                        const int p = at(t);
                        acc += coord(c4, p) * (weight(p) / wsum);
                    }
                    out_coord[c4] = acc;
                }
                if (POST) {
                    if (a.box_mode == PE_BOX_VAVG) {
                        out_var = 1.0 / wsum;
                    } else {
                        out_var = 0.0;
                        for (int t = 0; t < m; ++t) {
                            const int p = at(t);
                            const double lam = weight(p) / wsum;
                            out_var += (lam * lam) * gvar[p];
                        }
                    }
                }
            } else if (a.box_mode == PE_BOX_AVG) {
                for (int c4 = 0; c4 < 4; ++c4) {
                    double acc = 0.0;
                    for (int t = 0; t < m; ++t) acc += coord(c4, at(t));
                    out_coord[c4] = acc / (double)m;
                }
                if (POST) {
                    const double lam = 1.0 / (double)m;
                    out_var = 0.0;
                    for (int t = 0; t < m; ++t) out_var += (lam * lam) * gvar[at(t)];
                }
            } else {  // argmax: box of the first maximal score in cluster order
                const int bp = at(first_max([&](int t) { return gsc[at(t)]; }, m).index);
                for (int c4 = 0; c4 < 4; ++c4) out_coord[c4] = coord(c4, bp);
                if (POST) out_var = gvar[bp];
            }
        }
        if (POST) {
            a.out_vars[o] = out_var;
            a.out_members[o] = m;
        }
        a.out_scores[o] = (float)out_score;
        a.out_classes[o] = (float)out_class;
        a.out_keep[o] = piv_row;
        for (int c4 = 0; c4 < 4; ++c4) a.out_boxes[o * 4 + c4] = out_coord[c4];
    }
    if (want_cluster) {
        __syncthreads();
        for (int p = tid; p < n; p += kFuseThreads) a.out_cluster[beg + ord[p]] = rcl[p];
    }
    if (tid == 0) a.out_counts[img] = ncl;
}

// The 18 instantiations, stated once: the plain rule and "probEn-log" with each of its eight option sets, each in the sequential [0] and
// the bit-matrix [1] form.  fuse_impl's index: logp ? 1 + pool + 2 post + 4 pres : 0.
using FuseKernel = void (*)(ProbenArgs);
template <bool LOGP, bool POOL, bool POST, bool PRES>
constexpr FuseKernel kFuseForms[2] = {proben_fuse_kernel<false, LOGP, POOL, POST, PRES>, proben_fuse_kernel<true, LOGP, POOL, POST, PRES>};
constexpr const FuseKernel* kFuseKernels[9] = {
    kFuseForms<false, false, false, false>,
    kFuseForms<true, false, false, false>, kFuseForms<true, true, false, false>, kFuseForms<true, false, true, false>, kFuseForms<true, true, true, false>,
    kFuseForms<true, false, false, true>, kFuseForms<true, true, false, true>, kFuseForms<true, false, true, true>, kFuseForms<true, true, true, true>};

// pe_proben_fuse_batch / pe_proben_fuse_batch_logp: the argument checks, LDS sizing, clustering form, launch.  logp: a.probs holds the
// K+1 log-posteriors (required), a.score_mode is PE_SCORE_PROBEN_LOGP and is not the caller's to choose.  pool (implies logp):
// pe_proben_fuse_batch_pooled, a.row_source / a.pool_weights required, 8 more bytes of LDS per row for the staged weight.
// post (implies logp, pool = the caller gave row_source): pe_proben_fuse_batch_posterior, the three more outputs required.
// pres (implies logp; pool = the caller gave pool_weights, post = the caller gave the three posterior outputs): pe_proben_fuse_batch_presence,
// a.row_source / a.presence required, num_detectors in [1, PE_PRESENCE_MAX_DETECTORS], 4 more bytes of LDS per row for the staged source.
int fuse_impl(const char* what, bool logp, bool pool, bool post, bool pres, ProbenArgs a, int32_t max_rows_per_image, void* stream) {
    const int32_t num_images = a.B, num_classes = a.K;
    PE_CHECK_ARG(num_images >= 0, "%s: num_images < 0", what);
    if (num_images == 0) return PE_OK;
    PE_CHECK_ARG(a.boxes && a.scores && (a.probs || !logp) && a.vars && a.classes && a.offsets, "%s: null input pointer", what);
    PE_CHECK_ARG(a.out_boxes && a.out_scores && a.out_classes && a.out_keep && a.out_counts, "%s: null output pointer", what);
    PE_CHECK_ARG(!pool || (a.row_source && a.pool_weights), "%s: null input pointer (row_source / pool_weights)", what);
    PE_CHECK_ARG(!pres || (a.row_source && a.presence), "%s: null input pointer (row_source / presence)", what);
    PE_CHECK_ARG(!pres || (!a.out_log_posterior == !a.out_vars && !a.out_vars == !a.out_members),
                 "%s: out_log_posterior / out_vars / out_members go together (all NULL = a score-only run)", what);
    PE_CHECK_ARG(!pres || (a.num_detectors >= 1 && a.num_detectors <= PE_PRESENCE_MAX_DETECTORS), "%s: num_detectors %d not in [1,%d]", what,
                 a.num_detectors, PE_PRESENCE_MAX_DETECTORS);
    PE_CHECK_ARG(!post || pres || (!a.row_source == !a.pool_weights), "%s: row_source and pool_weights go together (both NULL = the unpooled rule)", what);
    PE_CHECK_ARG(!post || (a.out_log_posterior && a.out_vars && a.out_members),
                 "%s: null output pointer (out_log_posterior / out_vars / out_members)", what);
    PE_CHECK_ARG(!pool || (a.num_detectors >= 1 && a.num_detectors <= PE_POOL_MAX_DETECTORS), "%s: num_detectors %d not in [1,%d]", what,
                 a.num_detectors, PE_POOL_MAX_DETECTORS);
    PE_CHECK_ARG(logp || (a.score_mode >= 0 && a.score_mode <= 3), "%s: bad score_mode %d", what, a.score_mode);
    PE_CHECK_ARG(a.box_mode >= 0 && a.box_mode <= 3, "%s: bad box_mode %d", what, a.box_mode);
    // K <= 62: a wavefront keeps a cluster's per-class log-odds in lanes (K + background in 64 lanes).  Enough for every fusion the
    // reference can run: prediction files of different class counts cannot be fused there either (prepare_data concatenates the
    // `probs` arrays, demo_probEn.py:79-90), and the 80-class rgb_only file is evaluated on its own.
    PE_CHECK_ARG(num_classes >= 1 && num_classes <= 62, "%s: num_classes %d not in [1,62]", what, num_classes);
    PE_CHECK_ARG(a.probs || (a.score_mode != PE_SCORE_PROBEN && a.score_mode != PE_SCORE_MAX), "%s: probs required for this score_mode", what);
    PE_CHECK_ARG(max_rows_per_image >= 1 && max_rows_per_image <= 2048, "%s: max_rows_per_image %d not in [1,2048]", what,
                 max_rows_per_image);
    const int R = (max_rows_per_image + 1) & ~1;  // keep the int/short/byte carves 8-byte aligned
    const int L = (logp || a.score_mode == PE_SCORE_PROBEN) ? num_classes + 1 : (a.score_mode == PE_SCORE_PROBEN_BINARY ? 2 : 0);
    // a whole image's rows live in LDS (FuseLayout: 8 (11 + L) + 17 bytes per row, 8 more for the pooled form's weight, 4 more for the
    // presence form's detector index); the bit-matrix form where its two matrices fit beside them, else the sequential form.  Capacity
    // at K = 3: 1 192 rows per image ("probEn", "probEn-log"; 1 126 pooled, 1 158 with presence, 1 096 with both), 1 349
    // ("probEn_binary"), 1 555 ("avg", "max") - a detector contributes at most 100.  The bit-matrix form reaches 576 rows there (556 with pool weights
    // and presence).
    const size_t lds_seq = fuse_lds_bytes(R, L, pool, pres, false), lds_bits = fuse_lds_bytes(R, L, pool, pres, true);
    const bool bits = lds_bits + kFuseLdsStatic <= kFuseLdsLimit;
    const size_t lds = bits ? lds_bits : lds_seq;
    if (lds + kFuseLdsStatic > kFuseLdsLimit) {
        pe::set_error("%s: %zu bytes of LDS needed (> 160 KiB): max_rows_per_image %d is above the per-image capacity of %zu rows "
                      "for this score mode / class count", what, lds + kFuseLdsStatic, max_rows_per_image,
                      (kFuseLdsLimit - kFuseLdsStatic - fuse_lds_bytes(0, L, pool, pres, false)) / fuse_row_bytes(L, pool, pres));
        return PE_ERR_UNSUPPORTED;
    }
    a.max_rows = R;
    const FuseKernel kernel = kFuseKernels[logp ? 1 + (pool ? 1 : 0) + (post ? 2 : 0) + (pres ? 4 : 0) : 0][bits ? 1 : 0];
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            pe::set_error("%s: cannot raise dynamic LDS to %zu: %s", what, lds, hipGetErrorString(e));
            return PE_ERR_HIP;
        }
    }
    hipLaunchKernelGGL(kernel, dim3(num_images), dim3(kFuseThreads), lds, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}

}  // namespace

extern "C" int pe_proben_fuse_batch(const double* boxes, const double* scores, const double* probs,
                                    const double* variances, const int32_t* classes, const int32_t* offsets,
                                    const int32_t* row_counts, const int32_t* passthrough, int32_t num_images, int32_t num_classes, int32_t max_rows_per_image,
                                    int32_t score_mode, int32_t box_mode, double iou_thresh, double frame_w,
                                    double frame_h, double* out_boxes, float* out_scores, float* out_classes,
                                    int32_t* out_keep, int32_t* out_counts, void* stream) {
    const ProbenArgs a{boxes, scores, probs, variances, classes, offsets, row_counts, passthrough, num_images, num_classes, 0,
                       score_mode, box_mode, iou_thresh, frame_w, frame_h, out_boxes, out_scores, out_classes, out_keep, out_counts};
    return fuse_impl("pe_proben_fuse_batch", false, false, false, false, a, max_rows_per_image, stream);
}

extern "C" int pe_proben_fuse_batch_logp(const double* boxes, const double* scores, const double* log_probs,
                                         const double* variances, const int32_t* classes, const int32_t* offsets,
                                         const int32_t* row_counts, const int32_t* passthrough, int32_t num_images,
                                         int32_t num_classes, int32_t max_rows_per_image, int32_t box_mode, double iou_thresh,
                                         double frame_w, double frame_h, const double* log_prior, double* out_boxes,
                                         float* out_scores, float* out_classes, int32_t* out_keep, int32_t* out_counts, void* stream) {
    ProbenArgs a{boxes, scores, log_probs, variances, classes, offsets, row_counts, passthrough, num_images, num_classes, 0,
                 PE_SCORE_PROBEN_LOGP, box_mode, iou_thresh, frame_w, frame_h, out_boxes, out_scores, out_classes, out_keep, out_counts};
    a.log_prior = log_prior;
    return fuse_impl("pe_proben_fuse_batch_logp", true, false, false, false, a, max_rows_per_image, stream);
}

extern "C" int pe_proben_fuse_batch_pooled(const double* boxes, const double* scores, const double* log_probs,
                                           const double* variances, const int32_t* classes, const int32_t* row_source,
                                           const int32_t* offsets, const int32_t* row_counts, const int32_t* passthrough,
                                           int32_t num_images, int32_t num_classes, int32_t max_rows_per_image, int32_t box_mode,
                                           double iou_thresh, double frame_w, double frame_h, const double* log_prior,
                                           const double* pool_weights, int32_t num_detectors, double* out_boxes, float* out_scores,
                                           float* out_classes, int32_t* out_keep, int32_t* out_counts, int32_t* out_cluster,
                                           void* stream) {
    ProbenArgs a{boxes, scores, log_probs, variances, classes, offsets, row_counts, passthrough, num_images, num_classes, 0,
                 PE_SCORE_PROBEN_LOGP, box_mode, iou_thresh, frame_w, frame_h, out_boxes, out_scores, out_classes, out_keep, out_counts};
    a.log_prior = log_prior; a.row_source = row_source; a.pool_weights = pool_weights; a.num_detectors = num_detectors; a.out_cluster = out_cluster;
    return fuse_impl("pe_proben_fuse_batch_pooled", true, true, false, false, a, max_rows_per_image, stream);
}

extern "C" int pe_proben_fuse_batch_posterior(const double* boxes, const double* scores, const double* log_probs,
                                              const double* variances, const int32_t* classes, const int32_t* row_source,
                                              const int32_t* offsets, const int32_t* row_counts, const int32_t* passthrough,
                                              int32_t num_images, int32_t num_classes, int32_t max_rows_per_image, int32_t box_mode,
                                              double iou_thresh, double frame_w, double frame_h, const double* log_prior,
                                              const double* pool_weights, int32_t num_detectors, double* out_boxes, float* out_scores,
                                              float* out_classes, int32_t* out_keep, int32_t* out_counts, int32_t* out_cluster,
                                              double* out_log_posterior, double* out_vars, int32_t* out_members, void* stream) {
    ProbenArgs a{boxes, scores, log_probs, variances, classes, offsets, row_counts, passthrough, num_images, num_classes, 0,
                 PE_SCORE_PROBEN_LOGP, box_mode, iou_thresh, frame_w, frame_h, out_boxes, out_scores, out_classes, out_keep, out_counts};
    a.log_prior = log_prior; a.row_source = row_source; a.pool_weights = pool_weights; a.num_detectors = num_detectors; a.out_cluster = out_cluster;
    a.out_log_posterior = out_log_posterior; a.out_vars = out_vars; a.out_members = out_members;
    return fuse_impl("pe_proben_fuse_batch_posterior", true, row_source != nullptr && pool_weights != nullptr, true, false, a, max_rows_per_image, stream);
}

extern "C" int pe_proben_fuse_batch_presence(const double* boxes, const double* scores, const double* log_probs,
                                             const double* variances, const int32_t* classes, const int32_t* row_source,
                                             const int32_t* offsets, const int32_t* row_counts, const int32_t* passthrough,
                                             int32_t num_images, int32_t num_classes, int32_t max_rows_per_image, int32_t box_mode,
                                             double iou_thresh, double frame_w, double frame_h, const double* log_prior,
                                             const double* pool_weights, const double* presence, int32_t num_detectors, double* out_boxes,
                                             float* out_scores, float* out_classes, int32_t* out_keep, int32_t* out_counts,
                                             int32_t* out_cluster, double* out_log_posterior, double* out_vars, int32_t* out_members,
                                             int32_t* out_pattern, void* stream) {
    ProbenArgs a{boxes, scores, log_probs, variances, classes, offsets, row_counts, passthrough, num_images, num_classes, 0,
                 PE_SCORE_PROBEN_LOGP, box_mode, iou_thresh, frame_w, frame_h, out_boxes, out_scores, out_classes, out_keep, out_counts};
    a.log_prior = log_prior; a.row_source = row_source; a.pool_weights = pool_weights; a.num_detectors = num_detectors; a.out_cluster = out_cluster;
    a.out_log_posterior = out_log_posterior; a.out_vars = out_vars; a.out_members = out_members;
    a.presence = presence; a.out_pattern = out_pattern;
    return fuse_impl("pe_proben_fuse_batch_presence", true, pool_weights != nullptr, out_log_posterior != nullptr, true, a, max_rows_per_image, stream);
}
