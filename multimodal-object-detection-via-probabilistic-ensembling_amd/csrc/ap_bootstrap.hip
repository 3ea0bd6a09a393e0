// Bootstrap replicates of COCO accumulate (gfx950): detectron2/pycocotools/cocoeval.py:315-421 under a resample of the images, from
// the matches pe_cocoeval_bbox_matches exports once (csrc/cocoeval.cpp).  DESIGN.md 27 states the rule and why it equals the
// evaluator on the dataset that holds image i mult[i] times, bit for bit; include/proben_hip.h states the layout.
//
// One workgroup per (replicate, cell), one wavefront per IoU threshold.  The workgroup loads the replicate's multiplicity row, the
// recall thresholds and a zeroed q[T][R] into LDS and adds up NP (int64, integers: exact in any order).  Each wavefront then
//   1. adds up its threshold's weighted tp and fp over the whole list (int32, a wave reduction), and
//   2. walks the list in 64-entry chunks FROM THE RIGHT.  Per chunk: an inclusive wave scan of the weighted tp / fp, turned into the
//      running counts by the carry (the totals of step 1 minus the chunks already walked); pr_j = TP_j / (FP_j + TP_j + eps) in
//      float64 - the evaluator's expression on the same integers; a suffix-max wave scan with the envelope carried in from the
//      right.  A lane whose entry raises the recall owns the thresholds in (rc_{j-1}, rc_j] - two binary searches of rec_thrs in
//      LDS with the evaluator's comparison `rc >= thr` - and writes its envelope value to them.  Entry 0 owns the thresholds <= rc_0.
//      The ranges of different lanes are disjoint: no two lanes write one q[r].
// psum is q[0] + q[1] + ... added by one lane in that order.  Nothing depends on B, C or the grid: a replicate alone and the same
// replicate among others give the same bytes.  Built with -ffp-contract=off.
#include "common.h"

namespace {

constexpr double kEps = 2.220446049250313e-16;      // np.spacing(1)
constexpr int kMaxWaves = PE_AP_BOOTSTRAP_MAX_T;

struct ApArgs {
    const int64_t* list_off;
    const int32_t* list_img;
    const uint8_t* list_rank;
    const uint32_t* list_flags;
    long long stride;
    const int32_t* npig;
    const uint8_t* mult;
    int B, I, K, A, T;
    const double* rec_thrs;
    int R;
    const int32_t* cells;
    int C;
    double* psum;
    double* recall;
    int32_t* valid;
    double* precision;
};

__host__ __device__ inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
// LDS: rec_thrs [R] | q [T][R] | wave partials of NP [kMaxWaves] | mult row [I]
inline size_t lds_bytes(int I, int T, int R) { return align16((size_t)(R + T * R + kMaxWaves) * 8) + align16((size_t)I); }

// number of thresholds <= v (thr ascending): entry j owns [count_le(rc_{j-1}), count_le(rc_j)), the r with rc_{j-1} < thr[r] <= rc_j
__device__ __forceinline__ int count_le(const double* thr, int R, double v) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (thr[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int wave_scan_add(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

struct Entry { int img; int rank; uint32_t flags; };

__device__ __forceinline__ Entry load_entry(const ApArgs& a, long long off, const uint32_t* flags_row, int j, int n) {
    Entry e{0, 0x7fffffff, 0u};
    if (j >= 0 && j < n) {
        e.img = a.list_img[off + j];
        e.rank = a.list_rank[off + j];
        e.flags = flags_row[off + j];
    }
    return e;
}

// the entry's weight under this replicate and maxDet, split into its tp and fp parts at threshold t
__device__ __forceinline__ void weigh(const Entry& e, const uint8_t* mrow, int I, int max_det, int t, int* wt, int* wf) {
    const int w = (e.rank < max_det && (unsigned)e.img < (unsigned)I) ? (int)mrow[e.img] : 0;
    const bool matched = (e.flags >> t) & 1u, ignored = (e.flags >> (16 + t)) & 1u;
    *wt = (matched && !ignored) ? w : 0;
    *wf = (!matched && !ignored) ? w : 0;
}

__global__ __launch_bounds__(64 * kMaxWaves) void ap_bootstrap_kernel(ApArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = a.T, R = a.R, I = a.I;
    double* thr = reinterpret_cast<double*>(smem);
    double* q = thr + R;
    long long* np_part = reinterpret_cast<long long*>(q + T * R);
    uint8_t* mrow = reinterpret_cast<uint8_t*>(smem + align16((size_t)(R + T * R + kMaxWaves) * 8));
    const int tid = threadIdx.x, lane = tid & 63, t = tid >> 6, threads = blockDim.x;
    const int b = blockIdx.x / a.C, cell = blockIdx.x % a.C;
    const size_t out = (size_t)b * a.C + cell;

    const int k = a.cells[cell * 3], ar = a.cells[cell * 3 + 1], max_det = a.cells[cell * 3 + 2];
    bool ok = (unsigned)k < (unsigned)a.K && (unsigned)ar < (unsigned)a.A;
    long long off = 0, end = 0;
    if (ok) {
        off = a.list_off[k];
        end = a.list_off[k + 1];
        ok = off >= 0 && off <= end && end <= a.stride;
    }
    if (!ok) {                                  // workgroup-uniform
        if (tid == 0) a.valid[out] = -1;
        if (lane == 0) { a.psum[out * T + t] = 0.0; a.recall[out * T + t] = -1.0; }
        if (a.precision)
            for (int r = lane; r < R; r += 64) a.precision[(out * T + t) * R + r] = -1.0;
        return;
    }
    const int n = (int)(end - off);
    const uint32_t* flags_row = a.list_flags + (size_t)ar * a.stride;

    const uint8_t* mult = a.mult + (size_t)b * I;
    const int32_t* npig = a.npig + ((size_t)k * a.A + ar) * I;
    long long np = 0;
    for (int i = tid; i < I; i += threads) {
        const uint8_t m = mult[i];
        mrow[i] = m;
        np += (long long)m * npig[i];
    }
    for (int r = tid; r < R; r += threads) thr[r] = a.rec_thrs[r];
    for (int i = tid; i < T * R; i += threads) q[i] = 0.0;
    for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o);
    if (lane == 0) np_part[t] = np;
    __syncthreads();
    np = 0;
    for (int v = 0; v < T; ++v) np += np_part[v];
    if (np == 0) {                              // workgroup-uniform: the reference leaves such a cell at -1
        if (tid == 0) a.valid[out] = 0;
        if (lane == 0) { a.psum[out * T + t] = 0.0; a.recall[out * T + t] = -1.0; }
        if (a.precision)
            for (int r = lane; r < R; r += 64) a.precision[(out * T + t) * R + r] = -1.0;
        return;
    }
    const double npd = (double)np;

    // 1. this threshold's totals
    int tot_tp = 0, tot_fp = 0;
    for (int j = lane; j < n; j += 64) {
        int wt, wf;
        weigh(load_entry(a, off, flags_row, j, n), mrow, I, max_det, t, &wt, &wf);
        tot_tp += wt;
        tot_fp += wf;
    }
    for (int o = 32; o > 0; o >>= 1) {
        tot_tp += __shfl_xor(tot_tp, o);
        tot_fp += __shfl_xor(tot_fp, o);
    }

    // 2. from the right; the next chunk's entry is loaded before this one is worked on
    int carry_tp = tot_tp, carry_fp = tot_fp;   // counts at the end of the current chunk
    double carry_env = -1.0;                    // below every precision: nothing to the right yet
    double* qt = q + t * R;
    const int chunks = (n + 63) >> 6;
    Entry next = load_entry(a, off, flags_row, (chunks - 1) * 64 + lane, n);
    for (int c = chunks - 1; c >= 0; --c) {
        const int j = c * 64 + lane;
        const Entry e = next;
        next = load_entry(a, off, flags_row, j - 64, n);
        const bool live = j < n;
        int wt, wf;
        weigh(e, mrow, I, max_det, t, &wt, &wf);                // an entry past the end has rank INT_MAX: weight 0
        const int s_tp = wave_scan_add(wt, lane), s_fp = wave_scan_add(wf, lane);
        carry_tp -= __shfl(s_tp, 63);
        carry_fp -= __shfl(s_fp, 63);
        const int tp = carry_tp + s_tp, fp = carry_fp + s_fp;
        const double pr = (double)tp / ((double)fp + (double)tp + kEps);
        double env = live ? pr : -1.0;
        for (int o = 1; o < 64; o <<= 1) {
            const double v = __shfl_down(env, o);
            if (lane + o < 64 && v > env) env = v;
        }
        if (carry_env > env) env = carry_env;
        carry_env = __shfl(env, 0);
        if (live && (wt > 0 || j == 0)) {
            const int r0 = j == 0 ? 0 : count_le(thr, R, (double)(tp - wt) / npd);
            const int r1 = count_le(thr, R, (double)tp / npd);
            for (int r = r0; r < r1; ++r) qt[r] = env;
        }
    }
    __syncthreads();                            // every wavefront walks the same list: the trip counts are equal
    if (tid == 0) a.valid[out] = 1;
    if (lane == 0) {
        double s = 0.0;
        for (int r = 0; r < R; ++r) s += qt[r];
        a.psum[out * T + t] = s;
        a.recall[out * T + t] = n ? (double)tot_tp / npd : 0.0;
    }
    if (a.precision)
        for (int r = lane; r < R; r += 64) a.precision[(out * T + t) * R + r] = qt[r];
}

}  // namespace

extern "C" int pe_ap_bootstrap(const int64_t* list_off, const int32_t* list_img, const uint8_t* list_rank, const uint32_t* list_flags,
                               int64_t list_stride, const int32_t* npig, const uint8_t* mult, int32_t B, int32_t I, int32_t K, int32_t A,
                               int32_t T, const double* rec_thrs, int32_t R, const int32_t* cells, int32_t C, double* psum,
                               double* recall, int32_t* valid, double* precision, void* stream) {
    const char* what = "pe_ap_bootstrap";
    PE_CHECK_ARG(B >= 0 && C >= 0 && I >= 1 && K >= 1 && A >= 1 && T >= 1 && R >= 1 && list_stride >= 0,
                 "%s: bad sizes (B %d, C %d, I %d, K %d, A %d, T %d, R %d, list_stride %lld)", what, B, C, I, K, A, T, R,
                 (long long)list_stride);
    if (T > PE_AP_BOOTSTRAP_MAX_T || R > PE_AP_BOOTSTRAP_MAX_R || I > PE_AP_BOOTSTRAP_MAX_IMAGES ||
        list_stride > (int64_t)(INT32_MAX / 255) || (int64_t)B * C > INT32_MAX) {
        pe::set_error("%s: T %d > %d, R %d > %d, I %d > %d, list_stride %lld > %d (int32 counts of u8 multiplicities) or B * C > 2^31 - 1",
                      what, T, PE_AP_BOOTSTRAP_MAX_T, R, PE_AP_BOOTSTRAP_MAX_R, I, PE_AP_BOOTSTRAP_MAX_IMAGES, (long long)list_stride,
                      INT32_MAX / 255);
        return PE_ERR_UNSUPPORTED;
    }
    if (B == 0 || C == 0) return PE_OK;
    PE_CHECK_ARG(list_off && npig && mult && rec_thrs && cells && psum && recall && valid,
                 "%s: null pointer (list_off / npig / mult / rec_thrs / cells / psum / recall / valid)", what);
    PE_CHECK_ARG(list_stride == 0 || (list_img && list_rank && list_flags), "%s: null pointer (list_img / list_rank / list_flags)", what);
    const ApArgs args{list_off, list_img, list_rank, list_flags, (long long)list_stride, npig, mult, B, I, K, A, T, rec_thrs, R, cells, C,
                      psum, recall, valid, precision};
    hipLaunchKernelGGL(ap_bootstrap_kernel, dim3((unsigned)((int64_t)B * C)), dim3(64 * T), lds_bytes(I, T, R), (hipStream_t)stream, args);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}
