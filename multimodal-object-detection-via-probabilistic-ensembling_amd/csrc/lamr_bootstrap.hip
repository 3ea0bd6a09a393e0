// Bootstrap replicates of the KAIST log-average miss rate (gfx950): the accumulate of evalKAIST/evaluation_script.py - the evaluator
// behind demo/KAIST/demo_LAMR_KAIST.py:85,145 - under a resample of the images, from the per-image matches that
// lamr_bootstrap.export_lamr_matches exports once.  DESIGN.md 28 states the rule and why it equals the evaluator on the dataset that
// holds image i mult[i] times, bit for bit; include/proben_hip.h states the layout.
//
// One workgroup per replicate, one wavefront per cell (an image-index range [lo, hi): all / day / night are three cells over ONE
// list).  The workgroup stages the replicate's multiplicity row in LDS; after the one barrier the wavefronts are on their own.  A
// wavefront adds up N and NP over its range (int64), then walks the list left to right in 64-entry chunks: an exclusive int32 wave
// scan of the weighted false positives with the carry of the chunks before gives F_j; x = (double)F_j / (double)N is the evaluator's
// own division, `x <= thr[r]` its own comparison, and a lane whose entry is a weighted true positive adds its weight to the
// accumulators of the references it lies below.  The first weighted entry of the list decides the "no operating point below the
// reference reads the LAST one" rule: FPPI does not fall along the list, so no point lies below a reference exactly when the first
// one does not.  Every output is an integer, the lane accumulators are reduced once at the end, and nothing depends on B, on the
// other cells of the launch or on the run.  Built with -ffp-contract=off.
#include "common.h"

namespace {

constexpr int kMaxCells = PE_LAMR_BOOTSTRAP_MAX_CELLS;
constexpr int kMaxR = PE_LAMR_BOOTSTRAP_MAX_R;

struct LamrArgs {
    const int32_t* list_img;
    const uint8_t* list_flags;
    int n;
    const int32_t* npig;
    const uint8_t* mult;
    int B, I;
    const double* thr;
    int R;
    const int32_t* cells;
    int C;
    long long* tp_at;
    long long* totals;
    int32_t* valid;
};

__device__ __forceinline__ int wave_scan_add(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(64 * kMaxCells) void lamr_bootstrap_kernel(LamrArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mrow[];
    const int tid = threadIdx.x, lane = tid & 63, cell = tid >> 6, I = a.I, R = a.R, n = a.n;
    const int b = blockIdx.x;
    const uint8_t* mult = a.mult + (size_t)b * I;
    for (int i = tid; i < I; i += blockDim.x) mrow[i] = mult[i];
    __syncthreads();                            // the only barrier: from here on every wavefront works alone

    const size_t out = (size_t)b * a.C + cell;
    const int lo = a.cells[cell * 2], hi = a.cells[cell * 2 + 1];
    if (lo < 0 || hi > I || lo > hi) {          // wavefront-uniform
        if (lane == 0) a.valid[out] = -1;
        if (lane < 4) a.totals[out * 4 + lane] = 0;
        if (lane < R) a.tp_at[out * R + lane] = 0;
        return;
    }
    long long N = 0, NP = 0;
    for (int i = lo + lane; i < hi; i += 64) {
        const long long m = mrow[i];
        N += m;
        NP += m * a.npig[i];
    }
    N = wave_sum(N);
    NP = wave_sum(NP);
    const double Nd = (double)N;

    double thr[kMaxR];
#pragma unroll
    for (int r = 0; r < kMaxR; ++r) thr[r] = r < R ? a.thr[r] : 0.0;
    int acc[kMaxR];
#pragma unroll
    for (int r = 0; r < kMaxR; ++r) acc[r] = 0;

    int carry = 0, tot_tp = 0;                  // weighted fps of the chunks walked (wave-uniform); this lane's weighted tps
    int first = -1;                             // wave-uniform: the fp count at the list's first weighted copy (1 = an fp, 0 = a tp)
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        int w = 0;
        bool matched = false;
        if (j < n) {
            const int img = a.list_img[j];
            const unsigned f = a.list_flags[j];
            matched = f & 1u;
            if (img >= lo && img < hi && !(f & 2u)) w = mrow[img];      // lo >= 0 and hi <= I: an index outside [0, I) weighs 0
        }
        const int wt = matched ? w : 0, wf = matched ? 0 : w;
        const int incl = wave_scan_add(wf, lane);
        const int F = carry + incl - wf;        // exclusive
        carry += __shfl(incl, 63);
        tot_tp += wt;
        if (first < 0) {
            const unsigned long long live = __ballot(w > 0);
            if (live) first = (int)((__ballot(w > 0 && !matched) >> (__ffsll((long long)live) - 1)) & 1ull);
        }
        const double x = (double)F / Nd;
#pragma unroll
        for (int r = 0; r < kMaxR; ++r)
            if (r < R) acc[r] += x <= thr[r] ? wt : 0;
    }
    const long long TP = wave_sum(tot_tp), FP = carry;
    const double x0 = (double)first / Nd;       // read only where TP + FP > 0: then a weighted entry was seen
    const bool defined = NP != 0;
#pragma unroll
    for (int r = 0; r < kMaxR; ++r) {
        if (r < R) {
            long long v = wave_sum(acc[r]);
            if (TP + FP > 0 && !(x0 <= thr[r])) v = TP;     // searchsorted(...) - 1 == -1 reads the last operating point
            if (lane == 0) a.tp_at[out * R + r] = defined ? v : 0;
        }
    }
    if (lane == 0) {
        a.totals[out * 4 + 0] = N;
        a.totals[out * 4 + 1] = NP;
        a.totals[out * 4 + 2] = TP;
        a.totals[out * 4 + 3] = FP;
        a.valid[out] = defined ? 1 : 0;
    }
}

}  // namespace

extern "C" int pe_lamr_bootstrap(const int32_t* list_img, const uint8_t* list_flags, int64_t n_list, const int32_t* npig,
                                 const uint8_t* mult, int32_t B, int32_t I, const double* fppi_thrs, int32_t R, const int32_t* cells,
                                 int32_t C, int64_t* tp_at, int64_t* totals, int32_t* valid, void* stream) {
    const char* what = "pe_lamr_bootstrap";
    PE_CHECK_ARG(B >= 0 && C >= 0 && I >= 1 && R >= 1 && n_list >= 0, "%s: bad sizes (B %d, C %d, I %d, R %d, n_list %lld)", what, B, C, I, R,
                 (long long)n_list);
    if (C > PE_LAMR_BOOTSTRAP_MAX_CELLS || R > PE_LAMR_BOOTSTRAP_MAX_R || I > PE_AP_BOOTSTRAP_MAX_IMAGES ||
        n_list > (int64_t)(INT32_MAX / 255) || (int64_t)B * C > INT32_MAX) {
        pe::set_error("%s: C %d > %d, R %d > %d, I %d > %d, n_list %lld > %d (int32 counts of u8 multiplicities) or B * C > 2^31 - 1", what, C,
                      PE_LAMR_BOOTSTRAP_MAX_CELLS, R, PE_LAMR_BOOTSTRAP_MAX_R, I, PE_AP_BOOTSTRAP_MAX_IMAGES, (long long)n_list,
                      INT32_MAX / 255);
        return PE_ERR_UNSUPPORTED;
    }
    if (B == 0 || C == 0) return PE_OK;
    PE_CHECK_ARG(npig && mult && fppi_thrs && cells && tp_at && totals && valid,
                 "%s: null pointer (npig / mult / fppi_thrs / cells / tp_at / totals / valid)", what);
    PE_CHECK_ARG(n_list == 0 || (list_img && list_flags), "%s: null pointer (list_img / list_flags)", what);
    const LamrArgs args{list_img, list_flags, (int)n_list, npig, mult, B, I, fppi_thrs, R, cells, C,
                        reinterpret_cast<long long*>(tp_at), reinterpret_cast<long long*>(totals), valid};
    hipLaunchKernelGGL(lamr_bootstrap_kernel, dim3((unsigned)B), dim3(64 * C), ((size_t)I + 15) & ~(size_t)15, (hipStream_t)stream, args);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}
