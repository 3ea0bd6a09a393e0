// Weighted boxes fusion (Solovyev, Wang, Gabruseva: "Weighted boxes fusion: Ensembling boxes from different object detection models",
// Image and Vision Computing 107, 2021) for gfx950: ONE WORKGROUP PER IMAGE, ONE WAVEFRONT PER CLASS, whole per-image state in LDS.
//
// Not in the reference: its weighted_box_fusion() (demo/FLIR/demo_probEn.py:73-77) is the score-weighted box average this project
// calls "s-avg", over ProbEn's clusters.  This is the published method, the late-fusion baseline ProbEn is compared against.
// float64 throughout, compiled with -ffp-contract=off: every product, sum and quotient below rounds on its own, in the order written.
//
// The rule, per image, for rows (box, score, class, source) in detector order, detector weights u[D], IoU threshold thr, score floor skip:
//   U = u[0] + u[1] + ... (index order);  s = score * u[source].
//   A row is SKIPPED (counted in out_skipped, out_cluster -1, no further part) when source is outside [0, D), class is outside [0, K),
//   a coordinate or s is not finite, !(s > 0), or s < skip (s == skip is kept).
//   The kept rows are visited in the project's sort order (precedes() of proben.hip): s descending, ties by original index descending.
//   Classes are independent; per class the clusters are kept in creation order.  A cluster holds S, X[4], n and its fused box
//   F[k] = X[k] / S.  A visited row with box b is tested against EVERY cluster of its class, against the cluster's running fused box:
//     w = fmax(0, fmin(F.x2, b.x2) - fmax(F.x1, b.x1)), h likewise, inter = w * h,
//     iou = inter / ((F.x2 - F.x1) * (F.y2 - F.y1) + (b.x2 - b.x1) * (b.y2 - b.y1) - inter)       (continuous areas, no "+1", no class band)
//   best = the FIRST maximum of iou in creation order (a NaN never wins).  best > thr (strict): the row joins that cluster, else it opens
//   a new one (from zeros).  Joining: S += s; X[k] += s * b[k]; n += 1; F[k] = X[k] / S.
//   At the end conf = ((S / (double)n) * fmin((double)n, U)) / U, and the output rows are the clusters by conf descending, ties by class
//   ascending, then creation order ascending (a NaN conf - only weights the caller's contract excludes give one - sorts first).
//
// Why a kernel of its own: proben.hip's IoU tests use the rows' own geometry, never a fused box, so it ballots all pairs first and
// walks bit matrices afterwards.  Here the box a row is tested against moves with every row that joined before it: the walk over a
// class's rows is serial by definition, and the parallelism left is (a) the classes, a wavefront each, (b) the clusters a row is tested
// against, a lane each, (c) ranks, skip flags and the output, a thread per row / per cluster, (d) the images, a workgroup each.
//
// Kernel shape.  1024 threads = 16 wavefronts whatever K is: phases 1 and 3 are a thread per row / per cluster and use them all; in
// phase 2 a class belongs to wavefront (class mod 16) and wavefronts without a class wait at the barrier.
//   1  (workgroup) s and the skip flag a thread per row; ONE rank per kept row by counting, under the key (class ascending, then
//      precedes): the sorted rows of a class are contiguous, in visiting order, and the class's run [p0, p0 + cnt) of sorted positions is
//      also its region of cluster slots (a class has at most as many clusters as rows).  cnt is counted in the same loop.
//   2  (each wavefront alone, no workgroup barrier) for its classes' runs, row by row: lane l tests clusters l, l + 64, ... and keeps its
//      first maximum; the wave's maximum by a __shfl_xor butterfly, then the smallest cluster index among the lanes that hold it
//      (a second butterfly on the index): the first maximum in creation order.  The update is computed by every lane alike
//      (wave-uniform) and stored by lane 0.
//   3  (workgroup) conf a thread per cluster slot, its output row by counting, every output element written once by its owner.
// No atomics on floating-point values (one integer LDS counter for the skipped rows); an image's results depend on its own rows only.
#include "common.h"

namespace {

struct WbfArgs {
    const double *boxes, *scores;
    const int32_t *classes, *row_source, *offsets, *row_counts;
    int32_t B, K, max_rows;
    const double* det_weights;
    int32_t num_detectors;
    double thr, skip;
    double* out_boxes;
    float *out_scores, *out_classes;
    int32_t *out_counts, *out_cluster, *out_members, *out_skipped;
};

// The dynamic LDS of one image, stated once (the Cursor idiom of proben.hip's FuseLayout): every array in order, for max_rows R
// (even, so that every array starts 8-byte aligned).  K does not enter: no array is sized by the class count.
struct WbfPointers {
    template <typename T> using at = T*;
    unsigned char* next;
    template <typename T> __device__ T* take(size_t count) { T* p = reinterpret_cast<T*>(next); next = reinterpret_cast<unsigned char*>(p + count); return p; }
};
struct WbfBytes {
    template <typename T> using at = size_t;
    size_t next;
    template <typename T> size_t take(size_t count) { const size_t p = next; next += count * sizeof(T); return p; }
};
template <typename Cursor>
struct WbfLayout {
    template <typename T> using at = typename Cursor::template at<T>;
    at<double> rs;                          // [R] by ORIGINAL row: s = score * u[source]
    at<double> ss, sb;                      // [R], [4][R] by sorted position: s, the box
    at<double> cS, cX, cF, cA, conf;        // [R], [4][R], [4][R], [R], [R] by cluster slot: S, X, F, F's area, conf
    at<int> rc;                             // [R] by ORIGINAL row: class, -1 = skipped
    at<int> ord, scls, scnt, sslot;         // [R] by sorted position: original row, class, rows of the class, the row's cluster slot
    at<int> cn, crank;                      // [R] by cluster slot: n (0 = the slot holds no cluster), output row
    at<int> end;
    __host__ __device__ WbfLayout(Cursor c, int R) {
        const size_t r = (size_t)R;
        rs = c.template take<double>(r);
        ss = c.template take<double>(r); sb = c.template take<double>(4 * r);
        cS = c.template take<double>(r); cX = c.template take<double>(4 * r); cF = c.template take<double>(4 * r);
        cA = c.template take<double>(r); conf = c.template take<double>(r);
        rc = c.template take<int>(r);
        ord = c.template take<int>(r); scls = c.template take<int>(r); scnt = c.template take<int>(r); sslot = c.template take<int>(r);
        cn = c.template take<int>(r); crank = c.template take<int>(r);
        end = c.template take<int>(0);
    }
};
// 17 doubles + 7 ints = 164 bytes of LDS per row; 160 KiB less the static scratch hold 996 rows per image (PE_WBF_MAX_ROWS) at every K.
inline size_t wbf_lds_bytes(int R) { return WbfLayout<WbfBytes>(WbfBytes{0}, R).end + 16; }
inline size_t wbf_row_bytes() { return (wbf_lds_bytes(2) - wbf_lds_bytes(0)) / 2; }
constexpr size_t kWbfLdsLimit = 160 * 1024;
constexpr size_t kWbfLdsStatic = 256;           // the kernel's static __shared__ scratch (the weight table, two counters)
constexpr int kWbfThreads = 1024, kWbfWaves = kWbfThreads / 64;
// a launch's threads, gridDim.x * blockDim.x, must stay below 2^32
constexpr int32_t kWbfMaxImages = (int32_t)((1ull << 32) / kWbfThreads - 1);
static_assert(kWbfMaxImages == PE_WBF_MAX_IMAGES, "the header states the limit");
inline int wbf_capacity() { return (int)((kWbfLdsLimit - kWbfLdsStatic - wbf_lds_bytes(0)) / wbf_row_bytes()) & ~1; }

// The sort rule of proben.hip: NaN first, score descending, ties by ORIGINAL index descending.
__device__ __forceinline__ bool precedes(double sa, int ia, double sb, int ib) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return na;
    if (!na && sa != sb) return sa > sb;
    return ia > ib;
}

__device__ __forceinline__ bool finite(double x) { return x - x == 0.0; }

// everything one wavefront wrote to LDS is visible to its own lanes from here on
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kWbfThreads) void wbf_fuse_kernel(WbfArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double u_s[PE_WBF_MAX_DETECTORS];
    __shared__ int nskip_s;
    const int img = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int beg = a.offsets[img];
    const int n = a.row_counts ? a.row_counts[img] : a.offsets[img + 1] - beg;
    if (n > a.max_rows || n < 0) {
        if (tid == 0) { a.out_counts[img] = -1; a.out_skipped[img] = 0; }
        return;
    }
    const int R = a.max_rows, K = a.K, D = a.num_detectors;
    const WbfLayout<WbfPointers> lay(WbfPointers{smem}, R);
    double *rs = lay.rs, *ss = lay.ss, *sb = lay.sb, *cS = lay.cS, *cX = lay.cX, *cF = lay.cF, *cA = lay.cA, *conf = lay.conf;
    int *rc = lay.rc, *ord = lay.ord, *scls = lay.scls, *scnt = lay.scnt, *sslot = lay.sslot, *cn = lay.cn, *crank = lay.crank;

    if (tid < D) u_s[tid] = a.det_weights[tid];
    if (tid == 0) nskip_s = 0;
    __syncthreads();
    double U = 0.0;
    for (int d = 0; d < D; ++d) U += u_s[d];

    // ---- 1. s, skip flags, ranks ----
    for (int r = tid; r < n; r += kWbfThreads) {
        const size_t o = (size_t)beg + r;
        const int src = a.row_source[o], cls = a.classes[o];
        const double* b = a.boxes + o * 4;
        bool keep = src >= 0 && src < D && cls >= 0 && cls < K;
        const double s = a.scores[o] * (src >= 0 && src < D ? u_s[src] : 0.0);
        keep = keep && finite(b[0]) && finite(b[1]) && finite(b[2]) && finite(b[3]) && finite(s) && s > 0.0 && !(s < a.skip);
        rs[r] = s;
        rc[r] = keep ? cls : -1;
        cn[r] = 0;
        if (!keep) {
            a.out_cluster[o] = -1;
            atomicAdd(&nskip_s, 1);         // an integer count: the order of the additions cannot show
        }
    }
    __syncthreads();
    const int nk = n - nskip_s;             // kept rows = sorted positions [0, nk)
    for (int r = tid; r < n; r += kWbfThreads) {
        const int cls = rc[r];
        if (cls < 0) continue;
        const double s = rs[r];
        int rank = 0, same = 0;
#pragma unroll 4
        for (int q = 0; q < n; ++q) {
            const int cq = rc[q];
            if (cq < 0) continue;
            same += cq == cls ? 1 : 0;
            rank += (cq < cls || (cq == cls && precedes(rs[q], q, s, r))) ? 1 : 0;
        }
        const double* b = a.boxes + ((size_t)beg + r) * 4;
        ord[rank] = r;
        ss[rank] = s;
        scls[rank] = cls;
        scnt[rank] = same;
        for (int k = 0; k < 4; ++k) sb[(size_t)k * R + rank] = b[k];
    }
    __syncthreads();

    // ---- 2. the walk: a wavefront per class, a lane per cluster ----
    for (int p0 = 0; p0 < nk;) {
        const int cls = scls[p0], cnt = scnt[p0];       // wave-uniform (LDS broadcast)
        if (cls % kWbfWaves == wave) {
            int ncl = 0;                                // the class's clusters are slots p0 .. p0 + ncl - 1, in creation order
            for (int p = p0; p < p0 + cnt; ++p) {
                const double s = ss[p];
                const double b0 = sb[p], b1 = sb[(size_t)R + p], b2 = sb[2 * (size_t)R + p], b3 = sb[3 * (size_t)R + p];
                const double barea = (b2 - b0) * (b3 - b1);
                double best = -__builtin_huge_val();
                int bj = 0x7fffffff;
                for (int j = lane; j < ncl; j += 64) {
                    const int g = p0 + j;
                    const double f0 = cF[g], f1 = cF[(size_t)R + g], f2 = cF[2 * (size_t)R + g], f3 = cF[3 * (size_t)R + g];
                    const double w = fmax(0.0, fmin(f2, b2) - fmax(f0, b0));
                    const double h = fmax(0.0, fmin(f3, b3) - fmax(f1, b1));
                    const double inter = w * h;
                    const double iou = inter / (cA[g] + barea - inter);
                    if (iou > best) { best = iou; bj = j; }         // strict: the lane's first maximum; a NaN never wins
                }
                double top = best;
                for (int m = 32; m >= 1; m >>= 1) {
                    const double other = __shfl_xor(top, m, 64);
                    top = other > top ? other : top;
                }
                int first = (best == top) ? bj : 0x7fffffff;        // lanes that tested nothing hold 0x7fffffff
                for (int m = 32; m >= 1; m >>= 1) first = min(first, __shfl_xor(first, m, 64));
                const bool join = first != 0x7fffffff && top > a.thr;
                const int g = p0 + (join ? first : ncl);
                const double S = (join ? cS[g] : 0.0) + s;
                double X[4], F[4];
                X[0] = (join ? cX[g] : 0.0) + s * b0;
                X[1] = (join ? cX[(size_t)R + g] : 0.0) + s * b1;
                X[2] = (join ? cX[2 * (size_t)R + g] : 0.0) + s * b2;
                X[3] = (join ? cX[3 * (size_t)R + g] : 0.0) + s * b3;
                for (int k = 0; k < 4; ++k) F[k] = X[k] / S;
                const int members = (join ? cn[g] : 0) + 1;
                if (lane == 0) {
                    cS[g] = S;
                    for (int k = 0; k < 4; ++k) { cX[(size_t)k * R + g] = X[k]; cF[(size_t)k * R + g] = F[k]; }
                    cA[g] = (F[2] - F[0]) * (F[3] - F[1]);
                    cn[g] = members;
                    sslot[p] = g;
                }
                ncl += join ? 0 : 1;
                wave_sync();
            }
        }
        p0 += cnt;
    }
    __syncthreads();

    // ---- 3. conf, output order, output ----
    for (int g = tid; g < nk; g += kWbfThreads) {
        const int m = cn[g];
        if (m > 0) conf[g] = ((cS[g] / (double)m) * fmin((double)m, U)) / U;
    }
    __syncthreads();
    for (int g = tid; g < nk; g += kWbfThreads) {
        const int m = cn[g];
        if (m == 0) continue;
        const double c = conf[g];
        int rank = 0;
        // slots are ordered by class, then creation: the tie rule is the slot index ascending = precedes() on the NEGATED index
        for (int q = 0; q < nk; ++q) rank += (cn[q] > 0 && precedes(conf[q], -q, c, -g)) ? 1 : 0;
        crank[g] = rank;
        const size_t o = (size_t)beg + rank;
        for (int k = 0; k < 4; ++k) a.out_boxes[o * 4 + k] = cF[(size_t)k * R + g];
        a.out_scores[o] = (float)c;
        a.out_classes[o] = (float)scls[g];          // slot g lies in the run of its class
        a.out_members[o] = m;
    }
    if (tid == 0) {
        a.out_skipped[img] = n - nk;
    }
    __syncthreads();
    int ncl = 0;
    for (int p = tid; p < nk; p += kWbfThreads) a.out_cluster[(size_t)beg + ord[p]] = crank[sslot[p]];
    if (wave == 0) {        // the image's clusters: the occupied slots
        for (int g = lane; g < nk; g += 64) ncl += cn[g] > 0 ? 1 : 0;
        for (int m = 32; m >= 1; m >>= 1) ncl += __shfl_xor(ncl, m, 64);
        if (lane == 0) a.out_counts[img] = ncl;
    }
}

}  // namespace

extern "C" int pe_wbf_fuse_batch(const double* boxes, const double* scores, const int32_t* classes, const int32_t* row_source,
                                 const int32_t* offsets, const int32_t* row_counts, int32_t num_images, int32_t num_classes,
                                 int32_t max_rows_per_image, const double* det_weights, int32_t num_detectors, double iou_thresh,
                                 double skip_thresh, double* out_boxes, float* out_scores, float* out_classes, int32_t* out_counts,
                                 int32_t* out_cluster, int32_t* out_members, int32_t* out_skipped, void* stream) {
    const char* what = "pe_wbf_fuse_batch";
    PE_CHECK_ARG(num_images >= 0, "%s: num_images < 0", what);
    if (num_images == 0) return PE_OK;
    if (num_images > kWbfMaxImages) {
        pe::set_error("%s: num_images %d is above the %d images of one launch", what, num_images, kWbfMaxImages);
        return PE_ERR_UNSUPPORTED;
    }
    PE_CHECK_ARG(boxes && scores && classes && row_source && offsets && det_weights, "%s: null input pointer", what);
    PE_CHECK_ARG(out_boxes && out_scores && out_classes && out_counts && out_cluster && out_members && out_skipped,
                 "%s: null output pointer", what);
    PE_CHECK_ARG(num_classes >= 1, "%s: num_classes %d < 1", what, num_classes);
    PE_CHECK_ARG(num_detectors >= 1, "%s: num_detectors %d < 1", what, num_detectors);
    if (num_detectors > PE_WBF_MAX_DETECTORS) {
        pe::set_error("%s: num_detectors %d is above the %d entries of the weight table", what, num_detectors, PE_WBF_MAX_DETECTORS);
        return PE_ERR_UNSUPPORTED;
    }
    PE_CHECK_ARG(iou_thresh == iou_thresh, "%s: iou_thresh is NaN", what);
    PE_CHECK_ARG(skip_thresh == skip_thresh, "%s: skip_thresh is NaN", what);
    PE_CHECK_ARG(max_rows_per_image >= 1, "%s: max_rows_per_image %d < 1", what, max_rows_per_image);
    if (max_rows_per_image > wbf_capacity()) {
        pe::set_error("%s: max_rows_per_image %d is above the per-image capacity of %d rows (%zu bytes of LDS per row, 160 KiB, at every "
                      "class count)", what, max_rows_per_image, wbf_capacity(), wbf_row_bytes());
        return PE_ERR_UNSUPPORTED;
    }
    const int R = (max_rows_per_image + 1) & ~1;  // keep the int carves 8-byte aligned
    const size_t lds = wbf_lds_bytes(R);
    if (lds > 64 * 1024) PE_ENSURE_LDS(wbf_fuse_kernel, lds, what);
    const WbfArgs a{boxes, scores, classes, row_source, offsets, row_counts, num_images, num_classes, R, det_weights, num_detectors,
                    iou_thresh, skip_thresh, out_boxes, out_scores, out_classes, out_counts, out_cluster, out_members, out_skipped};
    hipLaunchKernelGGL(wbf_fuse_kernel, dim3(num_images), dim3(kWbfThreads), lds, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH(what);
    return PE_OK;
}
