// The candidate sweep: the first pass of the statistics that evaluate up to 64 candidates in one launch (pe_temperature_nll,
// pe_pool_nll, pe_bias_nll).  Lane = candidate, wavefront = item: the 64 lanes of a wave read the same item (a broadcast) and each
// keeps its own candidate and its own sums in registers.  DESIGN.md section 23.
//
// THE ORDER.  Wave w of workgroup g takes items g * 4 + w, + gridDim.x * 4, ... in that order; the workgroup adds its four waves in
// wave order and stores partial[(g * candidates + lane) * values + v]; pe::launch_finish (csrc/reduce2.h) adds the workgroups.  The grid
// is a function of the item count alone, so the same input gives the same bits.
//
// A statistic supplies a MODEL, passed to the kernel by value:
//   kMaxValues              the compile-time bound on the sums per candidate; sweep() keeps that many accumulators per lane and every
//                           loop over them is unrolled, so the model must index `acc` with compile-time constants only
//   Shared                  the LDS the model needs beside the hand-over (pe::NoShared: none); setup(sh) fills what the whole workgroup
//                           shares, and a barrier follows it
//   Lane, load(L, c, sh)    the per-lane state: candidate c (an idle lane gets candidate 0 and its sums are never stored)
//   item(L, acc, i, sh)     adds item i to the lane's sums; false (wave-uniform): the item is excluded, adds nothing and is flagged
//   items, nc, values()     the run-time counts;  partial, flags  where the results go
// and a named __global__ kernel whose body is pe::sweep(model).
//
// ZERO ITEMS: launch_sweep answers with a memset of the result (all sums 0) and the zeroed flags, without a launch.
#pragma once
#include "common.h"
#include "reduce2.h"

namespace pe {

constexpr int kSweepThreads = 256, kSweepWaves = kSweepThreads / 64;

struct NoShared {};

// The end of a sweep kernel: the lanes' sums go through LDS, thread (v, lane) adds value v of candidate lane over the workgroup's waves
// in wave order and stores it.  acc holds NV >= nv sums, indexed with compile-time constants only.
template <int NV>
__device__ __forceinline__ void sweep_store(const double (&acc)[NV], int nc, int nv, double* partial) {
    __shared__ double part[kSweepWaves][NV][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < NV; ++v) part[wv][v][lane] = acc[v];
    __syncthreads();
    for (int v = wv; v < nv; v += kSweepWaves) {
        if (lane < nc) {
            double s = part[0][v][lane];
            for (int u = 1; u < kSweepWaves; ++u) s += part[u][v][lane];
            partial[((size_t)blockIdx.x * nc + lane) * nv + v] = s;
        }
    }
}

template <class Model>
__device__ __forceinline__ void sweep(const Model& m) {
    constexpr int NV = Model::kMaxValues;
    __shared__ typename Model::Shared sh;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nc = m.nc;
    m.setup(sh);
    __syncthreads();
    typename Model::Lane L;
    m.load(L, lane < nc ? lane : 0, sh);
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    using Index = decltype(m.items);          // int or long long, as the statistic counts its items
    const Index step = (Index)gridDim.x * kSweepWaves;
    for (Index i = (Index)blockIdx.x * kSweepWaves + wv; i < m.items; i += step)      // wave-uniform
        if (!m.item(L, acc, i, sh) && lane == 0) flag_excluded(m.flags, i);
    sweep_store(acc, nc, m.values(), m.partial);
}

// zero_flags, the first pass over min(ceil(items / 4), max_blocks) workgroups, the second pass into out [nc * values]
template <class Model>
int launch_sweep(void (*kernel)(Model), const Model& m, int max_blocks, double* out, hipStream_t stream, const char* what) {
    const int nv = m.nc * m.values();
    if (int rc = zero_flags(m.flags, stream, what)) return rc;
    if (m.items == 0) {        // nothing to add up: zeros, no launch
        if (hipMemsetAsync(out, 0, (size_t)nv * sizeof(double), stream) != hipSuccess) {
            set_error("%s: hipMemsetAsync of the result failed", what);
            return PE_ERR_HIP;
        }
        return PE_OK;
    }
    const int blocks = (int)std::min<long long>((m.items + kSweepWaves - 1) / kSweepWaves, max_blocks);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kSweepThreads), 0, stream, m);
    PE_CHECK_LAUNCH(what);
    return launch_finish(m.partial, blocks, nv, 0, nullptr, out, stream, what);
}

// Host candidates -> dst on the device (the head of the workspace): they travel as kernel arguments, 256 doubles a launch, so the copy
// is stream-ordered and the host array is free again when the entry point returns.  what: the name PE_CHECK_LAUNCH reports.
struct StageArgs {
    double v[256];
    double* dst;
    int n;
};

static __global__ __launch_bounds__(256) void stage_kernel(StageArgs a) {
    if ((int)threadIdx.x < a.n) a.dst[threadIdx.x] = a.v[threadIdx.x];
}

inline int stage_candidates(const double* host, int n, double* dst, hipStream_t stream, const char* what) {
    for (int o = 0; o < n; o += 256) {
        StageArgs s{};
        s.n = std::min(256, n - o);
        s.dst = dst + o;
        for (int i = 0; i < s.n; ++i) s.v[i] = host[o + i];
        hipLaunchKernelGGL(stage_kernel, dim3(1), dim3(256), 0, stream, s);
        PE_CHECK_LAUNCH(what);
    }
    return PE_OK;
}

}  // namespace pe
