// The second pass, the exclusion flags and the workgroup tree of the six device-side calibration statistics: pe_temperature_nll,
// pe_pool_nll and pe_bias_nll (through csrc/sweep.h), pe_reliability_logits / _scores and pe_box_pair_stats take the second pass and the
// flags, pe_variance_stats the flags only; pe_variance_stats and pe_box_pair_stats add a workgroup's threads with block_tree.
// DESIGN.md sections 16 and 23.
//
// A first-pass kernel leaves nv eight-byte values per workgroup, partial[(size_t)k * nv + v] for workgroup k: the leading n_int of them
// int64 counts, the rest doubles.  No floating-point atomics anywhere, and the first-pass grid is a function of the item count alone,
// so the same input gives the same bits.
//
// THE SUMMATION ORDER (the one statement of it; tests/test_stat_sums_golden_gpu.py pins it to the bits recorded before this header
// existed).  Per value, with per = ceil(blocks / 16):
//   segment g of the 16 adds workgroups [g * per, min(blocks, (g + 1) * per)) in workgroup order, starting from 0;
//   then the 16 segment sums are added in segment order.
// Counts are integers: exact in any order.
//
// A file that takes the flags only defines PE_REDUCE2_FLAGS_ONLY before the include and carries no copy of the finish kernel.
#pragma once
#include "common.h"

namespace pe {

// flags[0] += 1, flags[1] = max(flags[1], 1 + index) saturating at INT32_MAX: the excluded items and one of them (the last).  The
// caller keeps its own lane predicate (lane == 0 where a wavefront owns the item).
__device__ __forceinline__ void flag_excluded(int32_t* flags, long long index) {
    atomicAdd(&flags[0], 1);
    atomicMax(&flags[1], (int)min(index + 1, (long long)0x7fffffff));
}

inline int zero_flags(int32_t* flags, hipStream_t stream, const char* what) {
    if (hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), stream) != hipSuccess) {
        set_error("%s: hipMemsetAsync of the flags failed", what);
        return PE_ERR_HIP;
    }
    return PE_OK;
}

// x[0 .. n - 1] of NV values each -> x[0], stride-halving tree: level by level, the same pairs whatever the data.  n is a power of two
// and the workgroup's size; the caller fills x before and lets thread 0 read x[0] after (no barrier follows the last level).
template <typename T, int NV>
__device__ __forceinline__ void block_tree(T (*x)[NV], int n) {
    for (int s = n >> 1; s > 0; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s)
            for (int v = 0; v < NV; ++v) x[threadIdx.x][v] += x[threadIdx.x + s][v];
    }
}

#ifndef PE_REDUCE2_FLAGS_ONLY

constexpr int kFinishSegments = 16;

// one workgroup of 16 segments x 64 lanes per 64 values: lane t of workgroup w owns value v = 64 w + t, a count where v < n_int
// (static: every file that launches it carries its own copy)
static __global__ __launch_bounds__(64 * kFinishSegments) void finish_kernel(const double* partial, int blocks, int nv, int n_int,
                                                                             long long* out_int, double* out_dbl) {
    __shared__ long long seg_int[kFinishSegments][64];
    __shared__ double seg_dbl[kFinishSegments][64];
    const int t = threadIdx.x & 63, g = threadIdx.x >> 6, v = blockIdx.x * 64 + t;
    const bool live = v < nv, is_int = v < n_int;
    const int per = (blocks + kFinishSegments - 1) / kFinishSegments;
    long long c = 0;
    double s = 0.0;
    if (live) {
        const int end = min(blocks, (g + 1) * per);
        for (int k = g * per; k < end; ++k) {
            const double x = partial[(size_t)k * nv + v];
            if (is_int) c += __double_as_longlong(x);
            else s += x;
        }
    }
    seg_int[g][t] = c;
    seg_dbl[g][t] = s;
    __syncthreads();
    if (g == 0 && live) {
        for (int k = 1; k < kFinishSegments; ++k) {
            c += seg_int[k][t];
            s += seg_dbl[k][t];
        }
        if (is_int) out_int[v] = c;
        else out_dbl[v - n_int] = s;
    }
}

// out_int [n_int] (not read when n_int is 0), out_dbl [nv - n_int]
inline int launch_finish(const double* partial, int blocks, int nv, int n_int, long long* out_int, double* out_dbl, hipStream_t stream,
                         const char* what) {
    hipLaunchKernelGGL(finish_kernel, dim3((nv + 63) / 64), dim3(64 * kFinishSegments), 0, stream, partial, blocks, nv, n_int, out_int, out_dbl);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s (finish): launch failed: %s", what, hipGetErrorString(e));
        return PE_ERR_HIP;
    }
    return PE_OK;
}

#endif  // PE_REDUCE2_FLAGS_ONLY

}  // namespace pe
