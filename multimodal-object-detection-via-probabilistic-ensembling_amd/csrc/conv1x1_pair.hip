// res3: conv3 + identity of a bottleneck block and conv1 of the NEXT block in one launch.
//
// Replaces, for a pair of consecutive identity blocks, the reference rows backbone/resnet.py:205-221 of the first block from conv3 on
//     y   = relu(fp16(W3 . t2 + b3 + residual))      128 -> 512, the block output (still written: the next block's shortcut and the FPN read it)
// and the first convolution of the second block
//     t1' = relu(fp16(W1' . y + b1'))                512 -> 128
// which today are a conv1x1_ring_kernel<true, true> launch and a conv_igemm2_kernel<128, 128> launch.  The second launch reads back the
// 1 KiB per pixel the first has just written; here y goes from the first product to the second through LDS, as fp16 - the rounding
// the round trip through HBM applies - and that read never reaches HBM.
//
// Structure.  One workgroup of four waves per CU (one wave per SIMD), persistent: workgroup w owns a contiguous run of 64-pixel tiles.
//   * Both weight matrices (2 x 128 KiB) live in REGISTERS for the whole launch, as MFMA A fragments: wave v holds rows [128 v, +128)
//     of W3 (32 fragments) and rows [32 v, +32) of W1' (32 fragments), 256 registers of the wave's 512.  No weight byte moves after
//     the prologue, neither through L2 nor through LDS.
//   * LDS holds two stages of 80 KiB: the tile's residual (64 px x 512 ch, later overwritten IN PLACE by y) and its t2 slab (64 px x 128 ch,
//     later the t1' output patch), both in the K-slab layout of the other 1x1 kernels ([64-channel slab][pixel row][8 chunks of 16 B],
//     chunk p of row r holding channels 8 (p ^ ((r >> 1) & 7))), filled by `buffer_load_dwordx4 ... lds`.  The next tile's stage is in
//     flight while this tile computes.
//   * product 1: per 64-channel slab of the wave's two and per 32-pixel block, two 32x32 accumulators, K = 128 from the t2 slab; the epilogue
//     adds bias (64 floats through the scalar cache per slab), then the residual read from LDS, ReLU, fp16, and writes y over the
//     residual.  The wave then stores its own two slabs as whole 128-byte lines.
//   * product 2 (after a barrier: every wave reads all 512 y channels): two 32x32 accumulators per wave (64 pixels x its 32 t1' channels), K = 512
//     from the y slabs with the fragment reads of the other 1x1 kernels; bias, ReLU, fp16 into the patch, barrier, whole 256-byte rows out.
// Bits: v_mfma_f32_32x32x16_f16, zero-initialised fp32 accumulators, K ascending, channel 16 ks + 8 (lane >> 5) + e in k-slot e of MFMA
// K-step ks exactly as conv_igemm2 / conv1x1_ring place it, the ring kernel's residual epilogue order (acc + bias, + residual), nothing
// summed across waves: y and t1' are the bits of the two launches (tests/test_conv1x1_pair_gpu.py).
// Rows beyond M are fetched as zeros through the buffer bounds check and their stores are dropped by it: one code path for partial tiles.
#include <atomic>
#include <cstdint>

#include "conv_common.h"

namespace {

typedef int int4v __attribute__((ext_vector_type(4)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));
typedef float float8v __attribute__((ext_vector_type(8)));

constexpr int PR_BM = 64;                        // pixels per tile
constexpr int PR_K1 = 128, PR_CY = 512, PR_C2 = 128;
constexpr int PR_SLAB_B = PR_BM * ROW_B;         // 8 KiB: 64 channels of 64 pixels
constexpr int PR_Y_B = (PR_CY / 64) * PR_SLAB_B;     // 64 KiB
constexpr int PR_T_B = (PR_K1 / 64) * PR_SLAB_B;     // 16 KiB
constexpr int PR_STAGE_B = PR_Y_B + PR_T_B;      // 80 KiB
constexpr int PR_LDS = 2 * PR_STAGE_B;           // 160 KiB: the whole CU
constexpr int PR_THREADS = 256;
constexpr unsigned PR_OOB = 0x80000000u;
static_assert(PR_LDS == 160 * 1024, "two stages fill the CU's LDS");
static_assert(PR_BM * PR_C2 * 2 == PR_T_B, "the t1' patch re-uses the t2 slab");

struct PairArgs {
    const _Float16* t2;
    const _Float16* w3;
    const float* b3;
    const _Float16* res;
    const _Float16* w1;
    const float* b1;
    _Float16* y;
    _Float16* t1;
    int M, ntiles;
};

__device__ __forceinline__ int4v pr_make_rsrc(const void* p, unsigned bytes) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(p);
    int4v r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
    r[1] = __builtin_amdgcn_readfirstlane((int)((a >> 32) & 0xffffu));
    r[2] = __builtin_amdgcn_readfirstlane((int)bytes);
    r[3] = 0x00020000;
    return r;
}

// two LDS-DMA pieces (64 lanes x 16 B each, lane-linear) at LDS byte addresses lds and lds + 1 KiB; v0 / v1 = per-lane byte offsets
// into the buffer (PR_OOB: the bounds check returns zeros and fetches nothing), soff = wave-uniform byte offset.  M0 is
// compiler-reserved: saved and restored inside the statement (the statement of csrc/conv1x1_ring.hip, two pieces long).
__device__ __forceinline__ void pr_dma2(unsigned lds, int4v rsrc, unsigned soff, unsigned v0, unsigned v1) {
    unsigned keep;
    lds = __builtin_amdgcn_readfirstlane(lds);
    soff = __builtin_amdgcn_readfirstlane(soff);
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %4, %2, %3 offen lds\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %5, %2, %3 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(lds), "s"(rsrc), "s"(soff), "v"(v0), "v"(v1)
        : "scc", "memory");
}

// NB floats of bias through the SCALAR cache (the address is wave-uniform), issued together and waited for once: the statements of
// csrc/conv1x1_ring.hip (asm, because the compiler will not prove that the kernel's own stores leave the bias alone and falls back to
// per-lane vector loads, which queue behind the DMA stream).  v[4 j + q] = channels [32 j + 8 q, +8).
struct PrBias64 { float8v v[8]; };
struct PrBias32 { float8v v[4]; };
__device__ __forceinline__ unsigned long long pr_uniform(const float* p) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ void pr_bias_issue(PrBias64& b, const float* p) {
    asm volatile(
        "s_load_dwordx8 %0, %8, 0x0\n\ts_load_dwordx8 %1, %8, 0x20\n\ts_load_dwordx8 %2, %8, 0x40\n\ts_load_dwordx8 %3, %8, 0x60\n\t"
        "s_load_dwordx8 %4, %8, 0x80\n\ts_load_dwordx8 %5, %8, 0xa0\n\ts_load_dwordx8 %6, %8, 0xc0\n\ts_load_dwordx8 %7, %8, 0xe0"
        : "=&s"(b.v[0]), "=&s"(b.v[1]), "=&s"(b.v[2]), "=&s"(b.v[3]), "=&s"(b.v[4]), "=&s"(b.v[5]), "=&s"(b.v[6]), "=&s"(b.v[7])
        : "s"(pr_uniform(p)));
}
__device__ __forceinline__ void pr_bias_issue(PrBias32& b, const float* p) {
    asm volatile("s_load_dwordx8 %0, %4, 0x0\n\ts_load_dwordx8 %1, %4, 0x20\n\ts_load_dwordx8 %2, %4, 0x40\n\ts_load_dwordx8 %3, %4, 0x60"
                 : "=&s"(b.v[0]), "=&s"(b.v[1]), "=&s"(b.v[2]), "=&s"(b.v[3])
                 : "s"(pr_uniform(p)));
}
__device__ __forceinline__ void pr_bias_wait(PrBias64& b) {      // every later use of b depends on this statement
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+s"(b.v[0]), "+s"(b.v[1]), "+s"(b.v[2]), "+s"(b.v[3]), "+s"(b.v[4]), "+s"(b.v[5]), "+s"(b.v[6]), "+s"(b.v[7]));
}
__device__ __forceinline__ void pr_bias_wait(PrBias32& b) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(b.v[0]), "+s"(b.v[1]), "+s"(b.v[2]), "+s"(b.v[3]));
}

// MFMA row i of a 32-channel block <- weight row perm(i): lane half h then holds channels 16 h + e in accumulator register e
// (conv1x1_ring's rg_perm)
__device__ __forceinline__ int pr_perm(int i) { return ((i >> 2) & 1) * 16 + (i >> 3) * 4 + (i & 3); }

__global__ __launch_bounds__(PR_THREADS) void conv1x1_pair_kernel(PairArgs a) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    typedef __attribute__((address_space(3))) unsigned char lds_byte;
    const unsigned smem_base = (unsigned)(unsigned long long)(lds_byte*)smem;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;
    const int tb0 = (int)((long long)blockIdx.x * a.ntiles / G), tb1 = (int)((long long)(blockIdx.x + 1) * a.ntiles / G);
    if (tb1 <= tb0) return;

    const int frow = lane & 31, fkh = lane >> 5;
    const int fsw = (frow >> 1) & 7;                 // (32 i + frow) >> 1 & 7
    const int prow = pr_perm(frow);
    const int lrow = lane >> 3, lp = lane & 7;

    const int4v rs_res = pr_make_rsrc(a.res, (unsigned)a.M * (PR_CY * 2));
    const int4v rs_t2 = pr_make_rsrc(a.t2, (unsigned)a.M * (PR_K1 * 2));
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, a.M * (PR_CY * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rt1 = __builtin_amdgcn_make_buffer_rsrc(a.t1, 0, a.M * (PR_C2 * 2), 0x00020000);

    // ---- loads of a tile: wave v fetches pixel rows [16 v, +16) of every slab (two 8-row pieces per slab) ----
    auto dma_y = [&](int tile, int stage) {
        unsigned vo[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int r = (wave * 2 + g) * 8 + lrow, m = tile * PR_BM + r;
            vo[g] = m < a.M ? (unsigned)m * (PR_CY * 2) + (unsigned)((lp ^ ((r >> 1) & 7)) * 16) : PR_OOB;
        }
        const unsigned lds = smem_base + stage * PR_STAGE_B + wave * 2048;
#pragma unroll
        for (int s = 0; s < PR_CY / 64; ++s) pr_dma2(lds + s * PR_SLAB_B, rs_res, (unsigned)(s * 128), vo[0], vo[1]);
    };
    auto dma_t = [&](int tile, int stage) {
        unsigned vo[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int r = (wave * 2 + g) * 8 + lrow, m = tile * PR_BM + r;
            vo[g] = m < a.M ? (unsigned)m * (PR_K1 * 2) + (unsigned)((lp ^ ((r >> 1) & 7)) * 16) : PR_OOB;
        }
        const unsigned lds = smem_base + stage * PR_STAGE_B + PR_Y_B + wave * 2048;
#pragma unroll
        for (int s = 0; s < PR_K1 / 64; ++s) pr_dma2(lds + s * PR_SLAB_B, rs_t2, (unsigned)(s * 128), vo[0], vo[1]);
    };
    dma_y(tb0, 0);
    dma_t(tb0, 0);

    // ---- the launch's weights, once: MFMA A fragments (row perm(lane & 31), k-chunk lane >> 5) straight from memory ----
    half8 w3f[4][8], w1f[32];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            w3f[j][ks] = *reinterpret_cast<const half8*>(a.w3 + (wave * 128 + j * 32 + prow) * PR_K1 + ks * 16 + fkh * 8);
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) w1f[ks] = *reinterpret_cast<const half8*>(a.w1 + (wave * 32 + prow) * PR_CY + ks * 16 + fkh * 8);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (int tile = tb0; tile < tb1; ++tile) {
        const int stage = (tile - tb0) & 1;
        unsigned char* ys = smem + stage * PR_STAGE_B;      // residual, then y: 8 slabs
        unsigned char* ts = ys + PR_Y_B;                    // t2: 2 slabs, then the t1' patch
        const int m0 = tile * PR_BM;
        // the next tile's residual into the other stage (its y was last read before the previous tile's second barrier)
        if (tile + 1 < tb1) dma_y(tile + 1, stage ^ 1);

        // ---- product 1 + epilogue: per 64-channel slab of the wave's two and per 32-pixel block, two accumulators ----
#pragma unroll
        for (int jh = 0; jh < 2; ++jh) {
            PrBias64 bs;
            pr_bias_issue(bs, a.b3 + wave * 128 + jh * 64);      // in flight under the first block's MFMAs
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float16v acc[2];
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
                const unsigned char* pa = ts + (i * 32 + frow) * ROW_B;
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    const half8 pf = *reinterpret_cast<const half8*>(pa + (ks >> 2) * PR_SLAB_B + ((((ks & 3) * 2 + fkh) ^ fsw) << 4));
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w3f[jh * 2 + j][ks], pf, acc[j], 0, 0, 0);
                }
                if (i == 0) pr_bias_wait(bs);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // the lane's channels 32 j + 16 fkh + [0, 16) of the slab: its chunks c0, c0 + 1
                    const int c0 = j * 4 + fkh * 2;
                    unsigned char* row = ys + (wave * 2 + jh) * PR_SLAB_B + (i * 32 + frow) * ROW_B;
                    half8* p0 = reinterpret_cast<half8*>(row + ((c0 ^ fsw) << 4));
                    half8* p1 = reinterpret_cast<half8*>(row + (((c0 + 1) ^ fsw) << 4));
                    const half8 r0 = *p0, r1 = *p1;
                    half8 h0, h1;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float b0 = fkh ? bs.v[j * 4 + 2][e] : bs.v[j * 4 + 0][e];
                        const float b1 = fkh ? bs.v[j * 4 + 3][e] : bs.v[j * 4 + 1][e];
                        float x0 = acc[j][e] + b0, x1 = acc[j][e + 8] + b1;      // the ring kernel's order: + bias, then + residual
                        x0 += (float)r0[e];
                        x1 += (float)r1[e];
                        h0[e] = (_Float16)pe::relu_nan(x0);
                        h1[e] = (_Float16)pe::relu_nan(x1);
                    }
                    *p0 = h0;
                    *p1 = h1;
                }
            }
        }
        // ---- y out: the wave's own two slabs, 8 whole 128-byte lines per instruction (the wave reads what it wrote itself) ----
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int s = wave * 2 + (q >> 3), r = (q & 7) * 8 + lrow;
            const half8 v = *reinterpret_cast<const half8*>(ys + s * PR_SLAB_B + (q & 7) * 1024 + lane * 16);
            const unsigned off = m0 + r < a.M ? (unsigned)(m0 + r) * (PR_CY * 2) + (unsigned)(s * 128 + ((lp ^ ((r >> 1) & 7)) << 4)) : PR_OOB;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4v, v), ry, off, 0, 0);
        }
        __syncthreads();      // y is complete; nobody reads this tile's t2 slab or the previous tile's patch any more
        if (tile + 1 < tb1) dma_t(tile + 1, stage ^ 1);

        // ---- product 2: 64 pixels x the wave's 32 channels, K = 512 from the y slabs ----
        PrBias32 bn;
        pr_bias_issue(bn, a.b1 + wave * 32);
        float16v acc2[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc2[i][e] = 0.f;
        {
            // two MFMA K-steps per group, the next group's fragments requested behind this group's MFMAs.  sched_barrier(0): left
            // alone, the scheduler hoists all 64 fragment reads (256 registers) above the first MFMA and spills the weights
            const unsigned char* pa = ys + frow * ROW_B;
            half8 pf[2][2][2];
            auto load = [&](int grp, int buf) {
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const int ks = grp * 2 + kk;
                    const int ch = (((ks & 3) * 2 + fkh) ^ fsw) << 4;
#pragma unroll
                    for (int i = 0; i < 2; ++i) pf[buf][kk][i] = *reinterpret_cast<const half8*>(pa + (ks >> 2) * PR_SLAB_B + i * 32 * ROW_B + ch);
                }
            };
            load(0, 0);
#pragma unroll
            for (int grp = 0; grp < 16; ++grp) {
                if (grp + 1 < 16) load(grp + 1, (grp + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        acc2[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1f[grp * 2 + kk], pf[grp & 1][kk][i], acc2[i], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        pr_bias_wait(bn);
        // bias, ReLU, fp16 into the patch: [64 px][256 B], 16-byte chunk c of row r in slot c ^ (r & 15)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            half8 h0, h1;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float b0 = fkh ? bn.v[2][e] : bn.v[0][e];
                const float b1 = fkh ? bn.v[3][e] : bn.v[1][e];
                h0[e] = (_Float16)pe::relu_nan(acc2[i][e] + b0);
                h1[e] = (_Float16)pe::relu_nan(acc2[i][e + 8] + b1);
            }
            const int r = i * 32 + frow, c0 = wave * 4 + fkh * 2;
            *reinterpret_cast<half8*>(ts + r * 256 + ((c0 ^ (r & 15)) << 4)) = h0;
            *reinterpret_cast<half8*>(ts + r * 256 + (((c0 + 1) ^ (r & 15)) << 4)) = h1;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of the next tile have landed (and its y stores are out)
        __syncthreads();                                      // ... everybody's; the patch is complete
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int piece = wave * 4 + q, r = piece * 4 + (lane >> 4);
            const half8 v = *reinterpret_cast<const half8*>(ts + piece * 1024 + lane * 16);
            const unsigned off = m0 + r < a.M ? (unsigned)(m0 + r) * (PR_C2 * 2) + (unsigned)((((lane & 15) ^ (r & 15))) << 4) : PR_OOB;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uint4v, v), rt1, off, 0, 0);
        }
    }
}

// CUs of the current device, asked once per device (the persistent grid is one workgroup per CU; any grid gives the same results)
int pair_cu_count() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        pe::set_error("pe_conv1x1_pair_f16: hipGetDevice failed");
        return 0;
    }
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            pe::set_error("pe_conv1x1_pair_f16: cannot read the CU count of device %d", dev);
            return 0;
        }
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

}  // namespace

extern "C" int pe_conv1x1_pair_supported(int32_t Cin, int32_t Cout, int32_t Cnext, int64_t pixels) {
    return Cin == PR_K1 && Cout == PR_CY && Cnext == PR_C2 && pixels * PR_CY * 2 < (1ll << 31);
}

extern "C" int pe_conv1x1_pair_f16(const void* t2, const void* w3, const float* b3, const void* residual, const void* w1_next,
                                   const float* b1_next, void* out, void* t1_next, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                   int32_t Cout, int32_t Cnext, void* stream) {
    PE_CHECK_ARG(t2 && w3 && b3 && residual && w1_next && b1_next && out && t1_next, "pe_conv1x1_pair_f16: null pointer");
    PE_CHECK_ARG(N > 0 && H > 0 && W > 0, "pe_conv1x1_pair_f16: bad dims");
    const long long M = (long long)N * H * W;
    PE_CHECK_ARG(pe_conv1x1_pair_supported(Cin, Cout, Cnext, M),
                 "pe_conv1x1_pair_f16: channels must be 128 -> 512 -> 128 (got %d -> %d -> %d) and no tensor larger than 2 GiB (32-bit buffer offsets; "
                 "got %lld pixels)", Cin, Cout, Cnext, M);
    // the next tile's inputs are fetched while this tile's outputs are stored: neither output may overlap an input tensor or the other output
    {
        const uintptr_t t2_b = (uintptr_t)M * PR_K1 * 2, y_b = (uintptr_t)M * PR_CY * 2, t1_b = (uintptr_t)M * PR_C2 * 2;
        auto apart = [](const void* p, uintptr_t pb, const void* q, uintptr_t qb) {
            return (uintptr_t)p + pb <= (uintptr_t)q || (uintptr_t)q + qb <= (uintptr_t)p;
        };
        PE_CHECK_ARG(apart(out, y_b, t2, t2_b) && apart(out, y_b, residual, y_b) && apart(t1_next, t1_b, t2, t2_b) &&
                         apart(t1_next, t1_b, residual, y_b) && apart(out, y_b, t1_next, t1_b),
                     "pe_conv1x1_pair_f16: out and t1_next must not overlap t2, residual or each other");
    }
    PairArgs a{};
    a.t2 = (const _Float16*)t2; a.w3 = (const _Float16*)w3; a.b3 = b3; a.res = (const _Float16*)residual;
    a.w1 = (const _Float16*)w1_next; a.b1 = b1_next; a.y = (_Float16*)out; a.t1 = (_Float16*)t1_next;
    a.M = (int)M; a.ntiles = pe::ceil_div(M, PR_BM);
    const int cus = pair_cu_count();      // one workgroup per CU: each takes a CU's whole LDS and register file
    if (cus <= 0) return PE_ERR_HIP;
    const int grid = a.ntiles < cus ? a.ntiles : cus;
    PE_ENSURE_LDS(conv1x1_pair_kernel, (size_t)PR_LDS, "pe_conv1x1_pair_f16");
    hipLaunchKernelGGL(conv1x1_pair_kernel, dim3(grid), dim3(PR_THREADS), (size_t)PR_LDS, (hipStream_t)stream, a);
    PE_CHECK_LAUNCH("pe_conv1x1_pair_f16");
    return PE_OK;
}
