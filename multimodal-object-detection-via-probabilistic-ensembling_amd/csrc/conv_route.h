// Which kernel takes a pe_conv2d_nhwc_f16 launch: the one statement of the rule.
//
// Host-only (no HIP header: the host compiler alone builds it).  conv2_dispatch (csrc/conv_igemm2.hip) switches over choose();
// pe_test_conv_variant (csrc/test_hooks.h) returns name(choose()) for the same arguments, which is what labels bench.py's roofline
// table and what the tests assert their kernel with.  All kernels compute the same convolution (tests/test_conv_exact_gpu.py), so the
// choice never shows in a frame's result - only in its time.
#pragma once

namespace pe {
namespace route {

// what the choice depends on, as pe_conv2d_nhwc_f16 has resolved it (cout_store and out_stride are never 0)
struct ConvShape {
    int M, K, Cout;               // output pixels, reduction length (Cin; 9 Cin for a 3x3), output channels
    int mode3x3;                  // 0: 1x1 / GEMM, 1: 3x3 stride 1 pad 1
    int stride, res_mode, out_f32, has_bias;
    int cout_store, out_stride;
    long long in_pixels;          // N * H * W of the input
};

// the kernels conv2_dispatch launches, and the 7x7 stem kernel pe_conv2d_nhwc_f16 launches itself (csrc/conv_igemm.hip)
enum Kernel {
    RING,
    BIG_3X3, BIG_1X1,
    RB_128_64, RB_256_128, RB_128_128,
    IGEMM2_128_64_3X3, IGEMM2_128_128_3X3,
    IGEMM2_128_64_1X1,
    IGEMM2_256_128_1X1_2STAGE, IGEMM2_128_128_1X1_2STAGE,
    IGEMM2_256_128_1X1, IGEMM2_128_128_1X1,
    STEM,
};

// exactly what rocprofv3 prints behind the namespace
inline const char* name(Kernel k) {
    switch (k) {
        case RING: return "conv1x1_ring_kernel";
        case BIG_3X3: return "conv_big_kernel<1>";
        case BIG_1X1: return "conv_big_kernel<0>";
        case RB_128_64: return "conv3x3rb_kernel<128, 64>";
        case RB_256_128: return "conv3x3rb_kernel<256, 128>";
        case RB_128_128: return "conv3x3rb_kernel<128, 128>";
        case IGEMM2_128_64_3X3: return "conv_igemm2_kernel<128, 64, 1, 1>";
        case IGEMM2_128_128_3X3: return "conv_igemm2_kernel<128, 128, 1, 1>";
        case IGEMM2_128_64_1X1: return "conv_igemm2_kernel<128, 64, 0, 1>";
        case IGEMM2_256_128_1X1_2STAGE: return "conv_igemm2_kernel<256, 128, 0, 2>";
        case IGEMM2_128_128_1X1_2STAGE: return "conv_igemm2_kernel<128, 128, 0, 2>";
        case IGEMM2_256_128_1X1: return "conv_igemm2_kernel<256, 128, 0, 1>";
        case IGEMM2_128_128_1X1: return "conv_igemm2_kernel<128, 128, 0, 1>";
        case STEM: return "conv_igemm_kernel<128, 64, 2>";
    }
    return "?";
}

constexpr int RING_BN = 256;               // output channels per tile of the ring kernel (static_assert in csrc/conv1x1_ring.hip)
constexpr long long TWO_GIB = 1ll << 31;   // the ring kernel addresses its tensors with 32-bit buffer offsets

inline long long tiles(long long n, int tile) { return (n + tile - 1) / tile; }

// policy: tile_bits of pe_test_set_conv_policy (csrc/test_hooks.h), reuse3x3: its second argument
inline Kernel choose(const ConvShape& s, int policy, int reuse3x3) {
    const bool narrow = s.Cout <= 64;
    // persistent loader / consumer 1x1 kernel (csrc/conv1x1_ring.hip; bit-identical results): policy bit 5 = the long-K, 256-output
    // layers (res4 conv1), bit 6 = every eligible launch (residual-free, fp16 out, bias, Cout % 256 == 0; K >= 512 at stride 1, the
    // stride-2 shortcut convolutions from K = 256).  Chosen by channel counts and stride only, never by the batch.
    const bool ring_fits = s.Cout % RING_BN == 0 && s.cout_store == s.Cout && s.K % 64 == 0 && s.in_pixels * s.K * 2 < TWO_GIB &&
                           (long long)s.Cout * s.K * 2 < TWO_GIB && (long long)s.M * s.out_stride * 2 < TWO_GIB;
    if ((policy & 96) && !s.mode3x3 && (s.stride == 1 || s.stride == 2) && !s.out_f32 && s.has_bias && ring_fits) {
        bool take;
        if (!(policy & 64)) take = s.stride == 1 && !s.res_mode && s.K >= 1024 && s.Cout == 256;
        else if (s.res_mode) take = s.stride == 1 && s.K >= 128 && (policy & 256) && (long long)s.M * s.Cout * 2 < TWO_GIB;      // bit 8: the residual layers too (conv3 of res3 / res5, FPN laterals)
        else take = s.K >= (s.stride == 1 ? 512 : 256);
        if (take) return RING;
    }
    // 256 x 256 two-stage kernel: fp16 output, whole 256-channel tiles, a grid that fills the 256 CUs
    // (measured r01: +24 % on the K = 12544 FC GEMM, neutral-to-negative on the convolutions -> long-K GEMMs only;
    //  policy bit 4 forces it everywhere it applies, for A/B runs)
    if ((policy & 8) && !s.out_f32 && s.Cout % 256 == 0 && s.cout_store == s.Cout && tiles(s.M, 256) * (s.Cout / 256) >= 224 &&
        ((policy & 16) || (!s.mode3x3 && s.K >= 4096)))
        return s.mode3x3 ? BIG_3X3 : BIG_1X1;
    if (s.mode3x3 && reuse3x3) {
        if (narrow) return RB_128_64;
        // 256-row tiles (8 waves) halve the weight-tile traffic per flop; keep 128 when the grid would not fill the chip
        const bool big = (policy & 1) && tiles(s.M, 256) * tiles(s.Cout, 128) >= 512;
        return big ? RB_256_128 : RB_128_128;
    }
    if (s.mode3x3) return narrow ? IGEMM2_128_64_3X3 : IGEMM2_128_128_3X3;
    if (narrow) return IGEMM2_128_64_1X1;
    const bool big1 = (policy & 2) && tiles(s.M, 256) * tiles(s.Cout, 128) >= 512;
    if (policy & 4) return big1 ? IGEMM2_256_128_1X1_2STAGE : IGEMM2_128_128_1X1_2STAGE;
    return big1 ? IGEMM2_256_128_1X1 : IGEMM2_128_128_1X1;
}

}  // namespace route
}  // namespace pe
