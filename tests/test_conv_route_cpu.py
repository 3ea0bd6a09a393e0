"""csrc/conv_route.h through its two hooks, without a GPU: pe_test_conv_variant names the kernel that pe_conv2d_nhwc_f16's dispatch picks
(the dispatch switches over the same choose()), and pe_conv1x1_pair_supported is the check pe_conv1x1_pair_f16 makes.  Both are plain
host functions.

The reference under the default policy is `frozen_variant_name`: the body layers.conv_variant_name had while it restated the rule in
Python (the commit before DESIGN 22), kept here so that moving the rule into the library is shown to have moved no label.  One term was
added to it, marked below: the Python copy sent every long-K launch with whole 256-channel tiles and a full grid to conv_big_kernel, the
dispatch only those with fp16 output and cout_store == Cout (conv_big's epilogue writes nothing else).  No launch of the detectors has
such a shape, so no label was wrong - but the sweep below has them, and there the dispatch is the truth."""
import ctypes
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGE_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}


def frozen_variant_name(M, Cout, kernel, K=0, *, stride=1, residual_mode=0, out_f32=False, has_bias=True, cout_store=0, out_stride=0, in_pixels=None):
    bn = 64 if Cout <= 64 else 128
    if kernel == 7:
        return "conv_igemm_kernel<128, 64, 2>"          # 7x7 stem, register-staged kernel
    if kernel == 1:
        ring = (stride in (1, 2) and not out_f32 and has_bias and Cout % 256 == 0
                and (K >= (512 if stride == 1 else 256) if residual_mode == 0 else (stride == 1 and K >= 128 and M * Cout * 2 < 2 ** 31))
                and (cout_store or Cout) == Cout and (in_pixels or M) * K * 2 < 2 ** 31 and Cout * K * 2 < 2 ** 31 and M * (out_stride or Cout) * 2 < 2 ** 31)
        if ring:
            return "conv1x1_ring_kernel"                # persistent loader / consumer kernel (csrc/conv1x1_ring.hip)
        if (K >= 4096 and Cout % 256 == 0 and ((M + 255) // 256) * (Cout // 256) >= 224
                and not out_f32 and (cout_store or Cout) == Cout):      # <- the added term (module docstring)
            return "conv_big_kernel<0>"                 # 256x256 two-stage kernel (long-K GEMM)
        return f"conv_igemm2_kernel<128, {bn}, 0, 1>"   # LDS-DMA 1x1 / GEMM
    if bn == 64:
        return "conv3x3rb_kernel<128, 64>"
    big = ((M + 255) // 256) * ((Cout + 127) // 128) >= 512
    return f"conv3x3rb_kernel<{256 if big else 128}, 128>"  # kw-reuse 3x3, double-buffered weight tile


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from proben_amd import layers
    assert layers._lib.test_hooks().pe_test_get_conv_policy() == layers.DEFAULT_CONV_POLICY      # every test that sets one puts it back
    return layers


def detector_convs(depth, N, H=512, W=640):
    """(M, Cout, kernel, K, keywords) of every pe_conv2d_nhwc_f16 launch of an R-`depth`-FPN forward on N frames of H x W with no fused
    launch: stem, bottlenecks (stride in the 1x1), FPN, RPN head on five levels, the three FC layers on 1000 proposals per frame."""
    out = [(N * (H // 2) * (W // 2), 64, 7, 4, dict(stride=2, in_pixels=N * H * W))]
    h, w, cin = H // 4, W // 4, 64
    levels = []
    for si, nb in enumerate(STAGE_BLOCKS[depth]):
        mid, cout = 64 << si, 256 << si
        for bi in range(nb):
            s = 2 if (bi == 0 and si > 0) else 1
            px_in, h, w = N * h * w, h // s, w // s
            M = N * h * w
            if bi == 0:
                out.append((M, cout, 1, cin, dict(stride=s, in_pixels=px_in)))                      # shortcut
            out.append((M, mid, 1, cin, dict(stride=s, in_pixels=px_in)))                           # conv1
            out.append((M, mid, 3, 9 * mid, {}))                                                    # conv2
            out.append((M, cout, 1, mid, dict(residual_mode=1)))                                    # conv3
            cin = cout
        levels.append((h, w, cin))
    for i, (h, w, c) in enumerate(levels):
        out.append((N * h * w, 256, 1, c, dict(residual_mode=0 if i == 3 else 2)))                  # FPN lateral
        out.append((N * h * w, 256, 3, 9 * 256, {}))                                                # FPN output
    for h, w in [(h, w) for h, w, _ in levels] + [((levels[3][0] + 1) // 2, (levels[3][1] + 1) // 2)]:
        out.append((N * h * w, 256, 3, 9 * 256, {}))                                                # RPN conv
        out.append((N * h * w, 15, 1, 256, dict(out_f32=True, cout_store=15, out_stride=16)))       # RPN head
    out.append((N * 1000, 1024, 1, 49 * 256, {}))
    out.append((N * 1000, 1024, 1, 1024, {}))
    out.append((N * 1000, 17, 1, 1024, dict(out_f32=True, cout_store=17, out_stride=24)))
    return out


def edge_grid():
    """Cout x K x stride x residual mode x output type x bias x size, for the 1x1 and the 3x3: the sizes sit on both sides of the 224-tile
    threshold of conv_big (Cout 256: 224 tiles of 256 pixels), of the 512-tile threshold of the 256-row 3x3 tiles (Cout 256: 256 tiles,
    Cout 128: 512) and of the ring kernel's 2 GiB terms: M * out_stride * 2 and M * Cout * 2 (Cout 256: 2^22 pixels), in_pixels * K * 2
    (with its own axis below: the input of a strided launch) and Cout * K * 2 (its own cases: no layer is that wide)."""
    sizes = [1, 1000, 223 * 256, 223 * 256 + 1, 224 * 256, 255 * 256, 255 * 256 + 1, 511 * 256, 511 * 256 + 1, 2 ** 22 - 1, 2 ** 22]
    couts = [(64, {}), (128, {}), (256, {}), (15, dict(cout_store=15, out_stride=16)), (256, dict(out_stride=512))]
    for (cout, store), K, stride, res, f32, bias, M, kernel in itertools.product(
            couts, (64, 128, 256, 512, 1024, 4096, 12544), (1, 2), (0, 1, 2), (False, True), (True, False), sizes, (1, 3)):
        yield M, cout, kernel, K, dict(stride=stride, residual_mode=res, out_f32=f32, has_bias=bias, in_pixels=M * stride * stride, **store)
    for K, px in itertools.product((256, 1024, 4096), (-1, 0)):      # in_pixels * K * 2 on both sides of 2^31, few output pixels
        for stride, res in ((1, 0), (2, 0), (1, 1)):
            yield 4096, 256, 1, K, dict(stride=stride, residual_mode=res, in_pixels=2 ** 30 // K + px)
    for K in (2048, 4096):                                           # Cout * K * 2 on both sides of 2^31
        yield 1000, 2 ** 18, 1, K, {}


def test_default_policy_names_are_the_frozen_python_rule_on_every_detector_layer_and_an_edge_grid(L):
    cases = [c for depth in (50, 101) for N in (1, 32) for c in detector_convs(depth, N)] + list(edge_grid())
    seen = set()
    for M, cout, kernel, K, kw in cases:
        want = frozen_variant_name(M, cout, kernel, K, **kw)
        assert L.conv_variant_name(M, cout, kernel, K, **kw) == want, (M, cout, kernel, K, kw)
        seen.add(want)
    # the sweep reaches every kernel the default policy can choose, so neither side agrees by never leaving one branch
    assert seen == {"conv_igemm_kernel<128, 64, 2>", "conv1x1_ring_kernel", "conv_big_kernel<0>", "conv_igemm2_kernel<128, 64, 0, 1>",
                    "conv_igemm2_kernel<128, 128, 0, 1>", "conv3x3rb_kernel<128, 64>", "conv3x3rb_kernel<128, 128>", "conv3x3rb_kernel<256, 128>"}
    # R50 at batch 32: the layers whose kernels the roofline table and the conv tests name
    r50 = {(M, cout, k, K): frozen_variant_name(M, cout, k, K, **kw) for M, cout, k, K, kw in detector_convs(50, 32)}
    assert r50[32 * 32 * 40, 256, 1, 1024] == "conv1x1_ring_kernel"                       # res4 conv1
    assert r50[32 * 64 * 80, 512, 1, 128] == "conv1x1_ring_kernel"                        # res3 conv3 + residual
    assert r50[32 * 64 * 80, 128, 1, 512] == "conv_igemm2_kernel<128, 128, 0, 1>"         # res3 conv1
    assert r50[32 * 128 * 160, 256, 3, 2304] == "conv3x3rb_kernel<256, 128>"              # FPN output / RPN conv on p2
    assert r50[32 * 1000, 1024, 1, 12544] == "conv1x1_ring_kernel"                        # fc1


def test_other_policies_name_the_kernels_the_tests_select_with_them(L):
    hooks = L._lib.test_hooks()
    res4_conv1 = (32 * 32 * 40, 256, 1, 1024)
    long_k = (65536, 256, 1, 4096)
    cases = [
        # policy 9 = 1 | 8, the dispatch before the ring kernel: its shapes go to conv_igemm2, the long-K ones with a full grid to conv_big
        (9, 1, res4_conv1, {}, "conv_igemm2_kernel<128, 128, 0, 1>"),
        (9, 1, (32 * 64 * 80, 512, 1, 128), dict(residual_mode=1), "conv_igemm2_kernel<128, 128, 0, 1>"),
        (9, 1, (32 * 64 * 80, 1024, 1, 512), dict(stride=2, in_pixels=32 * 128 * 160), "conv_igemm2_kernel<128, 128, 0, 1>"),
        (9, 1, long_k, {}, "conv_big_kernel<0>"),
        (9, 1, (32 * 1000, 1024, 1, 12544), {}, "conv_big_kernel<0>"),
        (9, 1, (223 * 256, 256, 1, 4096), {}, "conv_igemm2_kernel<128, 128, 0, 1>"),
        (L.DEFAULT_CONV_POLICY, 1, long_k, {}, "conv1x1_ring_kernel"),
        # policy 25 = 9 | 16: conv_big wherever it applies (fp16 out, whole 256-channel tiles, >= 224 tiles), 3x3 included
        (25, 1, (65536, 256, 1, 64), {}, "conv_big_kernel<0>"),
        (25, 1, (65536, 256, 3, 2304), {}, "conv_big_kernel<1>"),
        (25, 1, (65536, 512, 1, 128), dict(residual_mode=1), "conv_big_kernel<0>"),
        (25, 1, (65536, 128, 1, 64), {}, "conv_igemm2_kernel<128, 128, 0, 1>"),
        (25, 1, (223 * 256, 256, 3, 2304), {}, "conv3x3rb_kernel<128, 128>"),
        (25, 1, (65536, 256, 1, 64), dict(out_f32=True), "conv_igemm2_kernel<128, 128, 0, 1>"),
        (25, 1, (65536, 256, 1, 64), dict(cout_store=248), "conv_igemm2_kernel<128, 128, 0, 1>"),
        # reuse3x3 = 0: the per-tap 3x3 kernel
        (L.DEFAULT_CONV_POLICY, 0, (65536, 256, 3, 2304), {}, "conv_igemm2_kernel<128, 128, 1, 1>"),
        (L.DEFAULT_CONV_POLICY, 0, (65536, 64, 3, 576), {}, "conv_igemm2_kernel<128, 64, 1, 1>"),
        (25, 0, (65536, 256, 3, 2304), {}, "conv_big_kernel<1>"),
        # the tile and pipeline bits of the generic 1x1 kernel (512 tiles of 256 x 128 from 256 * 256 pixels at Cout 256), and bit 0 off
        (2, 1, (256 * 256, 256, 1, 64), {}, "conv_igemm2_kernel<256, 128, 0, 1>"),
        (2, 1, (256 * 256 - 256, 256, 1, 64), {}, "conv_igemm2_kernel<128, 128, 0, 1>"),
        (4, 1, (256 * 256, 256, 1, 64), {}, "conv_igemm2_kernel<128, 128, 0, 2>"),
        (6, 1, (256 * 256, 256, 1, 64), {}, "conv_igemm2_kernel<256, 128, 0, 2>"),
        (6, 1, (256 * 256, 64, 1, 64), {}, "conv_igemm2_kernel<128, 64, 0, 1>"),
        (0, 1, (256 * 256, 256, 3, 2304), {}, "conv3x3rb_kernel<128, 128>"),
        (1, 1, (256 * 256, 256, 3, 2304), {}, "conv3x3rb_kernel<256, 128>"),
        # bit 5 alone: the ring kernel for K >= 1024, Cout == 256, no residual, stride 1 only; bit 6 without bit 8: not with a residual
        (32, 1, res4_conv1, {}, "conv1x1_ring_kernel"),
        (32, 1, (32 * 32 * 40, 512, 1, 1024), {}, "conv_igemm2_kernel<128, 128, 0, 1>"),
        (32, 1, (32 * 32 * 40, 256, 1, 512), {}, "conv_igemm2_kernel<128, 128, 0, 1>"),
        (64, 1, (32 * 64 * 80, 512, 1, 128), dict(residual_mode=1), "conv_igemm2_kernel<128, 128, 0, 1>"),
        (64 | 256, 1, (32 * 64 * 80, 512, 1, 128), dict(residual_mode=1), "conv1x1_ring_kernel"),
        (64 | 256, 1, (32 * 64 * 80, 512, 1, 64), dict(residual_mode=1), "conv_igemm2_kernel<128, 128, 0, 1>"),
        (64, 1, res4_conv1, dict(has_bias=False), "conv_igemm2_kernel<128, 128, 0, 1>"),
        (0, 1, (1000, 64, 7, 4), dict(stride=2), "conv_igemm_kernel<128, 64, 2>"),
    ]
    try:
        for policy, reuse, (M, cout, kernel, K), kw, want in cases:
            hooks.pe_test_set_conv_policy(policy, reuse)
            assert hooks.pe_test_get_conv_policy() == policy
            assert L.conv_variant_name(M, cout, kernel, K, **kw) == want, (policy, reuse, M, cout, kernel, K, kw)
    finally:
        hooks.pe_test_set_conv_policy(L.DEFAULT_CONV_POLICY, 1)
    assert hooks.pe_test_get_conv_policy() == L.DEFAULT_CONV_POLICY


def test_a_fresh_library_starts_with_the_default_policy(L):
    code = "import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).pe_test_get_conv_policy())"
    out = subprocess.run([sys.executable, "-c", code, L._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert int(out) == L.DEFAULT_CONV_POLICY


def test_pair_rule_of_the_library_is_the_python_rule_it_replaces(L):
    lib = L._lib.lib()
    assert lib.pe_conv1x1_pair_supported.argtypes[3] is ctypes.c_int64
    edge = 2 ** 31 // (512 * 2)      # pixels at which the 512-channel tensors reach 2 GiB
    channels = [(128, 512, 128), (256, 1024, 256), (64, 256, 64), (128, 512, 256), (128, 256, 128), (64, 512, 128), (512, 2048, 512)]
    for (cin, cout, cnext), pixels in itertools.product(channels, (1, 15, 64, 32 * 100 * 128, edge - 1, edge, edge + 1, 2 ** 31 // (256 * 2), 2 ** 33)):
        want = (cin, cout, cnext) == (128, 512, 128) and pixels * cout * 2 < 2 ** 31
        assert L.conv1x1_pair_supported(cin, cout, cnext, pixels) is want, (cin, cout, cnext, pixels)
        assert bool(lib.pe_conv1x1_pair_supported(cin, cout, cnext, pixels)) is want
