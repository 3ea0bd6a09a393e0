"""Every convolution kernel bit for bit against a float64 host reference, on operands whose answer does not depend on the
summation order, and with non-finite values located pixel by pixel (tests/conv_exact.py has the generator, the references, the
footprints and the comparator; tests/test_conv_exact_cpu.py shows that the comparator rejects the errors this module is after).

Operands are integers times powers of two, so every partial sum is an integer times the product grid and exact in fp32 while the
sum of the absolute terms stays under the bit budget.  Budget used: 2^20 grid steps (four bits under fp32's 24); the plainest case
(the generic LDS-DMA 1x1 on one tile) was bit-exact at it, so it was not lowered; the cases need between 2^15.1 and 2^19.1.
An fp16 output is then ONE round-to-nearest-even of the exact value (7 % - 56 % of the values at a rounding point are inexact in fp16 and thousands
are exact ties, asserted per case), an fp32 output is the value itself, and a fused chain is rounded in the reference where the
kernel rounds.  Comparison: NaN masks equal, every other element the same bits.  Output buffers are pre-filled with NaN wherever
the API takes out=, so an element the kernel never writes shows."""
import pytest
import torch

import conv_exact as E

pytestmark = pytest.mark.gpu

NAN, INF = E.NAN, E.INF


@pytest.fixture(scope="module")
def L():
    import proben_amd  # noqa: F401
    from proben_amd import layers
    return layers


@pytest.fixture(scope="module")
def hooks():
    from proben_amd import _lib
    return _lib.test_hooks()


def cu(t, dtype=torch.float16):
    return None if t is None else t.to(dtype).cuda().contiguous()


def nan_buf(shape, dtype=torch.float16):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ which kernel takes a launch
def dispatch_name(L, c):
    """Kernel that pe_conv2d_nhwc_f16 picks for the case under ITS policy (conv2_dispatch in csrc/conv_igemm2.hip); under the default
    policy the 1x1 answer is layers.conv_variant_name's."""
    Ho, Wo = c.out_hw
    M = c.N * Ho * Wo
    policy = L.DEFAULT_CONV_POLICY if c.policy < 0 else c.policy
    store = 15 if c.f32out else 0
    if c.k == 7 or (c.k == 1 and c.policy < 0):
        return L.conv_variant_name(M, c.Cout, c.k, c.Cin, stride=c.stride, residual_mode=c.res_mode, out_f32=c.f32out,
                                   cout_store=store, out_stride=16 if c.f32out else 0, in_pixels=c.N * c.H * c.W)
    assert not policy & 96 or c.k == 3, "the ring kernel's rule is conv_variant_name's"
    bn = 64 if c.Cout <= 64 else 128
    if policy & 8 and not c.f32out and c.Cout % 256 == 0 and -(-M // 256) * (c.Cout // 256) >= 224 and (policy & 16 or (c.k == 1 and c.Cin >= 4096)):
        return f"conv_big_kernel<{int(c.k == 3)}>"
    if c.k == 3 and c.reuse:
        big = policy & 1 and -(-M // 256) * -(-c.Cout // 128) >= 512
        name = "conv3x3rb_kernel<128, 64>" if bn == 64 else f"conv3x3rb_kernel<{256 if big else 128}, 128>"
        assert c.policy >= 0 or name == L.conv_variant_name(M, c.Cout, 3)
        return name
    if c.k == 3:
        return f"conv_igemm2_kernel<128, {bn}, 1, 1>"
    big1 = policy & 2 and -(-M // 256) * -(-c.Cout // 128) >= 512
    return f"conv_igemm2_kernel<{256 if big1 else 128}, {bn}, 0, {2 if policy & 4 else 1}>"


# ------------------------------------------------------------------------------------------------ runners
def run_conv(L, hooks, c, ops, ring_wgs=256):
    """The case's kernel on the (float64, grid) operands -> the output tensor on the host, in the layout of conv_exact.conv_expected."""
    x, w, b, res = cu(ops["x"]), cu(ops["w"]), cu(ops["b"], torch.float32), cu(ops["res"])
    Ho, Wo = c.out_hw
    if c.api in ("wd", "wd9"):
        assert L.conv_wd_supported(3, 1, c.H, c.W, c.Cin, c.Cout)
        packed = L.conv_wd_pack(w)
        try:
            hooks.pe_test_set_wd9_mode(2 if c.api == "wd9" else 0)
            assert hooks.pe_test_wd9_takes(c.N, c.H, c.W, c.Cin, c.Cout) == int(c.api == "wd9")
            if c.window:
                off, stride = c.window
                full = nan_buf((c.N, c.H, c.W, stride))
                L.conv3x3_wd(x, packed, b, c.Cout, relu=c.relu, out=full.view(-1)[off:], out_stride=stride)
                assert bool(torch.isnan(full[..., :off]).all()) and bool(torch.isnan(full[..., off + c.Cout:]).all())    # the rest of the window is untouched
                out = full[..., off:off + c.Cout]
            else:
                out = nan_buf((c.N, c.H, c.W, c.Cout))
                L.conv3x3_wd(x, packed, b, c.Cout, relu=c.relu, out=out)
            torch.cuda.synchronize()
        finally:
            hooks.pe_test_set_wd9_mode(-1)
        return out.cpu()
    if c.api == "stem_pool":
        wp = torch.zeros((64, 7, 8, 4), dtype=torch.float16, device="cuda")
        wp[:, :, 1:, :c.Cin] = w
        return L.stem_conv_pool(x, wp, b).cpu()
    if c.api == "stem":
        wp = torch.zeros((64, 8, 8, 4), dtype=torch.float16, device="cuda")
        wp[:, :7, :7, :c.Cin] = w
        assert dispatch_name(L, c) == c.variant
        out = nan_buf((c.N, Ho, Wo, 64))
        L.conv2d_nhwc(x, wp, b, kernel=7, stride=2, relu=c.relu, out=out)
        return out.cpu()
    try:
        hooks.pe_test_set_conv_policy(L.DEFAULT_CONV_POLICY if c.policy < 0 else c.policy, c.reuse)
        hooks.pe_test_set_ring_wgs(ring_wgs)
        assert dispatch_name(L, c) == c.variant, (dispatch_name(L, c), c.variant)
        if c.api == "linear":
            out = L.linear_f16(x.view(c.N, c.Cin), w.view(c.Cout, c.Cin), b, relu=c.relu).view(c.N, 1, 1, c.Cout)
        elif c.f32out:
            full = nan_buf((c.N, Ho, Wo, 16), torch.float32)
            L.conv2d_nhwc(x, w, b, kernel=c.k, stride=c.stride, relu=c.relu, out_f32=True, cout=c.Cout, cout_store=c.Cout, out_stride=16, out=full)
            assert bool(torch.isnan(full[..., c.Cout:]).all())                    # 15 of 16 columns: the pad column is not written
            out = full[..., :c.Cout]
        else:
            out = nan_buf((c.N, Ho, Wo, c.Cout))
            L.conv2d_nhwc(x, w, b, kernel=c.k, stride=c.stride, relu=c.relu, residual=res, residual_mode=c.res_mode, out=out)
        torch.cuda.synchronize()
    finally:
        hooks.pe_test_set_ring_wgs(256)
        hooks.pe_test_set_conv_policy(L.DEFAULT_CONV_POLICY, 1)
    return out.cpu().contiguous()


def run_chain(L, hooks, c, o):
    x, w, b = cu(o["x"]), cu(o["w"]), cu(o["b"], torch.float32)
    shape = (c.N, c.H, c.W)
    if c.kind == "head":
        pk, ph = L.conv_wd_pack(w), L.conv_wd_pack_head(cu(o["w2"]))
        b16 = torch.zeros(16, device="cuda")
        b16[:15] = cu(o["b2"], torch.float32)
        out = nan_buf(shape + (16,), torch.float32)
        try:
            hooks.pe_test_set_wd9_mode(2 | 8 if c.gen == "wd9" else 0)
            assert hooks.pe_test_wd9_head_takes(c.N, c.H, c.W) == int(c.gen == "wd9")
            L.conv3x3_wd_rpn_head(x, pk, b, ph, b16, out=out)
            torch.cuda.synchronize()
        finally:
            hooks.pe_test_set_wd9_mode(-1)
        return {"out": out[..., :15].cpu().contiguous(), "pad": out[..., 15].cpu()}
    if c.kind == "tail":
        out = nan_buf(shape + (c.Cout,))
        L.bottleneck_tail_wd(x, L.conv_wd_pack(w), b, L.conv_wd_pack_tail(cu(o["w2"])), cu(o["b2"], torch.float32), cu(o["res"]), c.Cout, out=out)
        return {"out": out.cpu()}
    packed = L.bneck64_pack(w, cu(o["w2"]), cu(o["wsc"]) if c.sc else None, cu(o["w3"]) if c.nxt else None)
    out, nxt = nan_buf(shape + (256,)), (nan_buf(shape + (64,)) if c.nxt else None)
    L.bneck64(x, cu(o["src"]), packed, b, cu(o["b2"], torch.float32), cu(o["bsc"], torch.float32) if c.sc else None,
              cu(o["b3"], torch.float32) if c.nxt else None, out=out, t1_next=nxt)
    got = {"out": out.cpu()}
    if c.nxt:
        got["t1_next"] = nxt.cpu()
    return got


def assert_chain(got, want, what):
    for key in ("out", "t1_next"):
        if key in want:
            E.assert_bits(got[key], want[key], f"{what}.{key}")


ids = lambda cases: [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ 1. exact operands
@pytest.mark.parametrize("c", E.CONV_CASES, ids=ids(E.CONV_CASES))
def test_conv_is_bit_exact_on_grid_operands(L, hooks, c):
    """The kernel's fp32 accumulator must BE the float64 sum, whatever its K order, tile walk or cross-wave reduction, and its
    fp16 output one round-to-nearest-even of it.  The ring kernel walks the same pixels to the same bits with 8 workgroups."""
    E.conv_conditions(c)
    ops, want = E.conv_clean(c)
    for wgs in ((256, 8) if c.variant == E.RING else (256,)):
        E.assert_bits(run_conv(L, hooks, c, ops, ring_wgs=wgs), want, f"{c.name} ({wgs} workgroups)")


@pytest.mark.parametrize("c", E.CHAIN_CASES, ids=ids(E.CHAIN_CASES))
def test_fused_chain_is_bit_exact_on_grid_operands(L, hooks, c):
    """The fused RPN head (fp32 out), the bottleneck tail and bneck64 (t1_next from the REFERENCE's block output): every stage is
    exact, so the fp16 roundings of the intermediates are deterministic and the whole chain is bit-comparable."""
    E.chain_conditions(c)
    o, want = E.chain_clean(c)
    got = run_chain(L, hooks, c, o)
    assert_chain(got, want, c.name)
    if c.kind == "head":
        assert float(got["pad"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2. non-finite values
def conv_mask(c, pixels):
    m = E.footprint(pixels, c.N, c.H, c.W, c.k, c.stride)
    return E.pool_footprint(m) if c.api == "stem_pool" else m


def bad_expected(c, ops_bad, clean, foot):
    """Expected output on operands that differ from the clean ones inside the receptive fields of `foot` only."""
    if not c.heavy:
        return E.conv_expected(c, ops_bad)
    want = clean.clone()
    pix = torch.nonzero(foot)
    want[foot] = E.conv_finish(c, E.conv_exact(c, ops_bad, at=pix))
    return want


@pytest.mark.parametrize("c", E.CONV_CASES, ids=ids(E.CONV_CASES))
def test_conv_nan_pixel_poisons_exactly_its_receptive_field(L, hooks, c):
    """A NaN in input channel 0 at corners, row ends, image seams, both sides of every tile edge and an interior pixel: the output
    is NaN in ALL channels exactly on the footprint computed from geometry (window, stride, pool), and every other element keeps
    the clean reference's bits - a halo tap silenced by a multiply, a row or image seam read through, or a neighbour column from
    the wrong row each change that set."""
    ops, clean = E.conv_clean(c)
    for pixels in E.plant_sets(c.N, c.H, c.W, c.k, c.stride):
        bad = dict(ops, x=E.plant(ops["x"], pixels, NAN))
        foot = E.footprint(pixels, c.N, c.H, c.W, c.k, c.stride)
        mask = conv_mask(c, pixels)[..., None].expand(clean.shape)
        want = bad_expected(c, bad, clean, foot)
        assert torch.equal(torch.isnan(want), mask), "the float64 reference disagrees with the geometric footprint"
        got = run_conv(L, hooks, c, bad)
        assert torch.equal(torch.isnan(got), mask), f"{c.name}: NaN set differs from the footprint at {int((torch.isnan(got) != mask).sum())} elements, planted {pixels}"
        E.assert_bits(torch.where(mask, clean, got), clean, f"{c.name} outside the footprint, planted {pixels}")


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus_inf", "minus_inf"])
@pytest.mark.parametrize("c", E.CONV_CASES, ids=ids(E.CONV_CASES))
def test_conv_inf_pixel_gives_signed_inf_or_nan_by_the_weight(L, hooks, c, sign):
    """One infinite term per receptive field: sign(w) * inf, NaN where that weight is zero (channels 0, 1, 2 have a zero, a positive
    and a negative weight on the planted channel), then ReLU: -inf -> 0, +inf and NaN stay."""
    ops, clean = E.conv_clean(c)
    for pixels in E.plant_sets(c.N, c.H, c.W, c.k, c.stride):
        bad = dict(ops, x=E.plant(ops["x"], pixels, sign * INF))
        foot = E.footprint(pixels, c.N, c.H, c.W, c.k, c.stride)
        mask = conv_mask(c, pixels)[..., None].expand(clean.shape)
        want = bad_expected(c, bad, clean, foot)
        assert not bool((~torch.isfinite(want) & ~mask).any())
        if foot.any():
            assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
        E.assert_bits(run_conv(L, hooks, c, bad), want, f"{c.name} {sign:+.0f}inf planted {pixels}")


@pytest.mark.parametrize("c", E.CONV_CASES, ids=ids(E.CONV_CASES))
def test_conv_nan_bias_poisons_exactly_its_channel(L, hooks, c):
    ops, clean = E.conv_clean(c)
    ch = 5
    b = ops["b"].clone()
    b[ch] = NAN
    want = clean.clone()
    want[..., ch] = NAN
    E.assert_bits(run_conv(L, hooks, c, dict(ops, b=b)), want, c.name)


RES_CASES = [c for c in E.CONV_CASES if c.res_mode]


@pytest.mark.parametrize("c", RES_CASES, ids=ids(RES_CASES))
def test_conv_nan_residual_element_poisons_its_element_or_its_2x2_block(L, hooks, c):
    """Mode 1: exactly that output element; mode 2: exactly its nearest-2x block, clipped on odd sizes; that channel only."""
    ops, clean = E.conv_clean(c)
    Ho, Wo = c.out_hw
    res = ops["res"].clone()
    rh, rw = res.shape[1], res.shape[2]
    want = clean.clone()
    for n, h, w, ch in [(0, 0, 0, 5), (c.N - 1, rh - 1, rw - 1, 7), (0, rh // 2, rw // 3, c.Cout - 1)]:
        res[n, h, w, ch] = NAN
        if c.res_mode == 1:
            want[n, h, w, ch] = NAN
        else:
            want[n, 2 * h:min(2 * h + 2, Ho), 2 * w:min(2 * w + 2, Wo), ch] = NAN
    if c.res_mode == 2 and Ho % 2:
        assert int(torch.isnan(want[c.N - 1, :, :, 7]).sum()) < 4                   # the last block is clipped
    if not c.heavy:
        assert torch.equal(torch.isnan(E.conv_expected(c, dict(ops, res=res))), torch.isnan(want))
    E.assert_bits(run_conv(L, hooks, c, dict(ops, res=res)), want, c.name)


@pytest.mark.parametrize("c", E.CONV_CASES, ids=ids(E.CONV_CASES))
def test_conv_fp16_overflow_is_one_rounding_of_the_fp32_sum(L, hooks, c):
    """Finite operands, a copy channel whose exact accumulator the test controls (conv_exact.with_overflow): 65519.875 rounds to
    65504, 65520 (the tie) to +inf; with a residual, 70000 - 10000 is a finite 60000 because the add is in fp32 in front of the
    one rounding."""
    ops, clean = E.conv_clean(c)
    pixels = E.plant_sets(c.N, c.H, c.W, c.k, c.stride)[0]
    over = E.with_overflow(c, ops, pixels)
    ch = E.COPY_CH
    one = dict(over, w=over["w"][ch:ch + 1], b=over["b"][ch:ch + 1], res=None if over["res"] is None else over["res"][..., ch:ch + 1])
    exact = E.conv_exact(c, one)
    assert bool((exact.float().double() == exact).all())                          # b + x (+ res): exact in fp32
    if c.heavy:
        foot = E.footprint(pixels, c.N, c.H, c.W, c.k, c.stride)
        want = bad_expected(c, over, clean, foot)
        want[..., ch] = E.conv_finish(c, exact)[..., 0]
    else:
        want = E.conv_expected(c, over)
    col = want[..., ch]
    if c.f32out:
        assert float(col.max()) == 65520.0
    elif c.res_mode:
        assert bool(torch.isfinite(col).all()) and float(col.max()) == 60000.0
    else:
        assert bool(torch.isposinf(col).any()) and bool((col == 65504.0).any())
    E.assert_bits(run_conv(L, hooks, c, over), want, c.name)


def chain_perturbations(c, o):
    """(name, operands, pixels whose 3x3 footprint must be NaN in every output channel | None)"""
    sets = E.plant_sets(c.N, c.H, c.W, 3, 1)
    for i, pixels in enumerate(sets):
        yield f"nan{i}", dict(o, x=E.plant(o["x"], pixels, NAN)), pixels
    yield "plus_inf", dict(o, x=E.plant(o["x"], sets[0], INF)), None
    yield "minus_inf", dict(o, x=E.plant(o["x"], sets[-1], -INF)), None
    b2 = o["b2"].clone()
    b2[5] = NAN
    yield "nan_bias2", dict(o, b2=b2), None
    b = o["b"].clone()
    b[7] = NAN
    yield "nan_bias1", dict(o, b=b), None
    for key in ("res", "src"):
        if o.get(key) is not None:
            r = o[key].clone()
            r[c.N - 1, c.H - 1, c.W - 1, 9] = NAN
            r[0, 0, 1, 3] = NAN
            yield f"nan_{key}", {**o, key: r}, None
    yield "overflow", E.chain_with_overflow(c, o, sets[0]), None


@pytest.mark.parametrize("c", E.CHAIN_CASES, ids=ids(E.CHAIN_CASES))
def test_fused_chain_carries_non_finite_values_like_the_reference(L, hooks, c):
    """NaN / +-Inf pixels (the first stage's footprint spreads through the second stage to ALL its outputs at those pixels), NaN in
    either bias, NaN in a residual / shortcut element, and an fp16 intermediate that overflows to +inf on finite operands."""
    o, clean = E.chain_clean(c)
    for name, bad, pixels in chain_perturbations(c, o):
        want = E.chain_expected(c, bad)
        if pixels is not None:
            for key in ("out", "t1_next"):
                if key in want:
                    mask = E.footprint(pixels, c.N, c.H, c.W, 3, 1)[..., None].expand(want[key].shape)
                    assert torch.equal(torch.isnan(want[key]), mask)
                    assert torch.equal(torch.where(mask, clean[key], want[key]), clean[key])
        if name == "overflow":
            assert bool(torch.isposinf(want["t"][..., E.COPY_CH]).any()) and bool((want["t"][..., E.COPY_CH] == 65504.0).any())
        assert_chain(run_chain(L, hooks, c, bad), want, f"{c.name} {name}")


@pytest.mark.parametrize("shape", [(2, 9, 13, 16), (1, 12, 8, 64)])
def test_pools_propagate_nan_and_keep_minus_inf_windows(L, shape):
    """maxpool3x3s2_nhwc and subsample2_nhwc: NaN propagates like torch.max_pool2d, with the footprint from geometry; a window
    that holds only -inf stays -inf."""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(H * W)
    x = E.ints(g, shape, 512) / 8.0
    x[0, :5, :5] = -INF
    x[N - 1, H - 4:, W - 4:, 1] = -INF
    clean = E.maxpool_ref(x).half()
    assert bool(torch.isneginf(clean[0, 0, 0]).all()) and bool(torch.isneginf(clean[0, 1, 1]).all())
    E.assert_bits(L.maxpool3x3s2_nhwc(cu(x)).cpu(), clean, "maxpool, clean")
    for pixels in E.plant_sets(N, H, W, 3, 2):
        bad = E.plant(x, pixels, NAN, channel=2)
        marked = torch.zeros((N, H, W), dtype=torch.bool)
        for n, h, w in pixels:
            marked[n, h, w] = True
        want = E.maxpool_ref(bad).half()
        mask = torch.zeros(want.shape, dtype=torch.bool)
        mask[..., 2] = E.pool_footprint(marked)
        assert torch.equal(torch.isnan(want), mask)
        got = L.maxpool3x3s2_nhwc(cu(bad)).cpu()
        E.assert_bits(got, want, f"maxpool, planted {pixels}")
        E.assert_bits(torch.where(mask, clean, got), clean, "maxpool outside the footprint")
        E.assert_bits(L.subsample2_nhwc(cu(bad)).cpu(), bad[:, ::2, ::2].contiguous().half(), f"subsample, planted {pixels}")
