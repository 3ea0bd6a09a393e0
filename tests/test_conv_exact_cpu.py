"""tests/conv_exact.py on the host: the generator's own conditions on every operand set tests/test_conv_exact_gpu.py uses (bit
budget, share of fp16-inexact values, exact ties, planted-pixel spacing, a zero / positive / negative weight under a planted Inf),
the float64 reference against torch and against the geometric footprints, and - the point of the module - mutants of the reference
that the bit comparator has to reject: the errors a 4e-3 tolerance lets through."""
import pytest
import torch

import conv_exact as E

NAN, INF = E.NAN, E.INF
ids = lambda cases: [c.name for c in cases]
LIGHT = [c for c in E.CONV_CASES if not c.heavy and c.api not in ("stem", "stem_pool", "linear")]
LIGHT = list({E._shape_key(c): c for c in LIGHT}.values())            # one case per operand set
LIGHT_3X3 = [c for c in LIGHT if c.k == 3]
LIGHT_F16 = [c for c in LIGHT if not c.f32out]


# ------------------------------------------------------------------------------------------------ the generator's conditions
@pytest.mark.parametrize("c", E.CONV_CASES, ids=ids(E.CONV_CASES))
def test_conv_operands_meet_budget_inexact_share_and_ties(c):
    (st,) = E.conv_conditions(c)
    assert st["log2_budget_used"] < 20
    ops, want = E.conv_clean(c)
    for t, dt in ((ops["x"], torch.float16), (ops["w"], torch.float16), (ops["res"], torch.float16), (ops["b"], torch.float32)):
        assert t is None or bool((t.to(dt).double() == t).all()), "operand not representable in the kernel's input type"
    assert bool(torch.isfinite(want).all())
    w0 = ops["w"][list(E.SIGN_ROWS)][..., 0]
    assert bool((w0[0] == 0).all()) and bool((w0[1] > 0).all()) and bool((w0[2] < 0).all())      # what an Inf in channel 0 meets
    assert float((ops["w"] == 0).double().mean()) > 0.2


@pytest.mark.parametrize("c", E.CHAIN_CASES, ids=ids(E.CHAIN_CASES))
def test_chain_operands_meet_the_conditions_at_every_rounding_point(c):
    stats = E.chain_conditions(c)
    assert [s["name"].split(".")[1] for s in stats] == {"head": ["t", "head"], "tail": ["t", "out"]}.get(c.kind, ["t", "out"] + ["t1_next"] * c.nxt)
    o, want = E.chain_clean(c)
    for key in ("x", "w", "w2", "w3", "src", "wsc", "res"):
        if o.get(key) is not None:
            assert bool((o[key].half().double() == o[key]).all()), key
    assert all(bool(torch.isfinite(v).all()) for v in want.values())


def test_budget_assertion_is_a_condition_not_a_measurement():
    c = E.by_name["ig128_k2048"]
    ops, _ = E.conv_clean(c)
    exact = E.conv_exact(c, ops)
    with pytest.raises(AssertionError, match="budget"):
        E.check_point("x", exact, exact.abs() + E.BUDGET * ops["grid"], ops["grid"])
    with pytest.raises(AssertionError, match="off the grid"):
        E.check_point("x", exact + ops["grid"] / 2, exact.abs() + 1, ops["grid"])
    with pytest.raises(AssertionError, match="inexact"):
        E.check_point("x", (exact / ops["grid"] / 64).round().clamp(-7, 7), exact.abs(), 1.0)


@pytest.mark.parametrize("c", E.CONV_CASES + E.CHAIN_CASES, ids=ids(E.CONV_CASES + E.CHAIN_CASES))
def test_planted_pixels_are_apart_and_cover_the_edges(c):
    sets = E.plant_sets(c.N, c.H, c.W, c.k, c.stride)
    d = max(3, c.k)
    assert all(E.min_spacing(s) >= d for s in sets)
    allp = {p for s in sets for p in s}
    assert len(allp) == sum(len(s) for s in sets)
    for n in (0, c.N - 1):
        assert {(n, 0, 0), (n, 0, c.W - 1), (n, c.H - 1, 0), (n, c.H - 1, c.W - 1)} <= allp
    assert {(0, c.H // 2, 0), (0, c.H // 2, c.W - 1), (0, c.H // 2, c.W // 2)} <= allp
    if c.N > 1:
        assert {(0, c.H - 1, c.W - 1), (1, 0, 0)} <= allp
    Ho, Wo = E.out_hw(c.H, c.W, c.k, c.stride)
    M = c.N * Ho * Wo
    hit = set()
    for p in allp:
        m = E.footprint([p], c.N, c.H, c.W, 1, c.stride)
        hit |= set(torch.nonzero(m.view(-1)).view(-1).tolist())
    assert {m for m in E.TILE_EDGES + (M - 1,) if m < M} <= hit          # both sides of every tile edge, and the last pixel


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("c", LIGHT + [E.by_name["stem_c3"], E.by_name["stem_c4"]], ids=lambda c: c.name)
def test_reference_is_torch_conv2d_in_float64_and_in_float32(c):
    """The per-tap float64 reference equals torch's float64 convolution - and torch's fp32 convolution in its own summation order,
    which is the whole point of the grid."""
    ops, _ = E.conv_clean(c)
    x = ops["x"][..., :c.Cin].permute(0, 3, 1, 2)
    w = ops["w"].permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(x, w, ops["b"], stride=c.stride, padding=c.k // 2).permute(0, 2, 3, 1)
    mine = E.conv_ref(ops["x"], ops["w"], ops["b"], c.stride)
    assert torch.equal(mine, ref)
    ref32 = torch.nn.functional.conv2d(x.float(), w.float(), ops["b"].float(), stride=c.stride, padding=c.k // 2).permute(0, 2, 3, 1)
    assert torch.equal(ref32.double(), mine)


@pytest.mark.parametrize("value", [NAN, INF, -INF])
@pytest.mark.parametrize("c", LIGHT, ids=ids(LIGHT))
def test_reference_agrees_with_the_geometric_footprint(c, value):
    """NaN mask of the float64 reference == the dilated planted mask (strides 1 and 2, 1x1 and 3x3); the footprint-only reference
    (used for the one large shape) equals the full one; an Inf gives NaN / +inf / -inf by the weight's sign."""
    ops, clean = E.conv_clean(c)
    for pixels in E.plant_sets(c.N, c.H, c.W, c.k, c.stride):
        bad = dict(ops, x=E.plant(ops["x"], pixels, value))
        foot = E.footprint(pixels, c.N, c.H, c.W, c.k, c.stride)
        want = E.conv_expected(c, bad)
        assert torch.equal((~torch.isfinite(want)).any(-1), foot)
        if value != value:
            assert torch.equal(torch.isnan(want), foot[..., None].expand(want.shape))
        else:
            z, p, n = (want[foot][:, r] for r in E.SIGN_ROWS)
            s = 1.0 if value > 0 else -1.0
            assert bool(torch.isnan(z).all())
            assert bool((p == (s * INF if not (c.relu and s < 0) else 0.0)).all())
            assert bool((n == (-s * INF if not (c.relu and s > 0) else 0.0)).all())
        E.assert_bits(torch.where(foot[..., None], clean, want), clean)
        part = E.conv_finish(c, E.conv_exact(c, bad, at=torch.nonzero(foot)))
        E.assert_bits(part, want[foot])


def test_pool_footprint_is_max_pool2d_of_the_mask():
    g = torch.Generator().manual_seed(1)
    for shape in [(2, 9, 11), (1, 18, 22), (1, 4, 4)]:
        m = torch.rand(shape, generator=g) < 0.05
        ref = torch.nn.functional.max_pool2d(m[:, None].float(), 3, 2, 1)[:, 0] > 0
        assert torch.equal(E.pool_footprint(m), ref)


def test_overflow_operands_hit_65504_the_tie_and_60000():
    c = E.by_name["rb64"]
    ops, _ = E.conv_clean(c)
    pixels = E.plant_sets(c.N, c.H, c.W, 3, 1)[0]
    want = E.conv_expected(c, E.with_overflow(c, ops, pixels))[..., E.COPY_CH]
    for i, (n, h, w) in enumerate(pixels):
        assert float(want[n, h, w]) == (INF if i % 2 == 0 else 65504.0)
    c = E.by_name["ig64_res1"]
    ops, _ = E.conv_clean(c)
    pixels = E.plant_sets(c.N, c.H, c.W, 1, 1)[0]
    over = E.with_overflow(c, ops, pixels)
    want = E.conv_expected(c, over)[..., E.COPY_CH]
    assert bool(torch.isfinite(want).all()) and float(want.max()) == 60000.0
    assert E.rejects(E.mutant_residual_after_rounding(c, over), E.conv_expected(c, over))       # inf - 10000 is inf


# ------------------------------------------------------------------------------------------------ the comparator bites
def test_comparator_accepts_equal_and_rejects_one_bit():
    a = torch.tensor([1.0, -0.0, INF, NAN, 65504.0, 3.0]).half()
    E.assert_bits(a, a.clone())
    for i, v in [(0, 1.0009765625), (1, 0.0), (2, -INF), (2, 65504.0), (3, 0.0), (5, NAN)]:
        b = a.clone()
        b[i] = v
        assert E.rejects(b, a), (i, v)
    with pytest.raises(AssertionError):
        E.assert_bits(a.float(), a)


@pytest.mark.parametrize("c", LIGHT_F16, ids=ids(LIGHT_F16))
def test_mutant_conversion_toward_zero_is_rejected(c):
    ops, want = E.conv_clean(c)
    got = E.mutant_toward_zero(c, ops)
    assert E.rejects(got, want)
    diff = (got.double() - want.double()).abs() / want.double().abs().clamp(min=1e-9)
    assert float(diff.max()) < 1e-3                     # ... and invisible at rtol = 4e-3: at most one fp16 ulp


@pytest.mark.parametrize("c", LIGHT_F16, ids=ids(LIGHT_F16))
def test_mutant_fp16_detour_of_a_partial_sum_is_rejected(c):
    ops, want = E.conv_clean(c)
    assert E.rejects(E.mutant_partial_fp16(c, ops), want)


@pytest.mark.parametrize("c", [c for c in LIGHT_F16 if c.res_mode], ids=lambda c: c.name)
def test_mutant_residual_added_after_the_rounding_is_rejected(c):
    ops, want = E.conv_clean(c)
    assert E.rejects(E.mutant_residual_after_rounding(c, ops), want)


@pytest.mark.parametrize("c", LIGHT_3X3, ids=ids(LIGHT_3X3))
def test_mutant_dropped_tap_at_a_border_pixel_is_rejected(c):
    ops, want = E.conv_clean(c)
    got = E.mutant_dropped_tap(c, ops)
    assert E.rejects(got, want)
    assert int((got != want).any(-1).sum()) == 1         # one pixel


@pytest.mark.parametrize("c", [c for c in LIGHT_F16 if c.relu], ids=lambda c: c.name)
def test_mutant_relu_that_turns_nan_into_zero_is_rejected(c):
    ops, _ = E.conv_clean(c)
    bad = dict(ops, x=E.plant(ops["x"], E.plant_sets(c.N, c.H, c.W, c.k, c.stride)[0], NAN))
    assert E.rejects(E.mutant_relu_drops_nan(c, bad), E.conv_expected(c, bad))
    assert not E.rejects(E.mutant_relu_drops_nan(c, ops), E.conv_expected(c, ops))      # a finite run cannot tell


@pytest.mark.parametrize("c", LIGHT_3X3, ids=ids(LIGHT_3X3))
def test_mutant_halo_silenced_by_a_multiply_is_rejected_only_with_planted_nan(c):
    ops, want = E.conv_clean(c)
    assert not E.rejects(E.mutant_halo_multiplied_by_zero(c, ops), want)                 # 0 * finite: every finite test passes it
    caught = 0
    for value in (NAN, INF):
        for pixels in E.plant_sets(c.N, c.H, c.W, 3, 1):
            bad = dict(ops, x=E.plant(ops["x"], pixels, value))
            caught += E.rejects(E.mutant_halo_multiplied_by_zero(c, bad), E.conv_expected(c, bad))
    assert caught >= 2                                   # the row ends are planted: 0 * NaN and 0 * inf are NaN in the next row


@pytest.mark.parametrize("c", LIGHT_3X3, ids=ids(LIGHT_3X3))
def test_mutant_column_0_tap_from_the_previous_rows_last_pixel_is_rejected(c):
    ops, want = E.conv_clean(c)
    assert E.rejects(E.mutant_seam_read_through(c, ops), want)
    bad = dict(ops, x=E.plant(ops["x"], [(0, c.H // 2, c.W - 1)], NAN))
    assert E.rejects(E.mutant_seam_read_through(c, bad), E.conv_expected(c, bad))        # and the NaN set grows past the footprint


@pytest.mark.parametrize("c", [c for c in E.CHAIN_CASES if c.gen == "wd"], ids=lambda c: c.name)
def test_chain_mutants_are_rejected(c):
    """In a chain: every fp16 rounding converted toward zero is rejected at an output; one NaN pixel is NaN in its 3x3 neighbourhood only."""
    o, want = E.chain_clean(c)
    real = E.to_half
    try:
        E.to_half = E.half_toward_zero
        got = E.chain_expected(c, o)
    finally:
        E.to_half = real
    assert any(E.rejects(got[k], want[k]) for k in want if k != "t")
    bad = E.chain_expected(c, dict(o, x=E.plant(o["x"], [(0, 1, 1)], NAN)))
    assert bool(torch.isnan(bad["out"][0, :3, :3]).all()) and int(torch.isnan(bad["out"]).any(-1).sum()) == 9
