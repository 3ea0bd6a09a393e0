"""csrc/roi_align.hip against the oracle where a random test does not look (tests/roi_cases.py has the builders,
tests/test_roi_align_edges_cpu.py shows on the CPU that every family tells a wrong rule from the right one).

Exact family: every weight, product and partial sum is exact in float32, so the fp32 tap form, the fp16 per-lane table form, the
fp16 wave-uniform form and the tap fallback inside the table kernels must all equal the oracle BIT FOR BIT (fp16: the oracle's
float32 output cast to float16) - through layers.roi_align_nhwc in both input forms, both processing orders and every channel count
that takes another launch shape, and through layers.ROIAlign on a 3-channel NCHW half input.  Levels: the float32 level rule at
its seams, in both forward forms, both orders and the backward kernel.  Random family: fp32 bit for bit, fp16 within a derived
bound.  Backward: bit for bit where the sample count is a power of two."""
import functools

import numpy as np
import pytest
import torch

import roi_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import proben_amd  # noqa: F401
    from proben_amd import layers
    return layers


@pytest.fixture(scope="module")
def hooks():
    from proben_amd import _lib
    return _lib.test_hooks()


def cu(a, half=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.half() if half else t).cuda()


@functools.lru_cache(maxsize=None)
def expectation(name):
    """The oracle on the case's 256-channel maps, once: every narrower channel count is a slice of it."""
    case = C.exact_cases()[name]
    return C.oracle(case, C.features(case, 256))


def first_difference(what, case, rows, got, want):
    """got, want: [len(rows), ph, pw, C] of the same dtype; raises naming the first differing (roi, bin, channel), both bit
    patterns and the box."""
    view = np.uint16 if got.dtype == np.float16 else np.uint32
    g, w = np.ascontiguousarray(got).view(view), np.ascontiguousarray(want).view(view)
    if np.array_equal(g, w):
        return
    i, ph, pw, c = (int(v) for v in np.argwhere(g != w)[0])
    r = int(rows[i])
    tags = [t for t, v in case.tags.items() if r in v]
    raise AssertionError(f"{what}, {case.name}: {int((g != w).sum())} of {g.size} elements differ; first at roi {r} {tags} bin ({ph}, {pw}) "
                         f"channel {c}: got {float(got[i, ph, pw, c])!r} ({int(g[i, ph, pw, c]):#x}), want {float(want[i, ph, pw, c])!r} "
                         f"({int(w[i, ph, pw, c]):#x}); box {case.boxes.reshape(-1, 4)[r].tolist()}")


def same_levels(what, case, rows, got, want):
    use = ~case.zero[rows]        # a negative area has no level
    assert np.array_equal(got[use], want[rows][use]), f"{what}, {case.name}: levels {got[use].tolist()} != {want[rows][use].tolist()}"


def forward_boxes(L, case, feats, sort):
    out, lv = L.roi_align_nhwc(feats, cu(case.boxes), scales=case.scales, pooled=case.pooled, sampling_ratio=case.ratio, aligned=case.aligned,
                               counts=cu(case.counts), per_image=case.boxes.shape[1], want_levels=True, sort=sort)
    return out.cpu().numpy(), lv.cpu().numpy()


def forward_rois5(L, case, feats):
    r5, rows = C.rois5(case)
    out, lv = L.roi_align_nhwc(feats, cu(r5), scales=case.scales, pooled=case.pooled, sampling_ratio=case.ratio, aligned=case.aligned,
                               want_levels=True)
    return out.cpu().numpy(), lv.cpu().numpy(), rows


def check_fp16(what, case, rows, got, want32, feats32):
    """Exact rows: the oracle's float32 cast to float16, bit for bit.  Rows that are not exact (bin 2.125): the derived bound."""
    ex = case.exact[rows]
    first_difference(what, case, rows[ex], got[ex], want32[rows][ex].astype(np.float16))
    if not ex.all():
        ref, _, A, terms = C.ref64(case, feats32, with_abs=True)
        err = np.abs(got[~ex].astype(np.float64) - ref[rows][~ex])
        bound = C.fp16_bound(ref, A, terms)[rows][~ex]
        assert (err <= bound).all(), f"{what}, {case.name}: error / bound up to {float((err / bound).max()):.3f} on the rows that are not exact"


# ------------------------------------------------------------------------------------------------ exact family, forward
@pytest.mark.parametrize("name", list(C.exact_cases()))
def test_exact_family_fp32_is_the_oracle_bit_for_bit(L, name):
    """fp32 features, C = 4 and 8: the tap form in the reference's order of operations - every row, the ones that are not exact too."""
    case = C.exact_cases()[name]
    want, lv = expectation(name)
    every = np.arange(len(lv))
    for ch in (4, 8):
        feats = [cu(f) for f in C.features(case, ch)]
        for sort in (False, True):
            got, gl = forward_boxes(L, case, feats, sort)
            first_difference(f"fp32 C={ch} sort={sort}", case, every, got, want[..., :ch])
            same_levels(f"fp32 C={ch} sort={sort}", case, every, gl, lv)
        got, gl, rows = forward_rois5(L, case, feats)
        first_difference(f"fp32 C={ch} rois5", case, rows, got, want[rows][..., :ch])
        same_levels(f"fp32 C={ch} rois5", case, rows, gl, lv)


@pytest.mark.parametrize("name", list(C.exact_cases()))
def test_exact_family_fp16_is_the_oracle_bit_for_bit(L, hooks, name):
    """fp16 features at C = 256 (wave-uniform form and, with the hook off, the per-lane form), 64, 16 and 8 - 8 at any pooled size and
    16 with pooled (7, 3) have fewer threads per pooled row than table slots: the block-size rule of roi_align_forward."""
    case = C.exact_cases()[name]
    want, lv = expectation(name)
    every = np.arange(len(lv))
    try:
        for ch in (256, 64, 16, 8):
            f32 = C.features(case, ch)
            feats = [cu(f, half=True) for f in f32]
            for fast in ((1, 0) if ch == 256 else (1,)):
                hooks.pe_test_set_roi_fast(fast)
                for sort in (False, True):
                    what = f"fp16 C={ch} fast={fast} sort={sort}"
                    got, gl = forward_boxes(L, case, feats, sort)
                    check_fp16(what, case, every, got, want[..., :ch], f32)
                    same_levels(what, case, every, gl, lv)
                got, gl, rows = forward_rois5(L, case, feats)
                check_fp16(f"fp16 C={ch} fast={fast} rois5", case, rows, got, want[..., :ch], f32)
                same_levels(f"fp16 C={ch} fast={fast} rois5", case, rows, gl, lv)
    finally:
        hooks.pe_test_set_roi_fast(1)


@pytest.mark.parametrize("name", [n for n, c in C.exact_cases().items() if len(c.scales) == 1])
def test_exact_family_through_the_module_on_three_half_channels(L, name):
    """layers.ROIAlign pads a 3-channel NCHW half input to C = 8: 8 * pooled_w / 8 threads per row for pooled_h + pooled_w slots."""
    case = C.exact_cases()[name]
    want, lv = expectation(name)
    r5, rows = C.rois5(case)
    (f32,) = C.features(case, 3)
    x = cu(f32, half=True).permute(0, 3, 1, 2).contiguous()
    out = L.ROIAlign(case.pooled, case.scales[0], case.ratio, aligned=case.aligned)(x, cu(r5))
    assert out.dtype == torch.float16 and tuple(out.shape) == (len(rows), 3) + case.pooled
    got = out.permute(0, 2, 3, 1).contiguous().cpu().numpy()
    check_fp16("ROIAlign module, 3 half channels", case, rows, got, want[..., :3], [f32])


# ------------------------------------------------------------------------------------------------ levels
def test_levels_at_the_seams_forward(L, hooks):
    """want_levels is the oracle's float32 level on every kept seam case (and the far, tiny and whole-image boxes), -1 on dead
    rows: fp16 C = 256 in both forms and both orders, fp32, and the [R, 5] form."""
    case = C.level_case()
    lv = C.case_levels(case)
    every = np.arange(len(lv))
    try:
        for ch, half in ((256, True), (4, False)):
            feats = [torch.zeros((case.N, h, w, ch), dtype=torch.float16 if half else torch.float32, device="cuda") for h, w in case.hw]
            for fast in ((1, 0) if half else (1,)):
                hooks.pe_test_set_roi_fast(fast)
                for sort in (False, True):
                    _, gl = forward_boxes(L, case, feats, sort)
                    bad = np.nonzero(gl != lv)[0]
                    assert not len(bad), (f"C={ch} fast={fast} sort={sort}: row {bad[0]} box {case.boxes.reshape(-1, 4)[bad[0]].tolist()} "
                                          f"got level {gl[bad[0]]}, want {lv[bad[0]]}; {len(bad)} rows differ")
                _, gl, rows = forward_rois5(L, case, feats)
                assert np.array_equal(gl, lv[rows])
    finally:
        hooks.pe_test_set_roi_fast(1)


@pytest.mark.parametrize("half", [False, True])
def test_levels_at_the_seams_backward(L, half):
    """The backward kernel repeats the level rule in its own code: every box is given an image of its own, so its gradient must
    land on its own image at the oracle's level, and every other level of that image must stay zero."""
    case = C.level_case()
    lv = C.case_levels(case)
    rows = np.nonzero(lv >= 0)[0]
    R, ch = len(rows), 8 if half else 4
    r5 = np.concatenate([np.arange(R, dtype=np.float32)[:, None], case.boxes.reshape(-1, 4)[rows]], axis=1)
    g = torch.ones((R,) + case.pooled + (ch,), dtype=torch.float16 if half else torch.float32, device="cuda")
    grads = L.roi_align_backward_nhwc(g, cu(r5), [(R, h, w, ch) for h, w in case.hw], scales=case.scales, sampling_ratio=case.ratio,
                                      aligned=case.aligned)
    hit = torch.stack([gr.abs().flatten(1).sum(1) > 0 for gr in grads], dim=1).cpu().numpy()      # [R, 4]
    want = np.arange(4)[None, :] == lv[rows][:, None]
    bad = np.nonzero((hit != want).any(axis=1))[0]
    assert not len(bad), (f"box {r5[bad[0], 1:].tolist()}: gradient on levels {np.nonzero(hit[bad[0]])[0].tolist()}, want level "
                          f"{lv[rows][bad[0]]}; {len(bad)} boxes differ")


# ------------------------------------------------------------------------------------------------ random family
@pytest.mark.parametrize("cfg", C.RANDOM_CONFIGS)
def test_random_family_fp32_is_the_oracle_bit_for_bit(L, cfg):
    case = C.random_case(*cfg)
    f32 = C.features(case, 4)
    want, lv = C.oracle(case, f32)
    every = np.arange(len(lv))
    feats = [cu(f) for f in f32]
    for sort in (False, True):
        got, gl = forward_boxes(L, case, feats, sort)
        first_difference(f"fp32 sort={sort}", case, every, got, want)
        assert np.array_equal(gl, lv)
    got, gl, rows = forward_rois5(L, case, feats)
    first_difference("fp32 rois5", case, rows, got, want[rows])


@pytest.mark.parametrize("cfg", C.RANDOM_CONFIGS)
def test_random_family_fp16_is_within_the_derived_bound(L, hooks, cfg):
    """Reference: the oracle's float32 coordinates and weights on the fp16 features, accumulated in float64; A the same sum over
    |w * f|.  Per element |got - ref| <= 2^-11 |ref| + 2^-25 + (npx + grid_h + grid_w + 4) * 2^-24 * A / count: the fp16 store, and
    a first-order bound for the float32 table sums, products, fused accumulation and division (roi_cases.fp16_bound).  Derived,
    not tuned.  Largest error / bound observed on the MI355X, per configuration (printed by the test): C = 256 from 0.9926
    (1 x 1) to 0.9976 (14 x 14), the wave-uniform and the per-lane form equal in every printed digit; C = 64 0.9783 to 0.9970;
    C = 8 0.9513 to 0.9970.  Close to 1 is what the store's term gives by itself: 2^-11 |ref| is exactly half an fp16 ulp where
    |ref| sits just above a power of two, and among 10^5 to 10^7 elements some do."""
    case = C.random_case(*cfg)
    f16 = [f.astype(np.float16) for f in C.features(case, 256)]
    f32 = [f.astype(np.float32) for f in f16]
    ref, lv, A, terms = C.ref64(case, f32, with_abs=True)
    bound = C.fp16_bound(ref, A, terms)
    feats = [cu(f) for f in f16]
    worst = {}
    try:
        for ch, fast in ((256, 1), (256, 0), (64, 1), (8, 1)):
            hooks.pe_test_set_roi_fast(fast)
            got, gl = forward_boxes(L, case, [f[..., :ch].contiguous() for f in feats], fast == 1)
            assert np.array_equal(gl, lv)
            assert np.isfinite(got).all()
            ratio = np.abs(got.astype(np.float64) - ref[..., :ch]) / bound[..., :ch]
            worst[(ch, fast)] = float(ratio.max())
    finally:
        hooks.pe_test_set_roi_fast(1)
    print(f"fp16 error / bound, {case.name}: " + ", ".join(f"C={c} fast={f}: {v:.4f}" for (c, f), v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("name", list(C.backward_cases()))
def test_backward_is_the_oracle_bit_for_bit_on_power_of_two_counts(L, name):
    """Exact family, sample counts 1, 2, 4, ..: every g * w / count is exact and no order of the atomic adds can show.  fp32 and
    fp16 grad_output, one level and four, dead rows and rows without samples (they carry a gradient and must pass on nothing),
    the validity-edge and clamp rows, pooled (7, 7) and (2, 4); boxes form with counts and the [R, 5] form."""
    case = C.backward_cases()[name]
    P = case.boxes.shape[1]
    for half, ch in ((False, 4), (True, 8)):
        grad, ok = C.backward_grad(case, ch)
        want = C.oracle_backward(case, grad)
        assert sum(float(np.abs(w).sum()) for w in want) > 0
        shapes = [(case.N, h, w, ch) for h, w in case.hw]
        g = cu(grad, half=half)
        kw = dict(scales=case.scales, sampling_ratio=case.ratio, aligned=case.aligned)
        got = L.roi_align_backward_nhwc(g, cu(case.boxes), shapes, counts=cu(case.counts), per_image=P, **kw)
        r5, rows = C.rois5(case)
        got5 = L.roi_align_backward_nhwc(g[torch.from_numpy(rows).cuda()], cu(r5), shapes, **kw)
        for form, res in (("boxes", got), ("rois5", got5)):
            for l, (a, w) in enumerate(zip(res, want)):
                a = a.cpu().numpy()
                bad = np.argwhere(C.f32_bits(a) != C.f32_bits(w))
                assert not len(bad), (f"{name} {'fp16' if half else 'fp32'} grad, {form}, level {l}: {len(bad)} elements differ; first at "
                                      f"(image, y, x, channel) {bad[0].tolist()}: got {a[tuple(bad[0])]!r} ({int(C.f32_bits(a)[tuple(bad[0])]):#x}), "
                                      f"want {w[tuple(bad[0])]!r} ({int(C.f32_bits(w)[tuple(bad[0])]):#x})")
