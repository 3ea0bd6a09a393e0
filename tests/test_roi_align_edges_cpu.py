"""tests/roi_cases.py on the CPU: the float64 restatement of the ROIAlign rule equals the oracle (oracle/csrc/roi_align.c, the
restatement of ROIAlign_cpu.cpp) bit for bit on every case of the exact family, every deliberately wrong rule that bears on a
family changes at least one output bit or level in it (a family that cannot tell a wrong rule apart is a failure of the family),
the exact family is exact (the oracle's float32 output is the float64 result rounded once), the oracle's backward is the float64
adjoint where the sample count is a power of two, and the level-seam cases meet the conditions they were built for.
No GPU; tests/test_roi_align_edges_gpu.py runs the same cases through csrc/roi_align.hip."""
import numpy as np
import pytest

import roi_cases as C

CPU_CHANNELS = 8        # a channel slice of the maps the GPU tests use: the rule does not depend on the channel


def bits_equal(a, b):
    return np.array_equal(C.f32_bits(a), C.f32_bits(b))


def rules_for(case):
    """The wrong rules that bear on a case of the exact family."""
    if case.name.startswith("exact_single"):
        rules = ["edge_exclusive", "count_valid", "no_last_clamp"]
        if case.ratio == 0:
            rules.append("grid_floor1")
        if case.aligned:
            rules += ["no_half", "clamp_aligned"]
        return rules
    if case.name.startswith("exact_fpn"):
        return ["count_valid", "no_half"] if case.aligned else ["count_valid"]
    if case.name.startswith("exact_grid_seam"):
        return ["grid_floor1"]
    if case.name.startswith("exact_table_seam"):
        return ["grid_floor1", "no_half", "count_valid"]
    if case.name.startswith("exact_min_size"):
        return ["edge_exclusive", "no_last_clamp"]
    if case.name.startswith("exact_negative"):
        return ["clamp_aligned"]
    raise AssertionError(case.name)


@pytest.mark.parametrize("name", list(C.exact_cases()))
def test_right_rule_equals_oracle_and_wrong_rules_show(name):
    case = C.exact_cases()[name]
    feats = C.features(case, CPU_CHANNELS)
    want, lv = C.oracle(case, feats)
    ref, lv64 = C.ref64(case, feats)
    assert np.array_equal(lv, lv64)
    exact = case.exact
    # exactness: the float64 result, rounded once, is the oracle's float32 output in every bit
    assert bits_equal(ref.astype(np.float32)[exact], want[exact]), name
    assert exact.sum() >= 3
    # rows the oracle refuses (negative size, aligned) and dead rows are zeros in both
    dead = (lv < 0) | case.zero
    assert not want[dead].any() and not ref[dead].any()
    live = ~dead & exact
    assert np.abs(want[live]).sum() > 0
    for rn in rules_for(case):
        wrong, wl = C.ref64(case, feats, C.WRONG_RULES[rn])
        assert not bits_equal(wrong.astype(np.float32)[exact], want[exact]), f"{name}: the wrong rule {rn} changes no bit"


@pytest.mark.parametrize("tag,rule", [("at_minus_one_y", "edge_exclusive"), ("at_minus_one_x", "edge_exclusive"), ("at_size_y", "edge_exclusive"),
                                      ("at_size_x", "edge_exclusive"), ("at_size_y", "no_last_clamp"), ("at_size_x", "no_last_clamp"),
                                      ("in_last_pixel_y", "no_last_clamp"), ("in_last_pixel_x", "no_last_clamp"),
                                      ("corner_tl", "count_valid"), ("corner_br", "count_valid"), ("zero_area", "clamp_aligned")])
def test_named_rows_are_where_their_rule_shows(tag, rule):
    """The named edge rows do what their names say: the wrong rule they were built for changes THAT row (7x7, adaptive, aligned)."""
    case = C.exact_single((7, 7), 0, True)
    feats = C.features(case, CPU_CHANNELS)
    want, _ = C.oracle(case, feats)
    wrong, _ = C.ref64(case, feats, C.WRONG_RULES[rule])
    rows = case.tags[tag]
    assert not bits_equal(wrong.astype(np.float32)[rows], want[rows])


def test_samples_beyond_the_edge_are_dropped_but_counted():
    case = C.exact_single((7, 7), 2, True)
    feats = C.features(case, CPU_CHANNELS)
    want, _ = C.oracle(case, feats)
    for tag in ("below_minus_one_y", "below_minus_one_x", "beyond_size_y", "beyond_size_x"):
        rows = case.tags[tag]
        wrong, _ = C.ref64(case, feats, C.WRONG_RULES["edge_exclusive"])      # nothing sits ON the edge in these rows
        assert bits_equal(wrong.astype(np.float32)[rows], want[rows]), tag
        wrong, _ = C.ref64(case, feats, C.WRONG_RULES["count_valid"])
        assert not bits_equal(wrong.astype(np.float32)[rows], want[rows]), tag


def test_family_contains_what_it_claims():
    cases = C.exact_cases()
    assert {c.pooled for c in cases.values()} >= set(C.POOLED)
    assert {c.ratio for c in cases.values()} == {0, 2, 4}
    single = C.exact_single((7, 7), 0, True)
    for tag in ["at_minus_one", "below_minus_one", "in_minus_one_zero", "at_size", "beyond_size", "in_last_pixel"]:
        assert tag + "_x" in single.tags and tag + "_y" in single.tags
    for tag in ["outside", "half_left", "half_right", "half_top", "half_bottom", "corner_tl", "corner_tr", "corner_bl", "corner_br", "zero_area"]:
        assert tag in single.tags
    # the box wholly outside is zeros, counts leave dead rows on both images
    want, lv = C.oracle(single, C.features(single, CPU_CHANNELS))
    assert not want[single.tags["outside"]].any()
    assert (lv.reshape(2, -1)[:, -1] == -1).all()
    # sample counts 3, 5, 6, 7, 9, 15, 21: the three-instruction division must be correctly rounded there
    counts = set()
    for tag, rows in single.tags.items():
        if tag.startswith("count_"):
            ay, ax = C.roi_axes(single, rows[0], 0)
            assert ay.grid * ax.grid == int(tag[6:])
            counts.add(ay.grid * ax.grid)
    assert counts == {3, 5, 6, 7, 9, 15, 21}
    # grid seam: 2.0 -> grid 2, 2.125 -> grid 3, per axis
    seam = C.exact_grid_seam(True)
    grids = {tag: tuple(a.grid for a in C.roi_axes(seam, rows[0], 0)) for tag, rows in seam.tags.items()}
    assert grids == {"bin_2.0x2.0": (2, 2), "bin_2.0x2.125": (2, 3), "bin_2.125x2.0": (3, 2), "bin_2.125x2.125": (3, 3)}
    # table seam: windows of 20 pixels (table form) and 21 (tap fallback), one axis each way
    tab = C.exact_table_seam()
    win = {tag: tuple(int(a.npx.max()) for a in C.roi_axes(tab, rows[0], 0)) for tag, rows in tab.tags.items()}
    assert win["table_19x19"] == (20, 20) and win["tap_20x20"] == (21, 21) and win["half_pixel_19"] == (20, 20)
    assert win["one_axis_19x20"] == (20, 21) and win["one_axis_20x19"] == (21, 20)
    def largest_side(c):      # in pixels of the level the box is pooled from: what the kernels' loops run over
        lv = C.case_levels(c)
        b = c.boxes.reshape(-1, 4)[lv >= 0]
        sc = np.array(c.scales)[lv[lv >= 0]]
        return float((np.maximum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]) * sc).max())
    assert largest_side(tab) == 140.0 == max(largest_side(c) for c in cases.values())      # the largest box anywhere in the suite
    # four levels: every level used, one image empty
    fpn = C.exact_fpn((7, 7), 0, True)
    assert set(C.case_levels(fpn).tolist()) == {-1, 0, 1, 2, 3} and fpn.counts[1] == 0
    # min-size clamp: both axes
    ms = C.exact_min_size((8, 8))
    ay, ax = C.roi_axes(ms, ms.tags["clamp_both"][0], 0)
    assert ay.grid == 1 and ax.grid == 1 and ay.W.sum() == 8 and ax.W.sum() == 8


def test_rois5_form_is_the_same_work():
    case = C.exact_fpn((7, 7), 0, True)
    r5, rows = C.rois5(case)
    assert len(rows) == int(C.live_mask(case).sum()) and np.array_equal(r5[:, 1:], case.boxes.reshape(-1, 4)[rows])
    b = r5[:, 0]
    assert (np.diff(b) < 0).any() and (np.diff(b) > 0).any()      # unordered batch indices


@pytest.mark.parametrize("name", list(C.backward_cases()))
def test_backward_is_the_float64_adjoint_on_power_of_two_counts(name):
    case = C.backward_cases()[name]
    grad, ok = C.backward_grad(case, CPU_CHANNELS)   # zero where the count is no power of two; dead and empty rows carry a gradient
    nothing = C.pow2_count_rows(case)[1]
    assert ok.sum() >= 2 and nothing.any() and np.abs(grad[nothing]).sum() > 0
    got = C.oracle_backward(case, grad)
    want = C.adjoint64(case, grad)
    assert sum(np.abs(g).sum() for g in got) > 0
    for l, (g, w) in enumerate(zip(got, want)):
        assert bits_equal(g, w.astype(np.float32)), (name, l)
        assert np.array_equal(g.astype(np.float64), w)          # exact, not merely equal after rounding
    # <forward(f), g> == <f, backward(g)>, exactly
    feats = C.features(case, CPU_CHANNELS)
    fwd, _ = C.ref64(case, feats)
    grad = np.where((C.case_levels(case) >= 0)[:, None, None, None], grad, 0)      # dead rows: forward zeros, no gradient
    lhs = float((fwd * grad).sum())
    rhs = float(sum((f.astype(np.float64) * w).sum() for f, w in zip(feats, want)))
    assert lhs == rhs, (lhs, rhs)
    o, _ = C.oracle(case, feats)
    assert float((o.astype(np.float64) * grad).sum()) == rhs


def test_level_seam_cases_meet_their_conditions():
    s = C.level_seams()
    assert s.core.sum() == 156
    assert np.array_equal(C.levels_restated(s.boxes), s.level)           # the step-by-step float32 restatement IS the oracle's rule
    kept = s.kept & s.core
    assert kept.sum() * 4 >= 3 * s.core.sum(), f"{kept.sum()} of {s.core.sum()} seam cases kept"
    print(f"seam cases kept: {kept.sum()} of {s.core.sum()}; with the wider steps {s.kept.sum()} of {len(s.kept)}")
    # every box that was dropped lies below a seam, within the 6 ulps
    assert (s.k[s.core & ~s.kept] < 0).all()
    for j in (-1, 0, 1):
        lv = set(s.level[s.kept & (s.seam == j)].tolist())
        assert lv == {j + 1, j + 2}, f"seam {j}: kept levels {lv}"
    # a kernel that 'improves' the rule's precision must fail: some kept case differs between float32 and float64 arithmetic
    f64 = C.levels_restated(s.boxes, f64=True)
    assert (s.kept & (f64 != s.level)).any()
    one_below = (s.seam == 0) & (s.k == -1) & (s.boxes[:, 3] == 224)
    assert one_below.sum() == 1 and s.kept[one_below][0] and s.level[one_below][0] == 2 and f64[one_below][0] == 1
    # far boxes, tiny boxes (p2) and whole-image boxes (p5)
    assert s.far_level.tolist() == [0, 1, 2, 3, 0, 0, 0, 3, 3, 0]
    assert np.array_equal(C.levels_restated(s.far, -1), s.far_level) and np.array_equal(C.levels_restated(s.far, 1), s.far_level)
    case = C.level_case()
    lv = C.case_levels(case)
    assert (lv.reshape(2, -1)[:, -5:] == -1).all() and set(lv.tolist()) == {-1, 0, 1, 2, 3}
    wl = C.case_levels(case, C.WRONG_RULES["level64"])
    assert (wl != lv).any()


@pytest.mark.parametrize("cfg", C.RANDOM_CONFIGS)
def test_random_family_float64_reference_is_within_its_own_bound_of_the_oracle(cfg):
    """The float64-accumulated reference the fp16 bound is measured from, against the oracle's float32 sums: within the float32
    part of the bound (no fp16 store here), so the bound's reference is the same operation."""
    case = C.random_case(*cfg, n_boxes=40)
    feats = C.features(case, CPU_CHANNELS)
    want, lv = C.oracle(case, feats)
    ref, _, A, terms = C.ref64(case, feats, with_abs=True)
    assert set(lv.tolist()) >= {-1, 0}
    # the oracle sums 4 * grid_h * grid_w products in float32, one after the other
    grids = np.zeros(lv.shape[0])
    for r in np.nonzero(lv >= 0)[0]:
        ay, ax = C.roi_axes(case, r, lv[r])
        grids[r] = 4 * ay.grid * ax.grid
    bound = (grids[:, None, None, None] + 4) * 2.0 ** -24 * A + 2.0 ** -149
    assert (np.abs(want - ref) <= bound).all()
