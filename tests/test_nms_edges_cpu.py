"""tests/nms_cases.py and oracle/nms.py on the CPU: the oracle's order of non-finite scores is torch's, every case builder
contains what it claims to contain, and every family keeps something else under a deliberately wrong rule than under the right
one - so tests/test_nms_edges_gpu.py, which compares csrc/nms.hip with the oracle index for index, can tell the two apart."""
import numpy as np
import pytest
import torch

import nms_cases as C
from oracle import nms as O


def keep_sets(case, rule):
    return [set(k.tolist()) for k in C.expected(case, rule, all_survivors=True)]


def right_sets(name):
    case = C.get(name)
    if case.max_out >= case.scores.shape[1]:
        return [set(k.tolist()) for k in C.want(name)]
    return keep_sets(case, C.RIGHT)


# ------------------------------------------------------------------------------------------------ the order rule
def score_sets():
    sp = C.special_scores()
    g = np.random.default_rng(3)
    yield "specials", sp
    yield "specials reversed", sp[::-1].copy()
    yield "nan only", C.bits_f32(C.NAN_BITS * 3)
    yield "zeros", np.asarray([0.0, -0.0, -0.0, 0.0, 1e-45, -1e-45, 0.0], dtype=np.float32)
    for k in range(4):
        s = g.standard_normal(200).astype(np.float32)
        s[g.permutation(200)[:60]] = sp[g.integers(0, len(sp), 60)]
        s[g.permutation(200)[:40]] = np.float32(0.25)                  # finite ties too
        yield f"mixed {k}", s
    for name in C.names("nonfinite_scores"):
        yield name, C.get(name).scores[0]


@pytest.mark.parametrize("name,scores", list(score_sets()), ids=[n for n, _ in score_sets()])
def test_order_desc_stable_is_torchs_stable_descending_sort(name, scores):
    want = torch.sort(torch.from_numpy(np.array(scores)), descending=True, stable=True).indices.numpy()
    got = O.order_desc_stable(scores)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, want)
    nan = np.isnan(scores)
    k = int(nan.sum())
    np.testing.assert_array_equal(got[:k], np.nonzero(nan)[0])        # every NaN first, whatever its bits, in index order
    if k and k < len(scores) and len(set(C.f32_bits(scores[nan]).tolist())) > 1 and np.isinf(scores).any():
        assert not np.array_equal(C.order_under(scores, C.NAN_LAST), want)
        assert not np.array_equal(C.order_under(scores, C.NAN_BY_SIGN), want)


def test_wrong_order_rules_are_what_they_say():
    s = np.concatenate([C.bits_f32(C.NAN_BITS), np.asarray([np.inf, 1.0, 1.0, -0.0, 0.0, -np.inf], dtype=np.float32)])
    np.testing.assert_array_equal(C.order_under(s, C.RIGHT), [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
    np.testing.assert_array_equal(C.order_under(s, C.NAN_LAST), [4, 5, 6, 7, 8, 9, 0, 1, 2, 3])
    np.testing.assert_array_equal(C.order_under(s, C.NAN_BY_SIGN), [2, 0, 4, 5, 6, 7, 8, 9, 1, 3])
    np.testing.assert_array_equal(C.order_under(s, C.TIE_HIGH), [3, 2, 1, 0, 4, 6, 5, 8, 7, 9])


@pytest.mark.parametrize("name", C.names("threshold", "threshold_wide", "degenerate", "nonfinite_scores", "nonfinite_boxes", "dead_rows"))
def test_the_restated_call_under_the_right_rule_is_the_oracle(name):
    """nms_under / batched_under carry the wrong rules; with every switch off they must be the oracle itself."""
    case = C.get(name)
    for b, want in enumerate(C.want(name)):
        live = C.live_rows(case, b)
        got = C.batched_under(case.boxes[b][live], case.scores[b][live], C.class_ids(case, b)[live], case.thr, case.mode, C.RIGHT,
                              restate=True)
        np.testing.assert_array_equal(live[got][:case.max_out], want)


# ------------------------------------------------------------------------------------------------ threshold
def test_threshold_family_has_the_classes_it_is_there_for():
    """(a) fl(p/q) == thr, which a >= would suppress; (b) the exact rational comparison, (c) p * fl(1/q) > thr decide otherwise
    than fl(p/q) > thr.  (a) at every threshold; (b) and (c) where the threshold has them: float32(0.7) < 7/10, so every
    p/q = 7/10 is above the threshold exactly and on it in float32, while 0.5 is exact and float32(0.3), float32(1/3) lie above 3/10
    and 1/3.
    (d) p > fl(thr * q) has NO member with q <= 4096 at these four thresholds, and the test says so instead of looking away: a
    p/q that is not exactly the decimal threshold is at least 1/(10 * 4096) away from it, so only the pairs of class (a) are
    within 2 ulp; they are not suppressed, and fl(thr * q) with thr = float32(t) (1 + e), |e| <= 1.7e-8 < 2^-25, rounds to
    t q = p exactly, so p > fl(thr * q) is false as well."""
    total = {c: 0 for c in "abcd"}
    for t, thr in C.THRESHOLDS.items():
        fam = C.threshold_pairs(t)
        n = {c: sum(c in cls for _, _, cls in fam) for c in "abcd"}
        assert n["a"] > 100, (t, n)
        above = float(thr) < {"0.5": 0.5, "0.7": 0.7, "0.3": 0.3, "third": 1 / 3}[t]
        assert (n["b"] > 100) == above, (t, n)
        for p, q, cls in fam:
            quot = np.float32(p) / np.float32(q)
            assert 1 <= p < q <= C.QMAX and abs(int(quot.view(np.int32)) - int(thr.view(np.int32))) <= 2
            assert ("a" in cls) == (quot == thr)
        for c in "abcd":
            total[c] += n[c]
    assert total["a"] and total["b"] and total["c"], total
    assert total["d"] == 0, total
    for t in C.WIDE:                      # so class (d) has a family of its own, at widths where it exists
        wide = C.threshold_pairs_wide(t)
        assert len(wide) == C.WIDE_PAIRS and all("d" in cls and 2 * q < 2 ** 24 and 1 <= p < q for p, q, cls in wide)


@pytest.mark.parametrize("name", C.names("threshold_wide"))
def test_wide_threshold_case_is_exact_and_has_class_d(name):
    case = C.get(name)
    b, s = case.boxes[0], case.scores[0]
    assert (b == np.round(b)).all() and b.min() >= 0 and len(np.unique(s)) == len(s) and not case.idxs.any() and case.mode == 1
    w = (b[:, 2] - b[:, 0]).astype(np.float64)
    assert ((b[:, 3] - b[:, 1]) == 1).all() and 2 * w.max() < 2 ** 24
    (right,) = right_sets(name)
    assert len(right) == case.claims["n_keep"] and 0 < len(right) < len(s)
    assert case.claims["classes"]["d"] == case.claims["wrong_d"] == C.WIDE_PAIRS
    (f64,) = keep_sets(case, C.F64)
    assert len(right ^ f64) == case.claims["classes"]["b"]


@pytest.mark.parametrize("name", C.names("threshold"))
def test_threshold_case_is_exact_and_tells_wrong_compares_apart(name):
    case = C.get(name)
    b, s, idx = case.boxes[0], case.scores[0], case.idxs[0]
    assert (b == np.round(b)).all() and b.min() >= 0
    assert b.max() + idx.max() * (b.max() + 1) < 2 ** 24                 # shifted coordinates are exact integers
    assert float((b[:, 2] - b[:, 0]).max() * (b[:, 3] - b[:, 1]).max()) * 2 < 2 ** 24
    assert len(np.unique(s)) == len(s)
    assert (case.mode == 0) == (len(np.unique(idx)) == 80) and b.size <= 20000   # batched_nms takes the trick form for it
    (right,) = right_sets(name)
    assert len(right) == case.claims["n_keep"]                             # only the controls suppress
    assert case.claims["controls"] > 20
    (ge,) = keep_sets(case, C.GE)
    assert len(right - ge) == case.claims["classes"]["a"]                 # >= loses one row of every family pair
    (f64,) = keep_sets(case, C.F64)
    assert len(right - f64) == case.claims["classes"]["b"]                # float64 sees 7/10 above float32(0.7)


# ------------------------------------------------------------------------------------------------ degenerate
@pytest.mark.parametrize("name", C.names("degenerate"))
def test_degenerate_case(name):
    case = C.get(name)
    (right,) = right_sets(name)
    assert len(right) == case.claims["n_keep"]
    b, s = case.boxes[0], case.scores[0]
    kept = np.asarray(sorted(right))
    tied = [r for r in range(len(s)) if b[r, 0] % 1000 == 10 and b[r, 1] == 10]
    assert len(tied) == 21 and sum(r in right for r in tied) == 7
    for j in range(7):                                                      # the lowest row of three tied duplicates
        grp = [r for r in tied if b[r, 0] // 1000 == j]
        assert min(grp) in right
    zero_area = (b[:, 0] == b[:, 2]) | (b[:, 1] == b[:, 3])
    assert zero_area.sum() == 7 * 6 and zero_area[kept].sum() == 7 * 6       # 0 / 0 and 0 / area suppress nothing
    inverted = b[:, 2] < b[:, 0]
    assert inverted.sum() == 7 * 4 and inverted[kept].sum() == 7 * 4
    (tie_high,) = keep_sets(case, C.TIE_HIGH)
    assert tie_high != right and len(tie_high) == len(right)
    (plus_one,) = keep_sets(case, C.PLUS_ONE)
    assert len(plus_one) < len(right)                                        # with "+ 1" stacked points have area 1 and IoU 1


# ------------------------------------------------------------------------------------------------ non-finite scores
@pytest.mark.parametrize("name", C.names("nonfinite_scores"))
def test_nonfinite_score_case(name):
    case = C.get(name)
    s, cl = case.scores[0], case.claims["cluster"]
    (right,) = right_sets(name)
    assert len(right) == case.claims["n_keep"] == len(np.unique(cl))          # one survivor per cluster
    order = O.order_desc_stable(s)
    rank = np.empty(len(s), dtype=np.int64)
    rank[order] = np.arange(len(s))
    for c in np.unique(cl):
        rows = np.nonzero(cl == c)[0]
        assert rows[np.argmin(rank[rows])] in right
    bits = set(C.f32_bits(s).tolist())
    want_bits = {0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001}
    if name != "scores_row0_inf":
        want_bits |= set(C.NAN_BITS)
        assert case.claims["bits"] == sorted(C.NAN_BITS)
        (nan_last,) = keep_sets(case, C.NAN_LAST)
        assert len(right ^ nan_last) >= 8
        (by_sign,) = keep_sets(case, C.NAN_BY_SIGN)
        assert len(right ^ by_sign) >= 4
    else:
        assert not np.isnan(s).any()
    assert want_bits <= bits
    (tie_high,) = keep_sets(case, C.TIE_HIGH)
    assert tie_high != right                                                   # -0 / +0 and NaN / NaN ties inside clusters
    if case.claims["presorted"]:
        idx = case.idxs[0].astype(np.int64)
        key = idx * len(s) + rank                                             # (class, place in the order): strictly increasing
        assert C.n_pad_of(len(s)) >= 1024 and (np.diff(key) > 0).all()
        assert idx[0] == 0 and (np.isnan(s[0]) if name == "scores_row0_nan" else s[0] == np.inf)


# ------------------------------------------------------------------------------------------------ non-finite boxes
@pytest.mark.parametrize("name", C.names("nonfinite_boxes"))
def test_nonfinite_box_case(name):
    case = C.get(name)
    val = case.claims["value"]
    for b in range(case.scores.shape[0]):
        bad = np.asarray(case.claims["bad"][b] if case.scores.shape[0] > 1 else case.claims["bad"])
        live = C.live_rows(case, b)
        bx = case.boxes[b]
        assert len(bad) >= 20
        fin = np.isfinite(bx).all(1)
        np.testing.assert_array_equal(np.nonzero(~fin)[0], bad)
        assert {"pinf": np.isposinf, "ninf": np.isneginf, "nan": np.isnan}[val](bx[bad]).sum() == len(bad)
        assert {int(np.nonzero(~np.isfinite(r))[0][0]) for r in bx[bad]} == {0, 1, 2, 3}
        live_bad = np.intersect1d(bad, live)
        assert len(live_bad) >= 10 and len(np.setdiff1d(live, bad)) > 100
        got = set(C.want(name)[b].tolist())
        collapses = case.mode == 0 and val in ("pinf", "nan")
        if collapses:                      # the trick's maximum is NaN / +Inf: every shifted box is NaN, every row survives
            assert got == set(live.tolist())
        else:                              # the bad rows stay, suppress nothing, and the rest is the NMS of the finite rows
            rest = np.setdiff1d(live, bad)
            with np.errstate(all="ignore"):
                k = C.batched_under(bx[rest], case.scores[b][rest], C.class_ids(case, b)[rest], case.thr, 1, C.RIGHT)
            assert got == set(rest[k].tolist()) | set(live_bad.tolist())
            assert len(got) < len(live)
        if case.scores.shape[0] == 1 and case.claims.get("clusters"):
            assert len(got) > case.claims["clusters"]                      # the runner-up of a cluster whose best row went bad


@pytest.mark.parametrize("name", C.names("dead_rows"))
def test_dead_row_case(name):
    case = C.get(name)
    zeroed = C.zero_dead_rows(case)
    for b in range(2):
        live, dead = C.live_rows(case, b), case.claims["dead"][b]
        assert not np.intersect1d(live, dead).size and len(live) + len(dead) == case.scores.shape[1]
        assert np.isfinite(case.boxes[b][live]).all() and case.boxes[b][live].min() >= 0 and np.isfinite(case.scores[b][live]).all()
        d = case.boxes[b][dead]
        assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d == -5).any() and (d == np.float32(1e30)).any()
        assert np.isnan(case.scores[b][dead]).sum() == 4
        assert (zeroed.boxes[b][dead] == 0).all() and np.array_equal(zeroed.boxes[b][live], case.boxes[b][live])
        np.testing.assert_array_equal(C.expected(zeroed)[b], C.want(name)[b])
        # a dead row that did take part would show: the call over all rows keeps something else
        everything = case._replace(counts=None, valid=None)
        assert not np.array_equal(C.expected(everything)[b], C.want(name)[b])
    assert len(C.want(name)[0]) == 70


# ------------------------------------------------------------------------------------------------ seams
def test_seam_sizes_and_layouts_are_the_ones_the_kernels_switch_at():
    sizes = {C.SEAMS[k]["n"] for k in C.SEAMS}
    assert sizes == {1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2049, 16076, 16077, 16128, 16129, 16384}
    outs = {C.SEAMS[k].get("max_out") for k in C.SEAMS}
    assert {1, 63, 64, 65, None} <= outs
    # csrc/nms.hip, pe_nms_batched: merge by rank while kept lists + flags + one key per row + 2 x 512 fit in 160 KiB
    def merge(n):
        lists = (((n * 2 + 15) & ~15) + C.n_pad_of(n) // 8 + 15) & ~15
        return lists + n * 8 + 1024 <= 160 * 1024
    assert merge(16076) and not merge(16077)
    assert C.n_pad_of(1023) == 1024 and C.n_pad_of(1025) == 2048 and C.n_pad_of(16384) == 16384


@pytest.mark.parametrize("name", C.names("seams"))
def test_seam_case(name):
    case = C.get(name)
    B, n = case.scores.shape
    key = name[len("seam_"):]
    if key in C.SEAMS:
        spec = C.SEAMS[key]
        assert n == spec["n"] and case.claims["nseg"] == (len(spec["runs"]) if "runs" in spec else min(spec["segs"], n))
        if "runs" in spec:
            assert case.claims["runs"] == sorted(spec["runs"]) and {64, 1} & set(spec["runs"])
        if case.claims["presorted"]:
            idx, s = case.idxs[0].astype(np.int64), case.scores[0]
            assert (np.diff(idx) >= 0).all() and (np.diff(s)[np.diff(idx) == 0] < 0).all()
        if case.claims["truncates"] and n <= 4096:
            (all_kept,) = C.expected(case, all_survivors=True)
            assert len(all_kept) > case.max_out and len(C.want(name)[0]) == case.max_out
        elif n > 1:
            assert 0 < len(C.want(name)[0]) < n                           # something is suppressed, something survives
    elif key == "disjoint2100":
        (got,) = C.want(name)
        assert len(got) == 2100 > 1024 and case.max_out == n and len(np.unique(case.idxs)) == 1
        assert not set(got.tolist()) & set(case.claims["copies"].tolist())
        # every "late" copy has exactly one box it overlaps, and that box stands past place 1024 of the kept list
        place = {r: i for i, r in enumerate(got.tolist())}
        for r in case.claims["late"]:
            same = np.nonzero((case.boxes[0] == case.boxes[0][r]).all(1))[0]
            orig = [x for x in same if x in place]
            assert len(orig) == 1 and place[orig[0]] >= 1024
    else:
        assert B == 3 and C.n_pad_of(n) >= 1024 and len(C.live_rows(case, 1)) == 0 and len(C.want(name)[1]) == 0
        assert (case.counts is not None and case.counts[1] == 0) or (case.valid is not None and not case.valid[1].any())
        for b in (0, 2):
            assert len(C.want(name)[b]) == case.max_out < len(C.expected(case, all_survivors=True)[b])


@pytest.mark.parametrize("n", C.SCRATCH_N)
def test_scratch_case(n):
    case = C.get(f"scratch_n{n}")
    assert case.scores.shape == (3, n) and case.counts.tolist() == [n, n // 2, 1]
    assert [len(k) for k in C.want(f"scratch_n{n}")][2] == 1
