"""PDQ without a GPU: the argument checks of pe_pdq_pair_quality and pe_pdq_assign, the assignment against SciPy's,
the bootstrap ratio and the paired difference on hand-made records, the label and variance fallbacks of a prediction row, and
tests/pdq_ref.py against hand-worked values of a hard box."""
import ctypes
import math

import numpy as np
import pytest

import pdq_ref as R


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.lib()


def err(L):
    return L.pe_last_error().decode()


P = 4096          # a pointer that is never followed: every check below answers before any device work


def pair_args(**kw):
    """The argument list of pe_pdq_pair_quality with every pointer set and small counts; kw overrides by name."""
    names = ["det_boxes", "det_vars", "det_log_probs", "det_offsets", "gt_boxes", "gt_classes", "gt_crowd", "gt_offsets", "image_hw",
             "pair_offsets", "num_images", "num_classes", "num_dets", "num_gt", "num_pairs", "table", "weights", "tau", "q", "fg", "bg", "label",
             "gt_live", "flags", "stream"]
    a = {n: P for n in names}
    a.update(num_images=1, num_classes=3, num_dets=2, num_gt=2, num_pairs=4, table=160, weights=None, tau=0.0027, stream=None)
    a.update(kw)
    return [a[n] for n in names]


def test_pair_quality_argument_checks(L):
    for name in ("det_boxes", "det_vars", "det_log_probs", "det_offsets", "gt_boxes", "gt_classes", "gt_crowd", "gt_offsets", "image_hw",
                 "pair_offsets", "q", "fg", "bg", "label", "gt_live", "flags"):
        assert L.pe_pdq_pair_quality(*pair_args(**{name: None})) == -1, name
        assert "pe_pdq_pair_quality" in err(L) and "null" in err(L), (name, err(L))
    assert L.pe_pdq_pair_quality(*pair_args(table=4097)) == -1 and "pe_pdq_pair_quality: W + H = 4097 is above 4096" in err(L)
    for tau in (-1e-9, 1.0, 2.0, float("nan")):
        assert L.pe_pdq_pair_quality(*pair_args(tau=tau)) == -1 and "tau" in err(L) and "[0, 1)" in err(L)
    for name in ("num_images", "num_dets", "num_gt", "num_pairs", "table"):
        assert L.pe_pdq_pair_quality(*pair_args(**{name: -1})) == -1 and "pe_pdq_pair_quality" in err(L), name
    assert L.pe_pdq_pair_quality(*pair_args(num_classes=0)) == -1 and "num_classes" in err(L)
    assert L.pe_pdq_pair_quality(*pair_args(num_pairs=5)) == -1 and "num_pairs 5" in err(L)
    assert L.pe_pdq_pair_quality(*pair_args(num_images=0)) == -1 and "without images" in err(L)
    bad = (ctypes.c_float * 4)(10, 10, 0, 5)
    assert L.pe_pdq_pair_quality(*pair_args(weights=bad)) == -1 and "bbox_reg_weights[2]" in err(L)


def call_assign(L, q, live, doff, goff, poff=None, take=None, counts=None):
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    live = np.ascontiguousarray(live, dtype=np.int32)
    d32, g32 = np.ascontiguousarray(doff, dtype=np.int32), np.ascontiguousarray(goff, dtype=np.int32)
    if poff is None:
        poff = np.concatenate([[0], np.cumsum(np.diff(g32).astype(np.int64) * np.diff(d32))])
    poff = np.ascontiguousarray(poff, dtype=np.int64)
    take = None if take is None else np.ascontiguousarray(take, dtype=np.int32)
    B, M, G, n = counts if counts is not None else (len(d32) - 1, int(d32[-1]), int(g32[-1]), int(poff[-1]))
    match = np.full(max(G, 1), -7, dtype=np.int32)
    p = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    st = L.pe_pdq_assign(p(q), p(live), p(take), p(d32), p(g32), p(poff), B, M, G, n, p(match))
    return st, match[:G]


def test_assign_argument_checks(L):
    q, live = np.ones(4), np.ones(2, dtype=np.int32)
    assert call_assign(L, q, live, [0, 2], [0, 2])[0] == 0
    for counts in ((-1, 2, 2, 4), (1, -2, 2, 4), (1, 2, -2, 4), (1, 2, 2, -4)):
        assert call_assign(L, q, live, [0, 2], [0, 2], counts=counts)[0] == -1 and "negative count" in err(L)
    assert call_assign(L, q, live, [0, 2], [0, 2], counts=(0, 2, 2, 4))[0] == -1 and "without images" in err(L)
    for doff, goff in (([0, 2, 1], [0, 1, 2]), ([0, 1, 2], [0, 2, 1])):
        st, _ = call_assign(L, np.ones(8), live, doff, goff, poff=[0, 2, 4], counts=(2, 2, 2, 4))
        assert st == -1 and "not monotone" in err(L)
    assert call_assign(L, q, live, [1, 2], [0, 2], poff=[0, 4], counts=(1, 2, 2, 4))[0] == -1 and "start at 0" in err(L)
    assert call_assign(L, q, live, [0, 2], [0, 2], poff=[0, 3], counts=(1, 2, 2, 3))[0] == -1 and "span 3 pairs" in err(L)
    assert call_assign(L, q, live, [0, 2], [0, 2], counts=(1, 3, 2, 4))[0] == -1 and "offsets end at" in err(L)
    a = lambda x: np.asarray(x).ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    d, g, po, m = np.array([0, 2], np.int32), np.array([0, 2], np.int32), np.array([0, 4], np.int64), np.zeros(2, np.int32)
    for hole in range(7):
        args = [a(q), a(live), None, a(d), a(g), a(po), 1, 2, 2, 4, a(m)]
        if hole == 2:
            continue                                # det_take is optional
        args[hole if hole < 6 else 10] = None
        assert L.pe_pdq_assign(*args) == -1 and "pe_pdq_assign: null pointer" in err(L), hole


def test_assign_against_scipy_on_random_matrices(L):
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(11)
    shapes = [(1, 1), (6, 9), (9, 6)] + [(int(g), int(m)) for g, m in zip(rng.integers(1, 7, 197), rng.integers(1, 10, 197))]
    shapes = [s if i % 2 == 0 else s[::-1] for i, s in enumerate(shapes)]
    assert len(shapes) == 200 and any(g > m for g, m in shapes) and any(g < m for g, m in shapes)
    worst = 0.0
    for G, M in shapes:
        q = rng.uniform(0.0, 1.0, (G, M))
        st, match = call_assign(L, q, np.ones(G), [0, M], [0, G])
        assert st == 0, err(L)
        ri, ci = linear_sum_assignment(q, maximize=True)
        want = math.fsum(q[ri, ci])
        hit = np.nonzero(match >= 0)[0]
        assert len(set(match[hit])) == len(hit) and all(0 <= match[g] < M for g in hit)       # one-to-one, inside the image
        got = math.fsum(q[hit, match[hit]])
        assert len(hit) == len(ri) == min(G, M)
        assert abs(got - want) <= min(G, M) * R.U * want, (G, M, got, want)
        worst = max(worst, abs(got - want) / (min(G, M) * R.U * want))
    print(f"pe_pdq_assign against linear_sum_assignment on 200 matrices: largest difference of the totals {worst:.3f} of its bound")


def test_assign_hand_cases(L):
    st, m = call_assign(L, [[0.9, 0.8], [0.8, 0.1]], [1, 1], [0, 2], [0, 2])          # greedy takes 0.9 and is left with 0.1
    assert st == 0 and m.tolist() == [1, 0]
    st, m = call_assign(L, [[0.0, 0.0], [0.3, 0.7]], [1, 1], [0, 2], [0, 2])          # an all-zero row: no true positive for it
    assert st == 0 and m.tolist() == [-1, 1]
    st, m = call_assign(L, np.zeros((3, 2)), [1, 1, 1], [0, 2], [0, 3])
    assert st == 0 and m.tolist() == [-1, -1, -1]
    st, m = call_assign(L, np.zeros(0), np.zeros(0), [0, 3], [0, 0])                  # G = 0
    assert st == 0 and m.size == 0
    st, m = call_assign(L, np.zeros(0), [1, 1], [0, 0], [0, 2])                       # M = 0
    assert st == 0 and m.tolist() == [-1, -1]
    # a dead ground truth is skipped (its 0.99 is not taken), a detection below the threshold too; two images, flat indices out
    q = np.concatenate([np.array([[0.99, 0.2], [0.5, 0.6]]).ravel(), np.array([[0.4, 0.9, 0.8]]).ravel()])
    st, m = call_assign(L, q, [0, 1, 1], [0, 2, 5], [0, 2, 3], take=[1, 1, 1, 0, 1])
    assert st == 0 and m.tolist() == [-1, 1, 4]
    st, m = call_assign(L, [[float("nan"), 0.5], [0.4, float("nan")]], [1, 1], [0, 2], [0, 2])
    assert st == 0 and m.tolist() == [1, 0]


def test_python_callers_refuse_offsets_that_do_not_rise():
    """pe_pdq_pair_quality's offsets are device memory, which the entry point cannot read before device work: the Python callers check
    them on the host, before anything else (pair_quality before it asks for device tensors)."""
    import torch
    from proben_amd import pdq
    q, live = np.ones(4), np.ones(2, dtype=np.int32)
    assert pdq.assign(q, live, [0, 2], [0, 2]).tolist() in ([0, 1], [1, 0])
    for doff, goff in (([0, 2, 1], [0, 1, 2]), ([0, 1, 2], [0, 2, 1]), ([1, 2], [0, 2]), ([0, 2], [1, 2])):
        with pytest.raises(ValueError, match="do not start at 0 and rise"):
            pdq.assign(q, live, doff, goff)
    with pytest.raises(ValueError, match="offsets of 1 and 2 images"):
        pdq.assign(q, live, [0, 2], [0, 1, 2])
    with pytest.raises(ValueError, match="pair qualities"):
        pdq.assign(np.ones(3), live, [0, 2], [0, 2])
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)      # noqa: E731
    zi = lambda *shape: torch.zeros(shape, dtype=torch.int32)      # noqa: E731
    for doff, goff in (([0, 2, 1], [0, 1, 2]), ([0, 1, 2], [0, 2, 1])):
        with pytest.raises(ValueError, match="do not start at 0 and rise"):
            pdq.pair_quality(z(2, 4), z(2), z(2, 4), doff, z(2, 4), zi(2), zi(2), goff, zi(2, 2))


def records():
    """Hand-made per-image records: sum q, TP, FP, FN, ..."""
    a = np.zeros((4, 8))
    a[:, :4] = [[1.5, 2, 1, 0], [0.5, 1, 0, 2], [0.0, 0, 3, 1], [0.8, 1, 1, 1]]
    b = a.copy()
    b[:, 0] = [1.7, 0.6, 0.0, 0.9]
    return a, b


def test_bootstrap_ratio_and_paired_difference():
    from proben_amd import bootstrap, pdq
    a, b = records()
    mult = np.array([[1, 1, 1, 1], [2, 0, 1, 1], [0, 0, 4, 0], [0, 3, 0, 1]])
    got = pdq.replicate_pdq(a, mult)
    n = a[:, 1] + a[:, 2] + a[:, 3]
    close = lambda x, y: abs(x - y) <= 4 * R.U * abs(y)      # noqa: E731
    assert close(got[0], a[:, 0].sum() / n.sum()) and close(got[0], 2.8 / 13)
    assert close(got[1], (2 * 1.5 + 0.8) / (2 * 3 + 4 + 3)) and got[2] == 0.0 and close(got[3], (3 * 0.5 + 0.8) / (3 * 3 + 3))
    assert np.isnan(pdq.replicate_pdq(np.zeros((2, 8)), np.ones((1, 2))))[0]
    out = pdq.bootstrap_pdq(a, b, replicates=500, seed=3, confidence=0.9)
    mult = bootstrap.resample_multiplicities(4, 500, 3)
    xa, xb = pdq.replicate_pdq(a, mult), pdq.replicate_pdq(b, mult)
    assert out["a"]["point"] == xa[0] and out["b"]["point"] == xb[0]
    ok = ~(np.isnan(xa[1:]) | np.isnan(xb[1:]))
    d = (xb[1:] - xa[1:])[ok]
    assert out["paired"]["point"] == xb[0] - xa[0] > 0
    assert out["paired"]["lo"] == np.quantile(d, 0.05) and out["paired"]["hi"] == np.quantile(d, 0.95)
    assert out["paired"]["lo"] <= out["paired"]["point"] <= out["paired"]["hi"]
    assert out["a"]["lo"] == np.quantile(xa[1:][~np.isnan(xa[1:])], 0.05) and out["a"]["se"] == np.std(xa[1:][~np.isnan(xa[1:])], ddof=1)
    assert out["paired"]["p"] == min(1.0, 2.0 * min(np.mean(d <= 0), np.mean(d >= 0)))     # b >= a on every image: d >= 0 always
    s = pdq.summarise(a)
    assert close(s["pdq"], 2.8 / 13) and close(s["pair_quality"], 2.8 / 4) and (s["tp"], s["fp"], s["fn"]) == (4, 5, 4)
    with pytest.raises(ValueError):
        pdq.bootstrap_pdq(a, b[:3])


def test_label_spread_and_variance_default():
    from proben_amd import pdq
    lp = pdq.label_spread([0.7, 1.0, 0.25], [1, 0, 3], 3)
    np.testing.assert_array_equal(lp[0], np.log([(1 - 0.7) / 3, 0.7, (1 - 0.7) / 3, (1 - 0.7) / 3]))
    np.testing.assert_array_equal(lp[1], [0.0, -np.inf, -np.inf, -np.inf])
    np.testing.assert_array_equal(lp[2], np.log([0.25, 0.25, 0.25, 0.25]))
    assert abs(np.exp(lp[0]).sum() - 1) < 4 * R.U and np.isnan(pdq.label_spread([0.5, 1.5], [4, 0], 3)).all()
    # a fused file of a conventional method: no logits, no probabilities, the schema's placeholder variance -> the spread and a hard box
    pred = {"image": ["a"], "image_id": [1], "boxes": [[[1, 2, 9, 8], [0, 0, 4, 4]]], "scores": [[0.9, 0.6]], "classes": [[2, 0]],
            "class_logits": [[[], []]], "probs": [[[], []]], "vars": [[[1.0], [1.0]]]}
    boxes, var, lp, score = pdq._rows(pred, 0, 1.0, 2.0, 3, "cpu")
    assert var.tolist() == [0.0, 0.0] and score.tolist() == [0.9, 0.6] and boxes.shape == (2, 4)
    np.testing.assert_array_equal(lp, pdq.label_spread([0.9, 0.6], [2, 0], 3))
    del pred["vars"]
    assert pdq._rows(pred, 0, 1.0, 2.0, 3, "cpu")[1].tolist() == [0.0, 0.0]
    # probabilities but no logits: a variance head's output is a variance, scaled
    pred.update(probs=[[[0.05, 0.05, 0.9], [0.6, 0.2, 0.1]]], vars=[[[0.5], [2.0]]])
    assert pdq._rows(pred, 0, 1.0, 2.0, 3, "cpu")[1].tolist() == [1.0, 4.0]
    assert pdq.infer_num_classes(pred) == 3 and pdq.infer_num_classes({"class_logits": [[[]]], "probs": [[[]]]}) is None


def image(H, W, dets, gts, K=3):
    """dets: (box, var, class it is sure of); gts: (box, class, crowd)."""
    lp = np.full((len(dets), K + 1), -100.0)
    for i, d in enumerate(dets):
        lp[i, d[2]] = 0.0
    return dict(H=H, W=W, det_boxes=np.array([d[0] for d in dets], dtype=np.float64).reshape(-1, 4), det_vars=np.array([d[1] for d in dets], dtype=np.float64),
                det_lp=lp, gt_boxes=np.array([g[0] for g in gts], dtype=np.float64).reshape(-1, 4), gt_classes=[g[1] for g in gts],
                gt_crowd=[g[2] for g in gts], scores=np.ones(len(dets)))


def test_reference_hard_box_by_hand():
    # an 8 x 8 image, the hard box [2, 6] x [2, 6]: 16 pixels at P = 1, the rest at P = 0
    P, Q = R.detection([2, 2, 6, 6], 0.0, 8, 8)
    assert P.sum() == 16 and (P[2:6, 2:6] == 1).all() and ((P == 0) | (P == 1)).all() and (Q == 1 - P).all()
    S = R.gt_pixels(np.array([2.0, 2, 6, 6]), 8, 8)
    r = R.pair(P, Q, S, 0.0027)
    assert r["FG"] == 0.0 and r["BG"] == 0.0 and r["n_g"] == 16
    # the ground truth two pixels to the right: 8 of its 16 pixels at P = 0 (log eps each), 8 pixels of the box outside it at Q = 0
    S = R.gt_pixels(np.array([4.0, 2, 8, 6]), 8, 8)
    r = R.pair(P, Q, S, 0.0027)
    assert r["FG"] == 8 * math.log(1e-14) / 16 and r["BG"] == 8 * math.log(1e-14) / 16
    im = image(8, 8, [([2, 2, 6, 6], 0.0, 1)], [([2, 2, 6, 6], 1, 0), ([4, 2, 8, 6], 1, 0), ([4, 2, 8, 6], 2, 0)])
    (res,), flags = R.pair_quality([im], 3)
    assert res["q"][0, 0] == 1.0 and res["fg"][0, 0] == 1.0 and res["bg"][0, 0] == 1.0 and res["label"][0, 0] == 1.0
    assert abs(res["fg"][1, 0] - 1e-7) < 1e-21 and abs(res["q"][1, 0] - 1e-7) < 1e-21 and res["label"][2, 0] == math.exp(-100.0)
    assert flags == [0, 0, 0, 0]
    # half-pixel edges: x1g = 2.5 includes pixel 2, x2g = 5.5 excludes pixel 5
    S = R.gt_pixels(np.array([2.5, 0.0, 5.5, 1.0]), 8, 8)
    assert np.nonzero(S[0])[0].tolist() == [2, 3, 4] and S.sum() == 3
    # a soft box: one column's p and q by hand from math.erfc
    sx, sy = R.sigmas(np.array([2.0, 2, 6, 6]), 4.0)
    assert sx == 2.0 * 4.0 * math.sqrt(1 / 100 + 1 / 100) == sy
    p, q = R.axis(2.0, 6.0, sx, 8)
    a, b = (3.5 - 2.0) / sx, (6.0 - 3 - 0.5) / sx
    Phi = lambda z: 0.5 * math.erfc(-z / math.sqrt(2))      # noqa: E731
    assert abs(p[3] - Phi(a) * Phi(b)) < 4 * R.U and abs(p[3] + q[3] - 1) < 4 * R.U
    # the records of the pipeline: one true positive at q = 1, one false positive, one false negative (the crowd box is neither)
    im = image(8, 8, [([2, 2, 6, 6], 0.0, 1), ([0, 0, 1, 1], 0.0, 0)], [([2, 2, 6, 6], 1, 0), ([6, 6, 8, 8], 2, 0), ([0, 0, 8, 8], 1, 1)])
    im["det_lp"][1, 2] = -np.inf          # eps keeps every spatial quality above 0: only a label probability of 0 makes q = 0
    rec, bound, value = R.pdq([im], 3)
    assert bound.shape == (8,) and (bound[1:4] == 0).all() and (bound[[0, 4, 5, 6, 7]] > 0).all()
    assert rec[0].tolist() == [1.0, 1, 1, 1, 1.0, 1.0, 1.0, 1.0] and value == 1.0 / 3
