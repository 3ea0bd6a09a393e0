"""Variance voting without a GPU: the rule's NumPy restatement (tests/var_vote_ref.py) on cases worked by hand, its invariants on
random piles and what it recovers; pe_boxhead_var_vote's argument checks, which answer before any device work; the cfg keys and the
CLI flag on their way to rcnn.DetectorConfig."""
import math
import os
import re

import numpy as np
import pytest

import var_vote_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
S = 0.025


def boxes_of(*rows):
    return np.array(rows, dtype=F32)


# ------------------------------------------------------------------------------------------------ hand-worked cases
def test_two_overlapping_boxes_by_hand():
    """b = [0,0,10,10], i = [5,0,15,10]: inter 50, union 150, IoU 1/3, p = exp(-(2/3)^2 / sigma_t).  Variances 0.25 and 0.5."""
    bx = boxes_of([0, 0, 10, 10], [5, 0, 15, 10])
    p = math.exp(-(1.0 - 50.0 / 150.0) ** 2 / float(F32(S)))
    w0, w1 = 1.0 / 0.25, p / 0.5
    want = [(w0 * 0 + w1 * 5) / (w0 + w1), 0.0, (w0 * 10 + w1 * 15) / (w0 + w1), 10.0]
    out = V.vote(bx, [0, 0], [0.25, 0.5], [0], S)
    np.testing.assert_array_equal(out[0], np.array(want, dtype=F32))
    np.testing.assert_array_equal(V.bits(out[1]), V.bits(bx[1]))               # not kept: its input bits
    # with sigma_t = 1 the weights are round enough to see: p = exp(-4/9)
    out = V.vote(bx, [0, 0], [0.25, 0.5], [0], 1.0)
    w1 = math.exp(-4.0 / 9.0) / 0.5
    assert out[0, 0] == F32(5 * w1 / (4 + w1)) and out[0, 2] == F32((40 + 15 * w1) / (4 + w1))


def test_three_overlapping_boxes_by_hand():
    """Kept [0,0,8,8] (var 1), a duplicate shifted by 4 in x (IoU 32/96 = 1/3, var 0.5) and one shifted by 4 in y (var 0.25); sigma_t =
    4/9 makes p = exp(-1) for both neighbours."""
    bx = boxes_of([0, 0, 8, 8], [4, 0, 12, 8], [0, 4, 8, 12])
    s = float(F32(4.0 / 9.0))
    p = math.exp(-(1.0 - 32.0 / 96.0) ** 2 / s)
    w = [1.0, p / 0.5, p / 0.25]
    sw = math.fsum(w)
    want = [w[1] * 4 / sw, w[2] * 4 / sw, (8 * w[0] + 12 * w[1] + 8 * w[2]) / sw, (8 * w[0] + 8 * w[1] + 12 * w[2]) / sw]
    out = V.vote(bx, [2, 2, 2], [1.0, 0.5, 0.25], [0], 4.0 / 9.0)
    assert V.within_one_ulp(out[0], np.array(want, dtype=F32))
    # the lower variance pulls harder: y moves more than x
    assert out[0, 1] > out[0, 0] > 0


def test_who_votes():
    """Another class on top of the kept box, a box sharing only an edge (IoU 0), a zero-area candidate inside it, and neighbours with
    variance 0, inf and NaN: none of them votes, so the kept box keeps its bits although a valid neighbour would have moved it."""
    kept = [10, 10, 30, 30]
    bx = boxes_of(kept, kept, [30, 10, 50, 30], [15, 15, 15, 25], [12, 10, 32, 30], [12, 10, 32, 30], [12, 10, 32, 30])
    cls = [1, 0, 1, 1, 1, 1, 1]
    var = [0.01, 0.01, 0.01, 0.01, 0.0, np.inf, np.nan]
    ids, iou = V.voters(bx, cls, var, 0)
    assert ids.tolist() == [0] and iou.tolist() == [1.0]
    np.testing.assert_array_equal(V.bits(V.vote(bx, cls, var, [0], S)), V.bits(bx))
    var[4] = 0.01                                                   # the same neighbour with a usable variance does move it
    assert V.vote(bx, cls, var, [0], S)[0, 0] > 10


def test_kept_box_with_bad_variance_or_no_area_is_unchanged():
    bx = boxes_of([10, 10, 30, 30], [12, 10, 32, 30], [40, 40, 40, 60], [40, 40, 44, 60])
    for bad in (0.0, np.inf, np.nan, -1.0):
        out = V.vote(bx, [0, 0, 0, 0], [bad, 0.01, 0.01, 0.01], [0], S)
        np.testing.assert_array_equal(V.bits(out), V.bits(bx))
    out = V.vote(bx, [0, 0, 0, 0], [0.01] * 4, [2], S)              # a kept box without area: IoU with itself is 0
    np.testing.assert_array_equal(V.bits(out), V.bits(bx))
    out = V.vote(bx, [0, 0, 0, 0], [0.01] * 4, [7, -1], S)          # keep ids outside the list are skipped
    np.testing.assert_array_equal(V.bits(out), V.bits(bx))


def test_sigma_to_zero_returns_the_input_bits():
    rng = np.random.default_rng(5)
    bx, cls, lv = V.random_pile(rng, 60, 2)
    bx[7], cls[7] = bx[3], cls[3]                                   # an exact duplicate of a kept box, with its own variance
    var = np.exp(lv).astype(F32)
    keep = [3, 7, 11, 20, 59]
    assert len(V.voters(bx, cls, var, 3)[0]) > 2
    out = V.vote(bx, cls, var, keep, 1e-30)
    np.testing.assert_array_equal(V.bits(out), V.bits(bx))
    assert (V.bits(V.vote(bx, cls, var, keep, S)[keep]) != V.bits(bx[keep])).any()


# ------------------------------------------------------------------------------------------------ invariants, recovery
def test_voted_boxes_stay_inside_the_image_with_positive_extent():
    rng = np.random.default_rng(11)
    for trial in range(20):
        hw = (int(rng.integers(200, 600)), int(rng.integers(200, 700)))
        bx, cls, lv = V.random_pile(rng, int(rng.integers(20, 120)), 3, image_hw=hw, bad_fraction=0.1)
        keep = rng.choice(len(bx), 10, replace=False)
        out = V.vote(bx, cls, np.exp(lv.astype(np.float64)).astype(F32), keep, S)
        assert (out >= 0).all() and (out[:, 0::2] <= hw[1]).all() and (out[:, 1::2] <= hw[0]).all()
        assert (out[:, 2] > out[:, 0]).all() and (out[:, 3] > out[:, 1]).all()
        rest = np.setdiff1d(np.arange(len(bx)), keep)
        np.testing.assert_array_equal(V.bits(out[rest]), V.bits(bx[rest]))
        for b in keep:                                              # a convex combination: inside the hull of its voters
            ids, _ = V.voters(bx, cls, np.exp(lv.astype(np.float64)).astype(F32), b)
            if b in ids:
                assert (out[b] >= bx[ids].min(0)).all() and (out[b] <= bx[ids].max(0)).all()


def test_voting_recovers_the_box_from_noisy_candidates():
    """2 000 piles of 12 candidates around a 100 x 60 box, corner errors N(0, var_i * size^2), var_i log-uniform in [1e-4, 1e-2], the
    kept box one of them at random, sigma_t = 0.025: the RMS corner error of the voted boxes is below half the kept boxes'.  (The rule
    alone gives 0.29 to 0.33 over seeds; 0.5 is a cap a broken weighting misses, not a measurement.)"""
    rng = np.random.default_rng(20190616)
    gt, boxes, var = V.recovery_piles(rng)
    kept = rng.integers(0, boxes.shape[1], len(gt))
    err_kept, err_voted = [], []
    for g, bx, v, b in zip(gt, boxes, var, kept):
        out = V.vote(bx, np.zeros(len(bx), dtype=np.int32), v, [b], S)
        err_kept.append(bx[b].astype(np.float64) - g)
        err_voted.append(out[b].astype(np.float64) - g)
    rms = lambda e: float(np.sqrt(np.mean(np.square(e))))
    ratio = rms(err_voted) / rms(err_kept)
    print(f"recovery: rms kept {rms(err_kept):.4f}, voted {rms(err_voted):.4f}, ratio {ratio:.4f}")
    assert ratio < 0.5, ratio


# ------------------------------------------------------------------------------------------------ the C-ABI without a GPU
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.lib()


def test_entry_point_is_declared_exported_and_bound(L):
    import proben_amd
    hdr = open(os.path.join(ROOT, "include", "proben_hip.h")).read()
    assert re.search(r"\bint\s+pe_boxhead_var_vote\s*\(", hdr) and re.search(r"#define\s+PE_VAR_VOTE_TILE\s+\d+", hdr)
    assert "pe_boxhead_var_vote" in proben_amd._lib.SIGNATURES and hasattr(L, "pe_boxhead_var_vote")


def test_argument_checks_answer_before_any_device_work(L):
    err = lambda: L.pe_last_error().decode()
    A = 4096                                                        # never dereferenced: every call below is refused first
    K = 3

    def call(head=A, stride=5 * K + 2, N=2, P=8, K=K, cmax=16, D=4, cb=A, cc=A, cr=A, ccnt=A, keep=A, kcnt=A, sigma=0.025, out=2 * A):
        return L.pe_boxhead_var_vote(head, stride, N, P, K, cmax, D, cb, cc, cr, ccnt, keep, kcnt, sigma, out, None)

    for sigma in (0.0, -0.025, float("nan"), float("inf"), -float("inf")):
        assert call(sigma=sigma) == -1 and "pe_boxhead_var_vote" in err() and "sigma_t" in err(), (sigma, err())
    assert call(out=A) == -1 and "alias" in err()
    assert call(K=81, stride=5 * 81 + 2) == -1 and "num_classes 81" in err()
    assert call(K=0) == -1 and "num_classes 0" in err()
    assert call(stride=5 * K + 1) == -1 and "head_stride" in err()
    for cmax in (0, 16385):
        assert call(cmax=cmax) == -1 and "cand_max" in err()
    assert call(D=0) == -1 and "max_det" in err()
    for name in ("head", "cb", "cc", "cr", "ccnt", "keep", "kcnt"):
        assert call(**{name: None}) == -1 and "null input" in err(), name
    assert call(out=None) == -1 and "null output" in err()
    assert call(N=0) == 0                                           # no image: nothing to do
    assert call(N=0, sigma=0.0) == -1                               # ... but the arguments are still checked


# ------------------------------------------------------------------------------------------------ configuration
def test_cfg_keys_reach_the_detector_config():
    import proben_amd
    from proben_amd.predictor import detector_config_from_cfg
    from proben_amd.rcnn import DetectorConfig
    d = DetectorConfig()
    assert d.var_voting is False and d.var_voting_sigma_t == 0.025
    cfg = proben_amd.get_cfg()
    assert cfg.PROBEN.VAR_VOTING is False and cfg.PROBEN.VAR_VOTING_SIGMA_T == 0.025
    d = detector_config_from_cfg(cfg)
    assert d.var_voting is False and d.var_voting_sigma_t == 0.025
    cfg.PROBEN.VAR_VOTING, cfg.PROBEN.VAR_VOTING_SIGMA_T = True, 0.01
    d = detector_config_from_cfg(cfg)
    assert d.var_voting is True and d.var_voting_sigma_t == 0.01
    old = proben_amd.get_cfg()                                      # a cfg from before the keys existed still loads, voting off
    del old["PROBEN"]["VAR_VOTING"], old["PROBEN"]["VAR_VOTING_SIGMA_T"]
    d = detector_config_from_cfg(old)
    assert d.var_voting is False and d.var_voting_sigma_t == 0.025
    del old["PROBEN"]
    assert detector_config_from_cfg(old).var_voting is False


def test_var_voting_needs_the_variance_head():
    from proben_amd.rcnn import DetectorConfig, GeneralizedRCNN
    with pytest.raises(ValueError, match="variance head"):
        GeneralizedRCNN(DetectorConfig(var_voting=True, enable_gaussian_nll=False), {})
    with pytest.raises(ValueError, match="sigma_t"):
        GeneralizedRCNN(DetectorConfig(var_voting=True, var_voting_sigma_t=0.0), {})


def test_cli_flag_sets_the_keys():
    from proben_amd.cli.save_predictions import build_cfg
    from proben_amd.opt import config_parser
    from proben_amd.predictor import detector_config_from_cfg
    base = ["--fusion_method", "thermal_only"]
    for argv, want in (([], (False, 0.025)), (["--var_voting"], (True, 0.025)), (["--var_voting", "0.01"], (True, 0.01))):
        args = config_parser(base + argv)
        cfg = build_cfg(args)
        assert (cfg.PROBEN.VAR_VOTING, cfg.PROBEN.VAR_VOTING_SIGMA_T) == want, argv
        d = detector_config_from_cfg(cfg)
        assert (d.var_voting, d.var_voting_sigma_t) == want
    assert config_parser(base).var_voting is None
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            config_parser(base + ["--var_voting", bad])
    # demo_probEn reads the same parser; its one-pass route builds one cfg per detector and every one carries the flag
    from proben_amd.cli import demo_probEn
    names = ["thermal_only", "early_fusion", "middle_fusion"]
    for argv, want in (([], (False, 0.025)), (["--var_voting"], (True, 0.025)), (["--var_voting", "0.05"], (True, 0.05))):
        args = config_parser(["--one-pass", "--detectors", ",".join(names)] + argv)
        assert args.one_pass
        cfgs = demo_probEn.detector_cfgs(args, names, ["synthetic://1", "synthetic://2", "synthetic://3"])
        assert [c.INPUT.FORMAT for c in cfgs] == ["BGR", "BGRT", "BGRTTT"] and [c.MODEL.WEIGHTS for c in cfgs][2] == "synthetic://3"
        for c in cfgs:
            d = detector_config_from_cfg(c)
            assert (d.var_voting, d.var_voting_sigma_t) == want and d.enable_gaussian_nll, argv
