"""Weighted boxes fusion (csrc/wbf.hip) without a GPU: the hand cases through the NumPy statement of the rule, that
statement against the textbook form in longdouble, the options, the command line and the argument checks of pe_wbf_fuse_batch."""
import ctypes
import os
import re

import numpy as np
import pytest

import wbf_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["thermal_only", "early_fusion"]


# ---- 1. the rule ----------------------------------------------------------------------------------------------------------------------

def test_hand_case_joins_the_fused_box_only():
    """C overlaps neither A (0.513) nor B (0.499) above 0.55 but the fused box of A and B (0.616): one cluster of 3.  A pivot clustering
    at the same threshold leaves C alone."""
    c = W.hand_case("joins_the_fused_box_only")
    r = W.numpy_rule(**c)
    assert r["count"] == 1 and r["rows"] == [[0, 1, 2]] and r["members"].tolist() == [3] and r["cluster"].tolist() == [0, 0, 0]
    assert r["conf"][0] == (((0.9 + 0.89) + 0.88) / 3.0 * 2.0) / 2.0 and round(float(r["conf"][0]), 12) == 0.89
    assert np.round(r["boxes"][0], 3).tolist() == [5.599, -3.970, 83.730, 113.876]
    pivot = W._iou(c["boxes"][:1], c["boxes"][2], np.float64)[0]
    assert round(float(pivot), 3) == 0.513 and pivot < 0.55


def test_hand_case_matches_the_pivot_not_the_fused_box():
    """C overlaps A with 0.630 but the fused box of A and B with about 0.47: two clusters."""
    c = W.hand_case("matches_the_pivot_not_the_fused_box")
    r = W.numpy_rule(**c)
    assert r["count"] == 2 and r["rows"] == [[0, 1], [2]] and r["cluster"].tolist() == [0, 0, 1]
    assert r["conf"][0] == ((0.9 + 0.89) / 2.0 * 2.0) / 2.0 and r["conf"][1] == (0.88 / 1.0 * 1.0) / 2.0
    assert [round(float(x), 12) for x in r["conf"]] == [0.895, 0.44]
    assert round(float(W._iou(c["boxes"][:1], c["boxes"][2], np.float64)[0]), 3) == 0.630
    assert abs(float(W._iou(r["boxes"][:1], c["boxes"][2], np.float64)[0]) - 0.47) < 0.01


def test_hand_case_exactly_at_the_threshold():
    """IoU exactly 0.5 at thr 0.5: the comparison is strict, two clusters."""
    c = W.hand_case("exactly_at_the_threshold")
    r = W.numpy_rule(**c)
    assert W._iou(c["boxes"][:1], c["boxes"][1], np.float64)[0] == 0.5 and r["margin"] == 0.0
    assert r["count"] == 2 and r["rows"] == [[0], [1]] and [float(x) for x in r["conf"]] == [0.45, 0.4]
    assert r["boxes"].tolist() == c["boxes"].tolist()


SETS = 60


def test_numpy_rule_against_textbook():
    """Seeded sets of up to 200 rows, 3 classes, 3 detectors, u = 1, 0.7, 1.3 (wbf_ref.random_set: all coordinates positive).  The
    running sums in float64 against member lists summed afresh in longdouble: the same clusters, in the same order, and every fused
    coordinate within (2 n + 4) u |x| for a cluster of n rows (first order in u, the derivation gives 2 n + 2; u =
    2^-53).  No IoU either form evaluates lies within 1e-9 of thr, so the two precisions cannot disagree on a decision: asserted, not
    skipped.  On these sets: 2 501 clusters of two or more rows, the largest of 8, worst ratio to the bound 0.35, closest IoU 1.1e-3."""
    multi, largest, worst, closest = 0, 0, 0.0, np.inf
    for seed in range(SETS):
        c = W.random_set(seed)
        assert len(c["scores"]) <= 200
        r, t = W.numpy_rule(**c), W.textbook(**c)
        closest = min(closest, r["margin"], t["margin"])
        assert r["rows"] == t["rows"] and r["count"] == t["count"] and r["classes"].tolist() == t["classes"].tolist(), seed
        assert r["cluster"].tolist() == t["cluster"].tolist() and r["skipped"] == t["skipped"] == 0
        for k, n in enumerate(r["members"]):
            x = t["boxes"][k]
            err = np.abs(r["boxes"][k].astype(np.longdouble) - x)
            bound = (2 * int(n) + 4) * W.U53 * np.abs(x)
            assert (err <= bound).all(), (seed, k, n)
            if n > 1:
                multi += 1
                largest = max(largest, int(n))
                worst = max(worst, float(np.max(err / bound)))
        # conf: a product per row, n - 1 additions, two divisions, a product and U's two additions - (n + 6) u, relative
        assert (np.abs(r["conf"].astype(np.longdouble) - t["conf"]) <= (r["members"] + 6) * W.U53 * t["conf"]).all(), seed
    print(f"{multi} multi-row clusters, largest {largest}, worst ratio {worst:.3f}, closest IoU to thr {closest:.3g}")
    assert closest > 1e-9
    assert multi > 1000 and largest >= 5


def test_skip_conditions_under_the_numpy_rule():
    """The skip conditions as the rule states them: s == skip is kept, one ulp below is not."""
    s = 0.3 * 0.7
    box = [[10.0, 10, 50, 50]] * 2
    r = W.numpy_rule(box, [0.3, 0.3], [0, 0], [1, 1], [1.0, 0.7], skip=s, K=1)
    assert r["skipped"] == 0 and r["count"] == 1
    r = W.numpy_rule(box, [0.3, 0.3], [0, 0], [1, 1], [1.0, 0.7], skip=np.nextafter(s, 1.0), K=1)
    assert r["skipped"] == 2 and r["count"] == 0 and r["cluster"].tolist() == [-1, -1]


# ---- 2. the options -------------------------------------------------------------------------------------------------------------------

def test_options_accept_the_pair_and_refuse_a_half():
    from proben_amd.options import FusionOptions
    o = FusionOptions("wbf", "wbf", num_detectors=2)
    assert o.wbf and o.needs_row_source and o.wbf_weights == [1.0, 1.0] and o.wbf_skip == 0.0 and not o.logp and not o.cavg
    with pytest.raises(ValueError, match="box_fusion 'wbf'"):
        FusionOptions("wbf", "v-avg")
    with pytest.raises(ValueError, match="score_fusion 'wbf'"):
        FusionOptions("avg", "wbf")
    plain = FusionOptions("probEn", "v-avg", num_detectors=2)
    assert not plain.wbf and plain.wbf_weights is None and plain.wbf_skip is None and not plain.needs_row_source
    with pytest.raises(ValueError, match="wbf_weights belong"):
        FusionOptions("probEn", "v-avg", wbf_weights=[1, 1])
    with pytest.raises(ValueError, match="wbf_skip belongs"):
        FusionOptions("probEn-log", "v-avg", wbf_skip=0.1)


@pytest.mark.parametrize("keyword", [dict(class_prior=[0.2, 0.3, 0.3, 0.2]), dict(pool_weights=[1.0, 0.5]), dict(presence=np.zeros((4, 4))),
                                     dict(with_posterior=True), dict(box_correlation=[[0.0, 0.3], [0.3, 0.0]]),
                                     dict(variance_scales=[1.0, 2.0])], ids=lambda k: next(iter(k)))
def test_options_refuse_what_wbf_does_not_read(keyword):
    from proben_amd.options import FusionOptions
    with pytest.raises(ValueError, match=f"{next(iter(keyword))} belongs? to .*got 'wbf'.*reads no variance, probability or logit"):
        FusionOptions("wbf", "wbf", num_detectors=2, **keyword)


def test_options_keep_temperatures_legal():
    from proben_amd.options import FusionOptions
    assert FusionOptions("wbf", "wbf", temperatures=[1.5, 0.8]).temperatures == [1.5, 0.8]


@pytest.mark.parametrize("weights, message", [([1.0], "1 wbf weights for 2 detectors"), ([1.0, 1.0, 1.0], "3 wbf weights for 2 detectors"),
                                              ([1.0, -0.5], "not finite and >= 0"), ([0.0, 0.0], "all 0"),
                                              ([1.0, float("nan")], "not finite and >= 0"), ([1.0, float("inf")], "not finite and >= 0")])
def test_options_validate_the_weights(weights, message):
    from proben_amd.options import FusionOptions
    with pytest.raises(ValueError, match=message):
        FusionOptions("wbf", "wbf", num_detectors=2, wbf_weights=weights)


def test_options_validate_the_skip_and_round_trip():
    from proben_amd.options import FusionOptions
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="wbf_skip"):
            FusionOptions("wbf", "wbf", num_detectors=2, wbf_skip=bad)
    o = FusionOptions("wbf", "wbf", wbf_weights=[1.0, 0.7], wbf_skip=0.05, temperatures=[1.2, 0.9])
    assert o.num_detectors == 2
    again = o.replace()
    assert (again.score_fusion, again.box_fusion, again.wbf_weights, again.wbf_skip, again.temperatures) == \
        ("wbf", "wbf", [1.0, 0.7], 0.05, [1.2, 0.9])
    assert o.replace(wbf_weights=[2.0, 1.0]).wbf_weights == [2.0, 1.0] and o.replace(wbf_skip=0.0).wbf_skip == 0.0
    assert o.named(NAMES) == {"temperatures": {"thermal_only": 1.2, "early_fusion": 0.9},
                              "wbf_weights": {"thermal_only": 1.0, "early_fusion": 0.7}, "wbf_skip": 0.05}
    assert "wbf_weights" not in FusionOptions("probEn", "v-avg", num_detectors=2).named(NAMES)
    with pytest.raises(ValueError, match="wbf_skip belongs"):
        o.replace(score_fusion="avg", box_fusion="avg", wbf_weights=None)


def test_entry_points_take_the_pair_through_of():
    """What fusion(), late_fusion, fuse_detections and FramePairPipeline do with their keywords: the detector count fills in the weights."""
    from proben_amd.options import FusionOptions
    o = FusionOptions.of(None, "late_fusion", 3, "wbf", "wbf")
    assert o.wbf_weights == [1.0, 1.0, 1.0] and o.who == "late_fusion"
    assert FusionOptions.of(o, "fuse_detections", 3) is o
    with pytest.raises(ValueError, match="options for 3 detectors, 2 given"):
        FusionOptions.of(o, "fuse_detections", 2)


# ---- 3. the command line --------------------------------------------------------------------------------------------------------------

def _args(*flags):
    from proben_amd.opt import config_parser
    return config_parser(["--detectors", ",".join(NAMES)] + list(flags))


def test_cli_parses_the_three_flag_forms():
    from proben_amd.options import FusionOptions
    wbf = ["--score_fusion", "wbf", "--box_fusion", "wbf"]
    a = _args(*wbf)
    assert a.wbf_iou == 0.55 and a.wbf_skip == 0.0 and a.wbf_weights is None
    o = FusionOptions.from_args(a, NAMES, say=None)
    assert o.wbf and o.wbf_weights == [1.0, 1.0] and o.wbf_skip == 0.0 and not o.with_posterior
    by_position = FusionOptions.from_args(_args(*wbf, "--wbf_weights", "1,0.7"), NAMES, say=None)
    by_name = FusionOptions.from_args(_args(*wbf, "--wbf_weights", "early_fusion=0.7,thermal_only=1"), NAMES, say=None)
    assert by_position.wbf_weights == by_name.wbf_weights == [1.0, 0.7]
    a = _args(*wbf, "--wbf_iou", "0.6", "--wbf_skip", "0.05", "--write_fused", "fused.json", "--temperatures", "1.4,0.9")
    o = FusionOptions.from_args(a, NAMES, say=None)
    assert a.wbf_iou == 0.6 and o.wbf_skip == 0.05 and a.write_fused == "fused.json" and not o.with_posterior and o.temperatures == [1.4, 0.9]
    with pytest.raises(ValueError, match="lists 3 values for 2"):
        FusionOptions.from_args(_args(*wbf, "--wbf_weights", "1,1,1"), NAMES, say=None)
    with pytest.raises(ValueError, match="all 0"):
        FusionOptions.from_args(_args(*wbf, "--wbf_weights", "0,0"), NAMES, say=None)


@pytest.mark.parametrize("flags", [["--score_fusion", "wbf"], ["--box_fusion", "wbf"], ["--wbf_weights", "1,1"],
                                   ["--score_fusion", "wbf", "--box_fusion", "wbf", "--variance_scales", "1,2"],
                                   ["--score_fusion", "wbf", "--box_fusion", "wbf", "--pool_weights", "1,1"],
                                   ["--score_fusion", "wbf", "--box_fusion", "wbf", "--class_prior", "0.25,0.25,0.25,0.25"],
                                   ["--score_fusion", "avg", "--box_fusion", "avg", "--write_fused", "x.json"]])
def test_cli_refuses_the_wrong_combinations(flags, capsys):
    with pytest.raises(SystemExit):
        _args(*flags)
    capsys.readouterr()


def test_cli_without_wbf_parses_as_before():
    from proben_amd.options import FusionOptions
    o = FusionOptions.from_args(_args(), NAMES, say=None)
    assert (o.score_fusion, o.box_fusion, o.wbf, o.wbf_weights, o.wbf_skip) == ("probEn", "v-avg", False, None, None)
    assert o.named(NAMES) == {}


# ---- 4. the C-ABI's argument checks ---------------------------------------------------------------------------------------------------

def _limits():
    txt = open(os.path.join(ROOT, "include", "proben_hip.h")).read()
    return {k: int(re.search(rf"#define {k} (\d+)", txt).group(1)) for k in ("PE_WBF_MAX_DETECTORS", "PE_WBF_MAX_ROWS", "PE_WBF_MAX_IMAGES")}


def test_argument_checks_answer_before_any_device_work():
    """Every refusal of pe_wbf_fuse_batch answers without a GPU, the three limits with the capacity in the message; B == 0 is PE_OK."""
    import __graft_entry__ as g
    g.build()
    import proben_amd
    L = proben_amd._lib.lib()
    lim = _limits()
    p = ctypes.c_void_p(4096)

    def call(B=1, K=3, R=16, D=2, thr=0.55, skip=0.0, inputs=None, outputs=None, counts=None):
        i = [p] * 5 if inputs is None else inputs            # boxes, scores, classes, row_source, offsets
        o = [p] * 7 if outputs is None else outputs
        st = L.pe_wbf_fuse_batch(i[0], i[1], i[2], i[3], i[4], counts, B, K, R, p, D, thr, skip, *o, None)
        return st, L.pe_last_error().decode()

    assert call(B=0)[0] == 0
    assert L.pe_wbf_fuse_batch(*([None] * 6), 0, 3, 16, None, 2, 0.55, 0.0, *([None] * 7), None) == 0        # nothing to do, nothing read
    st, msg = call(B=-1)
    assert st == -1 and "num_images < 0" in msg
    for k in range(5):
        st, msg = call(inputs=[None if j == k else p for j in range(5)])
        assert st == -1 and "null input pointer" in msg, k
    for k in range(7):
        st, msg = call(outputs=[None if j == k else p for j in range(7)])
        assert st == -1 and "null output pointer" in msg, k
    st, msg = call(K=0)
    assert st == -1 and "num_classes 0" in msg
    st, msg = call(D=0)
    assert st == -1 and "num_detectors 0" in msg
    st, msg = call(R=0)
    assert st == -1 and "max_rows_per_image 0" in msg
    st, msg = call(thr=float("nan"))
    assert st == -1 and "iou_thresh is NaN" in msg
    st, msg = call(skip=float("nan"))
    assert st == -1 and "skip_thresh is NaN" in msg
    # the three limits: PE_ERR_UNSUPPORTED, with the capacity
    st, msg = call(R=lim["PE_WBF_MAX_ROWS"] + 1)
    assert st == -2 and f"capacity of {lim['PE_WBF_MAX_ROWS']} rows" in msg and "164 bytes of LDS per row" in msg
    st, msg = call(D=lim["PE_WBF_MAX_DETECTORS"] + 1)
    assert st == -2 and f"above the {lim['PE_WBF_MAX_DETECTORS']} entries of the weight table" in msg
    st, msg = call(B=lim["PE_WBF_MAX_IMAGES"] + 1)
    assert st == -2 and f"above the {lim['PE_WBF_MAX_IMAGES']} images of one launch" in msg
    assert lim == {"PE_WBF_MAX_DETECTORS": 8, "PE_WBF_MAX_ROWS": 996, "PE_WBF_MAX_IMAGES": 4194303}


def test_fuse_batch_checks_its_wbf_arguments_on_the_host():
    import torch
    from proben_amd import fusion as F
    z = torch.zeros((2, 4), dtype=torch.float64)
    offs = torch.tensor([0, 2], dtype=torch.int32)
    src = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="needs row_source"):
        F.fuse_batch(z, z[:, 0], None, None, src, offs, "wbf", "wbf", wbf_weights=[1.0, 1.0], num_classes=3)
    with pytest.raises(ValueError, match="needs wbf_weights"):
        F.fuse_batch(z, z[:, 0], None, None, src, offs, "wbf", "wbf", row_source=src, num_classes=3)
    with pytest.raises(ValueError, match="probs .* or num_classes"):
        F.fuse_batch(z, z[:, 0], None, None, src, offs, "wbf", "wbf", row_source=src, wbf_weights=[1.0, 1.0])
    from proben_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError):
        F.fuse_batch(z, z[:, 0], None, None, src, offs, "wbf", "wbf", row_source=src, wbf_weights=[1.0, 1.0], num_classes=3)
    assert F.WBF == "wbf" and F.WBF not in F.SCORE_MODES and F.WBF not in F.BOX_MODES and F.WBF_IOU == 0.55
