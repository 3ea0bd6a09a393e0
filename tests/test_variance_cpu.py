"""Variance calibration without a GPU: the new symbols are exported, declared and bound and check their arguments before any device
work; parse_variance_scales and the calibration file's variance keys; the closed form of the fit on a NumPy float64 restatement; and
what a per-detector scale does (and a common one does not do) to the oracle's v-avg boxes."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pe_match_ground_truth", "pe_variance_stats", "pe_proben_pack_calibrated")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.lib()


def _err(L):
    return L.pe_last_error().decode()


# ---- NumPy float64 restatements (tests/test_variance_gpu.py imports them) ----------------------------------------------------

def np_deltas(src, tgt, weights=(10.0, 10.0, 5.0, 5.0)):
    """Box2BoxTransform.get_deltas (modeling.py) in float64: w[:2] * (tc - sc) / swh, w[2:] * log(twh / swh)."""
    src, tgt, w = np.asarray(src, np.float64), np.asarray(tgt, np.float64), np.asarray(weights, np.float64)
    swh, twh = src[:, 2:] - src[:, :2], tgt[:, 2:] - tgt[:, :2]
    sc, tc = src[:, :2] + 0.5 * swh, tgt[:, :2] + 0.5 * twh
    return np.concatenate([w[:2] * (tc - sc) / swh, w[2:] * np.log(twh / swh)], axis=1)


def np_stats(det, match, gt, var, s=1.0, weights=(10.0, 10.0, 5.0, 5.0)):
    """pe_variance_stats restated: per-row terms in float64 (the kernel's expression order), sums by math.fsum.
    Returns (n, sum q, sum log var, cover1, cover2, excluded rows, sum |q|, sum |log var|)."""
    det, gt, var = np.asarray(det, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4), np.asarray(var, np.float64)
    match = np.asarray(match)
    ok = (match >= 0) & np.isfinite(var) & (var > 0)
    tgt = gt[np.where(ok, match, 0)] if len(gt) else np.zeros_like(det)
    ok &= (det[:, 2] - det[:, 0] > 0) & (det[:, 3] - det[:, 1] > 0) & (tgt[:, 2] - tgt[:, 0] > 0) & (tgt[:, 3] - tgt[:, 1] > 0)
    r = np_deltas(det[ok], tgt[ok], weights)
    v = var[ok]
    r2 = r * r
    q = ((r2[:, 0] / v + r2[:, 1] / v) + r2[:, 2] / v) + r2[:, 3] / v
    lv = np.log(v)
    c1 = int((r2 <= (s * v)[:, None]).sum())
    c2 = int((r2 <= (4.0 * (s * v))[:, None]).sum())
    return (int(ok.sum()), math.fsum(q), math.fsum(lv), c1, c2, np.nonzero(~ok)[0], math.fsum(np.abs(q)), math.fsum(np.abs(lv)))


def np_nll(n, sum_q, sum_log_var, s):
    return 0.5 * (4 * n * math.log(s) + 4 * sum_log_var + sum_q / s)


def gaussian_rows(rng, n, s_true, weights=(10.0, 10.0, 5.0, 5.0)):
    """(det, gt, var): detections, ground-truth boxes built FROM them so that get_deltas(det, gt) is Gaussian with variance
    s_true * var_i by construction (the residual is measured from the detection as anchor, so the perturbation is applied from the
    detection), var log-uniform over two decades."""
    w = np.asarray(weights)
    x1, y1 = rng.uniform(0, 400, n), rng.uniform(0, 300, n)
    dw, dh = rng.uniform(20, 200, n), rng.uniform(20, 200, n)
    det = np.stack([x1, y1, x1 + dw, y1 + dh], 1)
    var = 10.0 ** rng.uniform(-3.0, -1.0, n)
    d = rng.standard_normal((n, 4)) * np.sqrt(s_true * var)[:, None]
    cx, cy = x1 + 0.5 * dw + d[:, 0] / w[0] * dw, y1 + 0.5 * dh + d[:, 1] / w[1] * dh
    gw, gh = dw * np.exp(d[:, 2] / w[2]), dh * np.exp(d[:, 3] / w[3])
    gt = np.stack([cx - 0.5 * gw, cy - 0.5 * gh, cx + 0.5 * gw, cy + 0.5 * gh], 1)
    return det, gt, var


# ---- symbols, bindings, argument checks ---------------------------------------------------------------------------------------

def test_new_symbols_are_exported_declared_and_bound(L):
    import proben_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "proben_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name + " is not declared"
        assert name in proben_amd._lib.SIGNATURES, name + " is not bound"
    assert re.search(r"#define\s+PE_VARIANCE_STATS_MAX_BLOCKS\s+1024", hdr)
    from proben_amd import calibration as C
    for fn in ("match_rows_device", "variance_stats", "fit_variance_scale", "check_variance_scale", "parse_variance_scales",
               "save_variance", "load_variance"):
        assert callable(getattr(C, fn)), fn
    assert os.path.exists(os.path.join(ROOT, "multimodal-object-detection-via-probabilistic-ensembling_amd", "csrc", "variance.hip"))


def _stats(L, scale=1.0, rows=10, gts=5, det=4096, match=4096, gt=4096, var=4096, work=4096, out=4096, flags=4096, w=None):
    return L.pe_variance_stats(det, match, gt, var, rows, gts, w, scale, work, out, flags, None)


@pytest.mark.parametrize("bad,shown", [(0.0, "0"), (-1.5, "-1.5"), (float("nan"), "nan"), (float("inf"), "inf")])
def test_bad_scales_are_named(L, bad, shown):
    assert _stats(L, bad) == -1
    assert "pe_variance_stats" in _err(L) and shown in _err(L) and "not finite and > 0" in _err(L)
    assert _pack(L, scales=[1.0, bad]) == -1
    assert "pe_proben_pack_calibrated" in _err(L) and shown in _err(L) and "detector 1" in _err(L)


def test_variance_stats_argument_checks(L):
    assert _stats(L, rows=-3) == -1 and "num_rows -3" in _err(L)
    assert _stats(L, gts=-1) == -1 and "num_gt -1" in _err(L)
    for kw in ("det", "match", "gt", "var"):
        assert _stats(L, **{kw: None}) == -1 and "null pointer (det_boxes" in _err(L), kw
    for kw in ("work", "out", "flags"):
        assert _stats(L, **{kw: None}) == -1 and "null pointer (workspace" in _err(L), kw
    w = (ctypes.c_float * 4)(10.0, 10.0, 0.0, 5.0)
    assert _stats(L, w=w) == -1 and "bbox_reg_weights[2]" in _err(L)


def test_match_ground_truth_argument_checks(L):
    ok = [4096] * 5 + [None]
    tail = [4096, 4096, 4096, None]
    assert L.pe_match_ground_truth(*ok, -1, 0.5, 3, *tail) == -1 and "num_images -1" in _err(L)
    assert L.pe_match_ground_truth(*ok, 2, 0.5, 0, *tail) == -1 and "num_classes 0" in _err(L)
    assert L.pe_match_ground_truth(*ok, 2, float("nan"), 3, *tail) == -1 and "iou_thresh" in _err(L)
    for i in range(5):
        a = list(ok)
        a[i] = None
        assert L.pe_match_ground_truth(*a, 2, 0.5, 3, *tail) == -1 and "null pointer" in _err(L), i
    for i in range(3):
        t = list(tail)
        t[i] = None
        assert L.pe_match_ground_truth(*ok, 2, 0.5, 3, *t) == -1 and "null output" in _err(L), i
    assert L.pe_match_ground_truth(*ok, 0, 0.5, 3, *tail) == 0          # no image: nothing to do


def _pack(L, scales=(1.0, 1.0), nd=2, logits=False, temps=True, both=False, outs=True, B=2, D=8, row_stride=None, tables=True, hole=None):
    """pe_proben_pack_calibrated with plausible (never dereferenced) pointers; every case here stops at an argument check."""
    tab = (ctypes.c_void_p * 4)(*([4096] * 4)) if tables else None
    holed = (ctypes.c_void_p * 4)(4096, 0, 4096, 4096)
    S = (ctypes.c_double * 4)(*(list(scales) + [1.0] * (4 - len(scales)))) if scales is not None else None
    T = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 1.0) if (logits and temps) else None
    o = 4096 if outs else None
    probs = tab if (not logits or both) else None
    return L.pe_proben_pack_calibrated(tab, probs, holed if hole == "classes" else tab, probs, tab if logits else None,
                                       holed if hole == "vars" else tab, tab, T, S, nd, B, D, 3, 2, nd * D if row_stride is None else row_stride,
                                       o, o, o, None, o, o, o, o, o, None)


def test_pack_calibrated_argument_checks(L):
    assert _pack(L, nd=5) == -1 and "num_detectors 5" in _err(L)
    assert _pack(L, nd=0) == -1 and "num_detectors 0" in _err(L)
    assert _pack(L, B=-1) == -1 and "num_images -1" in _err(L)
    assert _pack(L, D=-2) == -1 and "det_stride -2" in _err(L)
    assert _pack(L, tables=False) == -1 and "null pointer" in _err(L)
    assert _pack(L, logits=True, temps=False) == -1 and "temperatures" in _err(L)
    assert _pack(L, logits=True, both=True) == -1 and "one route at a time" in _err(L)
    assert _pack(L, hole="vars") == -1 and "null pointer of detector 1" in _err(L)
    assert _pack(L, hole="classes") == -1 and "null pointer of detector 1" in _err(L)
    # past its own checks the call is the existing entry point's, whose checks answer in its own name
    assert _pack(L, row_stride=15) == -1 and "pe_proben_pack_detections: row_stride 15 < 16" in _err(L)
    assert _pack(L, outs=False) == -1 and "null output" in _err(L)
    assert _pack(L, logits=True, row_stride=15) == -1 and "pe_proben_pack_logits: row_stride 15 < 16" in _err(L)
    assert _pack(L, B=0) == 0 and _pack(L, scales=None, B=0) == 0


def test_python_layer_refuses_cpu_tensors_bad_scales_and_length_mismatches(L):
    import torch
    import proben_amd
    from proben_amd import calibration as C, fusion as F
    from proben_amd.late_fusion import late_fusion
    from proben_amd.pipeline import FramePairPipeline
    z = torch.zeros((4, 4), dtype=torch.float64)
    with pytest.raises(proben_amd._lib.HipLibraryError):
        C.variance_stats(z, torch.zeros(4, dtype=torch.int32), z, torch.ones(4, dtype=torch.float64))
    with pytest.raises(proben_amd._lib.HipLibraryError):
        C.match_rows_device(z, torch.tensor([0, 4], dtype=torch.int32), z, torch.tensor([0, 4], dtype=torch.int32), torch.zeros(4, dtype=torch.int32))
    for bad in (0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="not finite and > 0"):
            C.check_variance_scale(bad)
    d = {"img_name": "a", "bbox": [[0, 0, 5, 5]], "score": [0.9], "class": [0], "prob": [[0.9, 0.05, 0.03]], "vars": [[1.0]]}
    with pytest.raises(ValueError, match="3 variance scales for 2 detectors"):
        F.fusion(["probEn", "v-avg"], d, d, variance_scales=[1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="not finite and > 0"):
        F.fusion(["probEn", "v-avg"], d, d, variance_scales=[1.0, 0.0])
    j1 = {"image": ["a"], "boxes": [[[0, 0, 5, 5]]], "scores": [[0.9]], "classes": [[0]], "image_id": [1], "class_logits": [[[]]],
          "probs": [[[0.9, 0.05, 0.03]]], "vars": [[[1.0]]]}
    with pytest.raises(ValueError, match="1 variance scales for 2 detectors"):
        late_fusion([j1, j1], ["probEn", "v-avg"], variance_scales=[2.0])
    with pytest.raises(ValueError, match="2 variance scales for 3 detectors"):
        FramePairPipeline([None, None, None], variance_scales=[1.0, 2.0], concurrent=False)
    import types
    fake = {"scores": types.SimpleNamespace(shape=(1, 4), device="cpu"), "prob_score": types.SimpleNamespace(shape=(1, 4, 3))}
    with pytest.raises(ValueError, match="3 variance scales for 2 detectors"):
        F.pack_rows([fake, fake], variance_scales=[1.0, 2.0, 3.0])
    assert C.scale_j1_vars(j1, 0.5)["vars"] == [[[0.5]]] and j1["vars"] == [[[1.0]]]


# ---- parsing, the file -------------------------------------------------------------------------------------------------------

def test_variance_scales_match_detectors_by_position_or_by_name():
    from proben_amd import calibration as C
    names = ["thermal_only", "early_fusion", "middle_fusion"]
    assert C.parse_variance_scales("0.5,2,1", names) == [0.5, 2.0, 1.0]
    assert C.parse_variance_scales("middle_fusion=1,thermal_only=0.5,early_fusion=2", names) == [0.5, 2.0, 1.0]
    with pytest.raises(ValueError, match="mixes"):
        C.parse_variance_scales("0.5,early_fusion=2,1", names)
    with pytest.raises(ValueError, match="names early_fusion twice"):
        C.parse_variance_scales("thermal_only=0.5,early_fusion=2,early_fusion=3", names)
    with pytest.raises(ValueError, match="no variance scale for middle_fusion"):
        C.parse_variance_scales("thermal_only=0.5,early_fusion=2", names)
    with pytest.raises(ValueError, match="2 values for 3"):
        C.parse_variance_scales("0.5,2", names)
    with pytest.raises(ValueError, match="not finite and > 0"):
        C.parse_variance_scales("0.5,-2,1", names)


def test_calibration_file_round_trips_the_variance_keys_and_a_parent_format_file_has_none(tmp_path):
    from proben_amd import calibration as C
    p = tmp_path / "cal.json"
    C.save(p, {"thermal_only": 1.37, "early_fusion": 0.8125}, {"thermal_only": {"before": 10.5, "after": 9.25}}, {"thermal_only": 1200},
           holdout=0.5, fitted_image_ids=[10, 11])
    parent = json.load(open(p))
    assert C.load_variance(p) is None                                     # the parent's format: nothing to apply
    assert not any(k.startswith("variance") for k in C.load(p))
    C.save_variance(p, {"thermal_only": 0.25, "early_fusion": 3.5}, {"thermal_only": {"before": 5.0, "after": 4.0}}, {"thermal_only": 77},
                    {"thermal_only": 3}, {"thermal_only": {"before": [0.9, 0.99], "after": [0.68, 0.95]}})
    assert C.load_variance(p) == {"thermal_only": 0.25, "early_fusion": 3.5}
    rec = C.load(p)                                                       # load itself is unchanged and keeps extra keys
    assert {k: rec[k] for k in parent} == parent
    assert rec["variance_nll"] == {"thermal_only": {"before": 5.0, "after": 4.0}} and rec["variance_rows"] == {"thermal_only": 77}
    assert rec["variance_excluded"] == {"thermal_only": 3} and rec["variance_coverage"]["thermal_only"]["after"] == [0.68, 0.95]
    assert C.resolve_variance_scales(C.load_variance(p), ["early_fusion", "thermal_only"], "cal.json") == [3.5, 0.25]
    with pytest.raises(ValueError, match="cal.json has no variance scale for middle_fusion"):
        C.resolve_variance_scales(C.load_variance(p), ["thermal_only", "middle_fusion"], "cal.json")
    with pytest.raises(ValueError, match="early_fusion"):
        C.save_variance(p, {"early_fusion": 0.0})
    rec["variance_scales"]["thermal_only"] = -1
    json.dump(rec, open(p, "w"))
    with pytest.raises(ValueError, match="thermal_only"):
        C.load_variance(p)
    (tmp_path / "none.json").write_text("{}")
    with pytest.raises(ValueError, match="not a calibration file"):
        C.save_variance(tmp_path / "none.json", {"a": 1.0})


def test_cli_flags():
    from proben_amd.opt import config_parser
    from proben_amd.cli import fit_temperature
    assert config_parser([]).variance_scales is None
    a = config_parser(["--variance_scales", "0.5,2", "--calibration", "c.json"])
    assert a.variance_scales == "0.5,2" and a.calibration == "c.json"
    b = fit_temperature.parse(["--predictions", "a.json", "--dataset_path", "d"])
    assert b.with_variance is False and b.bbox_reg_weights == [10.0, 10.0, 5.0, 5.0]
    b = fit_temperature.parse(["--predictions", "a.json", "--dataset_path", "d", "--with-variance", "--bbox_reg_weights", "1,1,1,1"])
    assert b.with_variance is True and b.bbox_reg_weights == [1.0, 1.0, 1.0, 1.0]
    with pytest.raises(SystemExit):
        fit_temperature.parse(["--predictions", "a.json", "--dataset_path", "d", "--bbox_reg_weights", "1,1,0,1"])


# ---- the closed form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s_true", [0.25, 1.0, 4.0])
def test_closed_form_minimises_the_restated_nll_and_recovers_the_scale(s_true):
    """s_hat = sum q / (4 n) is the stationary point of NLL(s) = 0.5 (4 n log s + 4 sum log var + sum q / s), a minimum: the NLL at
    s_hat (1 +- 1e-3) is larger.  And the restatement alone passes the recovery check of the GPU test: 4 n s_hat / s_true is
    chi-square with 4 n degrees of freedom, so |s_hat / s_true - 1| <= 5 sqrt(2 / (4 n)); coverage after the fit within 5 binomial
    standard errors of 0.6827 / 0.9545."""
    rng = np.random.default_rng(int(s_true * 100) + 7)
    n = 50_000
    det, gt, var = gaussian_rows(rng, n, s_true)
    m, sq, sl, _, _, bad, _, _ = np_stats(det, np.arange(n), gt, var)
    assert m == n and len(bad) == 0
    s_hat = sq / (4 * m)
    f = np_nll(m, sq, sl, s_hat)
    assert np_nll(m, sq, sl, s_hat * (1 + 1e-3)) > f and np_nll(m, sq, sl, s_hat * (1 - 1e-3)) > f
    assert abs(s_hat / s_true - 1) <= 5 * math.sqrt(2 / (4 * n)), s_hat
    _, _, _, c1, c2, _, _, _ = np_stats(det, np.arange(n), gt, var, s_hat)
    for c, p in ((c1, 0.682689492137086), (c2, 0.954499736103642)):
        assert abs(c / (4 * n) - p) <= 5 * math.sqrt(p * (1 - p) / (4 * n)), (c / (4 * n), p)


# ---- what a scale does to v-avg ----------------------------------------------------------------------------------------------

def _two_detector_rows(rng, n=12):
    base = np.stack([rng.uniform(50, 400, n), rng.uniform(50, 300, n)], 1)       # away from 0: the bound below is relative
    wh = rng.uniform(40, 120, (n, 2))
    boxes = []
    for _ in range(2):
        j = rng.normal(0, 3.0, (n, 4))
        boxes.append(np.concatenate([base, base + wh], 1) + j)
    cls = rng.integers(0, 3, n)
    probs = []
    for _ in range(2):
        p = rng.uniform(0.02, 0.1, (n, 3))
        p[np.arange(n), cls] = rng.uniform(0.6, 0.8, n)
        probs.append(p)
    var = [10.0 ** rng.uniform(-3, -1, n) for _ in range(2)]
    return boxes, cls, probs, var


def _oracle_vavg(boxes, cls, probs, var, scales):
    from oracle import proben as O
    b = np.concatenate(boxes)
    p = np.concatenate(probs)
    c = np.concatenate([cls, cls]).astype(np.float64)
    s = p[np.arange(len(c)), c.astype(int)]
    v = np.concatenate([var[0] * scales[0], var[1] * scales[1]])
    return O.nms_bayesian(b, s, c, p, v, 0.5, "probEn", "v-avg")


def test_oracle_vavg_ignores_a_common_scale_and_follows_unequal_ones():
    rng = np.random.default_rng(2024)
    rows = _two_detector_rows(rng)
    keep0, s0, b0, c0 = _oracle_vavg(*rows, (1.0, 1.0))
    assert len(keep0) < 24, "the case needs clusters of two"
    for c in (0.125, 3.0, 1e3):
        keep, s, b, cl = _oracle_vavg(*rows, (c, c))
        np.testing.assert_array_equal(keep, keep0)
        np.testing.assert_array_equal(s, s0)
        # the weights 1 / (c var) all carry the factor 1 / c, which cancels in sum(w b) / sum(w) up to the roundings of c * var, the
        # reciprocal, the products and the sums: a few 2^-53 relative on coordinates of a few hundred pixels
        np.testing.assert_allclose(b, b0, rtol=16 * 2.0 ** -53, atol=0)
    keep, s, b, cl = _oracle_vavg(*rows, (0.25, 4.0))
    np.testing.assert_array_equal(keep, keep0)
    np.testing.assert_array_equal(s, s0)                  # scores and classes do not see the variances
    assert np.abs(b - b0).max() > 1e-3, "unequal scales must move the v-avg boxes"
