"""Reliability statistics without a GPU: the two entry points are exported, declared and bound and check their arguments before any
device work; a NumPy float64 restatement of the binning (tests/test_reliability_gpu.py imports it); the host arithmetic of
calibration.summarise_reliability on hand cases; the recovery inputs of the GPU test, shown here to be satisfiable; and the report
driver's parsing and refusals."""
import functools
import json
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pe_reliability_logits", "pe_reliability_scores")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.lib()


def _err(L):
    return L.pe_last_error().decode()


# ---- NumPy float64 restatements (tests/test_reliability_gpu.py imports them) -------------------------------------------------

def np_softmax(logits, T):
    """softmax(logits / T) in float64, the expression of csrc/softmax_row.h (used where the device's own bits are not needed)."""
    z = np.asarray(logits, np.float32).astype(np.float64) / T
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _binned(conf, correct, ok, B):
    """Counts as exact integers, per-bin sums by math.fsum over the terms in the kernel's expression order: bin = min((int)(conf * B),
    B - 1) with one float64 multiply, term = d * d with d = conf - (correct ? 1.0 : 0.0).  Both kinds of term are >= 0, so the sums are
    also the sums of the absolute terms the summation bound needs."""
    conf, correct, ok = np.asarray(conf, np.float64), np.asarray(correct, bool), np.asarray(ok, bool)
    used = np.nonzero(ok)[0]
    c, k = conf[used], correct[used]
    bins = np.minimum((c * np.float64(B)).astype(np.int64), B - 1)
    d = c - np.where(k, 1.0, 0.0)
    term = d * d
    counts = np.zeros((B, 2), np.int64)
    sums = np.zeros((B, 2), np.float64)
    for b in range(B):
        sel = bins == b
        counts[b] = int(sel.sum()), int(k[sel].sum())
        sums[b] = math.fsum(c[sel]), math.fsum(term[sel])
    return {"counts": counts, "sums": sums, "excluded": np.nonzero(~ok)[0], "conf": conf, "correct": correct, "bins": bins}


def np_reliability(p, labels, classes, B):
    """pe_reliability_logits restated over given probabilities p f64 [M, K+1]: classes given - conf = p[class], correct = (label ==
    class); classes None - conf = max_k p_k, the first index that attains it is the prediction.  A label or class outside [0, K] or a
    NaN conf excludes the row."""
    p, labels = np.asarray(p, np.float64), np.asarray(labels)
    M, k1 = p.shape
    ok = (labels >= 0) & (labels < k1)
    with np.errstate(invalid="ignore"):
        if classes is not None:
            classes = np.asarray(classes)
            ok &= (classes >= 0) & (classes < k1)
            pred = classes
            conf = p[np.arange(M), np.where(ok, classes, 0)]
        else:
            conf = p.max(axis=1)                      # NaN propagates
            pred = (p == conf[:, None]).argmax(axis=1)   # the first index among equal maxima
    ok &= ~np.isnan(conf)
    return _binned(conf, pred == labels, ok, B)


def np_reliability_scores(conf, correct, B):
    conf = np.asarray(conf, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (conf >= 0.0) & (conf <= 1.0)
    return _binned(conf, np.asarray(correct) != 0, ok, B)


def np_figures(counts, sums):
    """(ece, mce, brier, N) of the restatement, in float64, written independently of calibration.summarise_reliability."""
    n, k = counts[:, 0].astype(np.float64), counts[:, 1].astype(np.float64)
    N = int(counts[:, 0].sum())
    if N == 0:
        return float("nan"), float("nan"), float("nan"), 0
    live = counts[:, 0] > 0
    gap = np.abs(k[live] / n[live] - sums[live, 0] / n[live])
    return float(np.sum(n[live] / N * gap)), float(gap.max()), float(np.sum(sums[live, 1] / N)), N


# ---- the recovery inputs (shared with the GPU test) --------------------------------------------------------------------------

RECOVERY = {"N": 200_000, "K": 3, "T_true": 1.7, "B": 15, "seed": 20261018, "spread": 4.0}


@functools.lru_cache(maxsize=1)
def recovery_rows():
    """(logits f32 [N, K+1], labels i32 [N]): logits N(0, spread^2), labels drawn from softmax(logits / T_true): at T_true the top-label
    confidence is calibrated by construction, at T_true / 3 it is over-confident and at 3 T_true under-confident."""
    r = RECOVERY
    rng = np.random.default_rng(r["seed"])
    logits = (rng.standard_normal((r["N"], r["K"] + 1)) * r["spread"]).astype(np.float32)
    p = np_softmax(logits, r["T_true"])
    u = rng.random(r["N"])
    labels = np.minimum((np.cumsum(p, axis=1) < u[:, None]).sum(axis=1), r["K"]).astype(np.int32)
    logits.setflags(write=False)
    labels.setflags(write=False)
    return logits, labels


def recovery_bound():
    """A calibrated sample has E[ECE] <= 0.5 sqrt(B / N): per bin E|acc_b - conf_b| <= sqrt(1 / (4 n_b)) (a mean of n_b Bernoulli draws
    around its expectation), so E[ECE] <= sum_b (n_b / N) / (2 sqrt(n_b)) = sum_b sqrt(n_b) / (2 N) <= sqrt(B N) / (2 N) by
    Cauchy-Schwarz over the bins.  The assertion allows three times that."""
    return 1.5 * math.sqrt(RECOVERY["B"] / RECOVERY["N"])


def test_recovery_inputs_separate_the_true_temperature_from_a_wrong_one():
    logits, labels = recovery_rows()
    r = RECOVERY
    ece = {}
    for name, T in (("true", r["T_true"]), ("sharp", r["T_true"] / 3), ("flat", 3 * r["T_true"])):
        ref = np_reliability(np_softmax(logits, T), labels, None, r["B"])
        assert len(ref["excluded"]) == 0
        ece[name] = np_figures(ref["counts"], ref["sums"])[0]
    print("ECE at T_true, T_true / 3, 3 T_true:", ece, "bound", recovery_bound())
    assert ece["true"] <= recovery_bound()
    assert ece["sharp"] > recovery_bound() and ece["flat"] > recovery_bound()


# ---- symbols, bindings, argument checks --------------------------------------------------------------------------------------

def test_new_symbols_are_exported_declared_and_bound(L):
    import proben_amd
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "proben_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\s*\(", hdr), name + " is not declared"
        assert name in proben_amd._lib.SIGNATURES, name + " is not bound"
    assert re.search(r"#define\s+PE_RELIABILITY_MAX_BINS\s+64\b", hdr)
    assert re.search(r"#define\s+PE_RELIABILITY_MAX_BLOCKS\s+1024\b", hdr)
    from proben_amd import calibration as C
    for fn in ("reliability", "reliability_scores", "summarise_reliability"):
        assert callable(getattr(C, fn)), fn
    assert os.path.exists(os.path.join(ROOT, "multimodal-object-detection-via-probabilistic-ensembling_amd", "csrc", "reliability.hip"))


def _logits(L, T=1.0, rows=10, cols=4, bins=15, logits=4096, labels=4096, classes=None, work=4096, counts=4096, sums=4096, flags=4096):
    """pe_reliability_logits with plausible (never dereferenced) pointers: every case here stops at an argument check."""
    return L.pe_reliability_logits(logits, labels, classes, rows, cols, T, bins, work, counts, sums, flags, None)


def _scores(L, rows=10, bins=15, conf=4096, correct=4096, work=4096, counts=4096, sums=4096, flags=4096):
    return L.pe_reliability_scores(conf, correct, rows, bins, work, counts, sums, flags, None)


@pytest.mark.parametrize("bad,shown", [(0.0, "0"), (-1.5, "-1.5"), (float("nan"), "nan"), (float("inf"), "inf")])
def test_bad_temperatures_are_named(L, bad, shown):
    assert _logits(L, T=bad) == -1
    assert "pe_reliability_logits" in _err(L) and shown in _err(L) and "not finite and > 0" in _err(L)


def test_reliability_logits_argument_checks(L):
    for b in (0, 65):
        assert _logits(L, bins=b) == -1 and "pe_reliability_logits" in _err(L) and f"num_bins {b}" in _err(L)
    assert _logits(L, cols=1) == -1 and "pe_reliability_logits" in _err(L) and "num_columns 1" in _err(L)
    assert _logits(L, rows=-3) == -1 and "pe_reliability_logits" in _err(L) and "num_rows -3" in _err(L)
    for kw in ("logits", "labels"):
        assert _logits(L, **{kw: None}) == -1 and "pe_reliability_logits: null pointer (logits / labels)" in _err(L), kw
    for kw in ("work", "counts", "sums", "flags"):
        assert _logits(L, **{kw: None}) == -1 and "pe_reliability_logits: null pointer (workspace" in _err(L), kw
    # no rows: nothing is read, no pointer is needed (classes is optional anyway)
    assert _logits(L, rows=0, logits=None, labels=None, work=None, counts=None, sums=None, flags=None) == 0


def test_reliability_scores_argument_checks(L):
    for b in (0, 65):
        assert _scores(L, bins=b) == -1 and "pe_reliability_scores" in _err(L) and f"num_bins {b}" in _err(L)
    assert _scores(L, rows=-3) == -1 and "pe_reliability_scores" in _err(L) and "num_rows -3" in _err(L)
    for kw in ("conf", "correct"):
        assert _scores(L, **{kw: None}) == -1 and "pe_reliability_scores: null pointer (conf / correct)" in _err(L), kw
    for kw in ("work", "counts", "sums", "flags"):
        assert _scores(L, **{kw: None}) == -1 and "pe_reliability_scores: null pointer (workspace" in _err(L), kw
    assert _scores(L, rows=0, conf=None, correct=None, work=None, counts=None, sums=None, flags=None) == 0


def test_python_layer_refuses_cpu_tensors_and_bad_arguments(L):
    import torch
    import proben_amd
    from proben_amd import calibration as C
    lg, lab = torch.zeros((4, 4)), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(proben_amd._lib.HipLibraryError):
        C.reliability(lg, lab)
    with pytest.raises(proben_amd._lib.HipLibraryError):
        C.reliability_scores(torch.zeros(4, dtype=torch.float64), lab)


# ---- the restatement on rows whose answer is known -----------------------------------------------------------------------------

def test_restatement_bins_edges_ties_and_exclusions():
    p = np.array([[0.5, 0.5], [1.0, 0.0], [0.3, 0.7], [np.nan, np.nan], [0.2, 0.8], [0.6, 0.4]])
    labels = np.array([0, 0, 1, 1, 2, -1])
    top = np_reliability(p, labels, None, 10)
    assert top["excluded"].tolist() == [3, 4, 5]
    assert top["counts"][5].tolist() == [1, 1]              # 0.5 exactly: bin 5; the tie goes to index 0 = the label
    assert top["counts"][9].tolist() == [1, 1]              # conf == 1.0 lands in the last bin
    assert top["counts"][7].tolist() == [1, 1] and int(top["counts"][:, 0].sum()) == 3
    own = np_reliability(p, np.array([0, 0, 1, 1, 1, 1]), np.array([1, 1, 0, 0, 2, -1]), 10)
    assert own["excluded"].tolist() == [3, 4, 5]
    assert own["counts"][5].tolist() == [1, 0] and own["counts"][0].tolist() == [1, 0] and own["counts"][3].tolist() == [1, 0]
    assert own["sums"][5].tolist() == [0.5, 0.25] and own["sums"][3, 1] == 0.3 * 0.3
    sc = np_reliability_scores([0.0, 0.1, 1.0, np.nan, -0.1, 1.5, 0.3], [1, 0, 1, 1, 1, 1, 0], 10)
    assert sc["excluded"].tolist() == [3, 4, 5] and sc["counts"][:, 0].tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 0, 1]
    assert sc["counts"][3].tolist() == [1, 0]               # 0.3 * 10 = 3.0000000000000004 -> bin 3; 0.1 * 10 = 1.0 -> bin 1


# ---- summarise_reliability -----------------------------------------------------------------------------------------------------

def test_summarise_all_rows_in_one_bin():
    from proben_amd.calibration import summarise_reliability
    s = summarise_reliability([[0, 0], [4, 3], [0, 0]], [[0.0, 0.0], [2.0, 0.5], [0.0, 0.0]])
    assert s["rows"] == 4 and s["ece"] == abs(0.75 - 0.5) and s["mce"] == 0.25 and s["brier"] == 0.125
    assert s["bins"][1] == {"count": 4, "correct": 3, "conf_sum": 2.0, "brier_sum": 0.5, "accuracy": 0.75, "confidence": 0.5}
    assert math.isnan(s["bins"][0]["accuracy"]) and math.isnan(s["bins"][2]["confidence"])


def test_summarise_skips_an_empty_bin_and_no_rows_give_nan():
    from proben_amd.calibration import summarise_reliability
    a = summarise_reliability([[2, 1], [0, 0], [2, 2]], [[0.5, 0.25], [0.0, 0.0], [1.5, 0.125]])
    b = summarise_reliability([[2, 1], [2, 2]], [[0.5, 0.25], [1.5, 0.125]])
    assert (a["ece"], a["mce"], a["brier"], a["rows"]) == (b["ece"], b["mce"], b["brier"], b["rows"]) and a["rows"] == 4
    z = summarise_reliability(np.zeros((15, 2), np.int64), np.zeros((15, 2)))
    assert z["rows"] == 0 and all(math.isnan(z[k]) for k in ("ece", "mce", "brier")) and len(z["bins"]) == 15
    with pytest.raises(ValueError, match="do not list the same bins"):
        summarise_reliability(np.zeros((3, 2), np.int64), np.zeros((2, 2)))


def test_summarise_two_bins_in_closed_form():
    """30 rows at confidence 0.2 of which 3 are correct, 10 rows at 0.9 of which 10: ECE = (30 / 40) |0.1 - 0.2| + (10 / 40) |1 - 0.9|
    = 0.1, MCE = 0.1, Brier = (27 * 0.04 + 3 * 0.64 + 10 * 0.01) / 40 = 0.0775."""
    from proben_amd.calibration import summarise_reliability
    s = summarise_reliability([[30, 3], [10, 10]], [[30 * 0.2, 27 * 0.04 + 3 * 0.64], [10 * 0.9, 10 * 0.01]])
    assert abs(s["ece"] - 0.1) <= 1e-15 and abs(s["mce"] - 0.1) <= 1e-15 and abs(s["brier"] - 0.0775) <= 1e-15
    e, m, br, N = np_figures(np.array([[30, 3], [10, 10]]), np.array([[30 * 0.2, 27 * 0.04 + 3 * 0.64], [10 * 0.9, 10 * 0.01]]))
    assert N == 40 and abs(e - s["ece"]) <= 1e-15 and abs(m - s["mce"]) <= 1e-15 and abs(br - s["brier"]) <= 1e-15


# ---- the driver ----------------------------------------------------------------------------------------------------------------

BASE = ["--dataset_path", "d", "--predictions", "val_a_predictions.json", "val_b_predictions.json", "--calibration", "c.json"]


def test_driver_parsing():
    from proben_amd.cli import calibration_report as R
    a = R.parse(BASE)
    assert (a.bins, a.iou, a.on, a.score_fusion, a.box_fusion, a.out) == (15, 0.5, "heldout", "probEn", "v-avg", None)
    a = R.parse(BASE + ["--bins", "64", "--on", "all", "--score_fusion", "probEn-log", "--out", "r.json"])
    assert (a.bins, a.on, a.score_fusion, a.out) == (64, "all", "probEn-log", "r.json")
    for bad in (["--bins", "0"], ["--bins", "65"], ["--on", "validation"], ["--iou", "1.5"]):
        with pytest.raises(SystemExit):
            R.parse(BASE + bad)
    with pytest.raises(SystemExit):
        R.parse(BASE[:3] + ["val_a_predictions.json", "--calibration", "c.json"])        # one file: nothing to fuse


def test_driver_chooses_images_and_refuses_an_empty_choice(tmp_path):
    from proben_amd import calibration as C
    from proben_amd.cli import calibration_report as R
    order = [11, 12, 13, 14, 15, 16]
    assert R.select_images(order, [11, 12, 13], "heldout") == [14, 15, 16]
    assert R.select_images(order, [11, 12, 13], "fitted") == [11, 12, 13]
    assert R.select_images(order, [11, 12, 13], "all") == order
    with pytest.raises(ValueError, match="--on"):
        R.select_images(order, order, "heldout")
    with pytest.raises(ValueError, match="not one of"):
        R.select_images(order, [], "validation")
    # the same refusal from the command line, before any prediction file or the GPU is touched: a file fitted with --holdout 1.0
    root = tmp_path / "val"
    root.mkdir()
    json.dump({"images": [{"id": i, "file_name": f"{i}.jpeg", "height": 8, "width": 8} for i in order], "annotations": [],
               "categories": [{"id": 1, "name": "person"}]}, open(root / "FLIR_thermal_RGBT_pairs_val.json", "w"))
    cal = tmp_path / "cal.json"
    C.save(cal, {"a": 1.2, "b": 0.9}, holdout=1.0, fitted_image_ids=order)
    cmd = ["--dataset_path", str(root), "--predictions", str(tmp_path / "val_a_predictions.json"), str(tmp_path / "val_b_predictions.json"),
           "--calibration", str(cal)]
    with pytest.raises(ValueError, match=r"nothing is held out.*--on fitted / --on all"):
        R.main(cmd)
