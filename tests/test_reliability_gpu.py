"""Reliability statistics on the GPU, through the C-ABI: pe_reliability_logits against pe_calibrated_softmax's own output binned by the
NumPy restatement of tests/test_reliability_cpu.py (counts exact, sums within the first-order bound of a fixed summation order),
bit-for-bit repeatability, pe_reliability_scores, the Python layer, recovery of a known temperature, and the report driver end to end."""
import functools
import json
import math

import numpy as np
import pytest
import torch

from fuse_inputs import weights, write_flir
from fuse_ref import U

pytestmark = pytest.mark.gpu

MAX_BLOCKS, ROWS_PER_BLOCK = 1024, 256          # PE_RELIABILITY_MAX_BLOCKS, the rows per workgroup that size the grid


# ---- raw calls -----------------------------------------------------------------------------------------------------------------

def _outputs(B):
    """Output buffers filled with a pattern, so that an entry the kernels did not write shows."""
    dev = "cuda"
    return (torch.full((B, 2), -7, dtype=torch.int64, device=dev), torch.full((B, 2), float("nan"), dtype=torch.float64, device=dev),
            torch.full((2,), -7, dtype=torch.int32, device=dev), torch.empty((MAX_BLOCKS * B * 4,), dtype=torch.float64, device=dev))


def raw_logits(logits, labels, classes, T, B):
    from proben_amd import _lib
    cnt, sums, flags, work = _outputs(B)
    M, k1 = logits.shape
    st = _lib.lib().pe_reliability_logits(_lib.ptr(logits), _lib.ptr(labels), _lib.ptr(classes), M, k1, float(T), B, _lib.ptr(work),
                                          _lib.ptr(cnt), _lib.ptr(sums), _lib.ptr(flags), _lib.stream())
    _lib.check(st, "pe_reliability_logits")
    return cnt.cpu().numpy(), sums.cpu().numpy(), flags.cpu().numpy()


def raw_scores(conf, correct, B):
    from proben_amd import _lib
    cnt, sums, flags, work = _outputs(B)
    st = _lib.lib().pe_reliability_scores(_lib.ptr(conf), _lib.ptr(correct), conf.numel(), B, _lib.ptr(work), _lib.ptr(cnt), _lib.ptr(sums),
                                          _lib.ptr(flags), _lib.stream())
    _lib.check(st, "pe_reliability_scores")
    return cnt.cpu().numpy(), sums.cpu().numpy(), flags.cpu().numpy()


def device_softmax(logits, T):
    """pe_calibrated_softmax's own output, all K + 1 columns: the reference's confidences are the device's bits."""
    from proben_amd import _lib
    M, k1 = logits.shape
    out = torch.empty((M, k1), dtype=torch.float64, device=logits.device)
    _lib.check(_lib.lib().pe_calibrated_softmax(_lib.ptr(logits), M, k1, float(T), _lib.ptr(out), _lib.stream()), "pe_calibrated_softmax")
    return out.cpu().numpy()


# ---- 1 / 2. counts exact, sums within the summation bound ----------------------------------------------------------------------

K1S, MS, BS, TS = (2, 4, 5, 64, 65), (1, 63, 64, 65, 257, 4097), (1, 10, 15, 64), (0.5, 1.0, 2.5)
# a thinned cross-product: every value of every axis appears, K + 1 = 2 meets B = 10 (the planted p = 0.5), and both the lane-group
# path and the serial path (65) see more than one workgroup; every case runs in both `classes` modes
CASES = [(K1S[i % 5], MS[i % 6], BS[i % 4], TS[i % 3]) for i in range(10)] + [(65, 4097, 15, 1.0), (4, 4097, 64, 2.5)]


def _rows(k1, M, seed):
    """Random rows plus, from 16 rows on, the planted ones.  Returns (logits, labels, classes, planted: {name: row})."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 3.0, (M, k1)).astype(np.float32)
    labels = rng.integers(0, k1, M).astype(np.int32)
    classes = rng.integers(0, k1, M).astype(np.int32)
    planted = {}
    if M >= 16:
        at = iter(rng.choice(M, 10, replace=False).tolist())
        def plant(name, row=None, label=None, cls=None):
            r = planted[name] = next(at)
            if row is not None:
                logits[r] = row
            if label is not None:
                labels[r] = label
            if cls is not None:
                classes[r] = cls
        even = np.zeros(k1, np.float32)
        plant("even", even, 0, 0)                                          # K + 1 = 2: p = 0.5 exactly
        sat = np.full(k1, -200.0, np.float32)
        sat[k1 - 1] = 200.0
        plant("saturated", sat, k1 - 1, k1 - 1)                            # conf == 1.0: the last bin
        tie = np.full(k1, -5.0, np.float32)
        tie[0] = tie[1] = 3.0
        plant("tie, label on the first index", tie, 0, 0)
        plant("tie, label on the second index", tie, 1, 1)                 # top label: index 0 is predicted, so this row is wrong
        bad = rng.normal(0, 1, k1).astype(np.float32)
        bad[k1 // 2] = np.nan
        plant("NaN logit", bad)
        bad = rng.normal(0, 1, k1).astype(np.float32)
        bad[0] = np.inf
        plant("+inf logit", bad)
        plant("label -1", label=-1)
        plant("label K + 1", label=k1)
        plant("class -1", cls=-1)
        plant("class K + 1", cls=k1)
    return logits, labels, classes, planted


@functools.lru_cache(maxsize=None)
def _case(k1, M, B, T, with_classes):
    """(device counts, sums, flags, the restatement over the device's own softmax, planted rows) of one case, computed once."""
    from test_reliability_cpu import np_reliability
    logits, labels, classes, planted = _rows(k1, M, 1000 * k1 + M)
    lg, lab, cls = (torch.from_numpy(a).cuda() for a in (logits, labels, classes))
    got = raw_logits(lg, lab, cls if with_classes else None, T, B)
    ref = np_reliability(device_softmax(lg, T), labels, classes if with_classes else None, B)
    return got, ref, planted, (labels, classes)


@pytest.mark.parametrize("with_classes", [True, False], ids=["own class", "top label"])
@pytest.mark.parametrize("k1,M,B,T", CASES)
def test_counts_are_exact(k1, M, B, T, with_classes):
    (cnt, _, flags), ref, planted, (labels, classes) = _case(k1, M, B, T, with_classes)
    assert cnt.dtype == np.int64 and cnt.shape == (B, 2)
    np.testing.assert_array_equal(cnt, ref["counts"])
    bad = ref["excluded"]
    assert flags.tolist() == [len(bad), int(bad.max()) + 1 if len(bad) else 0]
    assert int(cnt[:, 0].sum()) + len(bad) == M                            # an excluded row is in no bin
    if planted:
        out = {planted[n] for n in ("NaN logit", "+inf logit", "label -1", "label K + 1")}
        if with_classes:
            out |= {planted["class -1"], planted["class K + 1"]}
        assert out <= set(bad.tolist()) and len(bad) == len(out)           # the planted rows and no others
        conf, bins, correct = ref["conf"], dict(zip(np.nonzero(~np.isin(np.arange(M), bad))[0].tolist(), ref["bins"].tolist())), ref["correct"]
        assert conf[planted["saturated"]] == 1.0 and bins[planted["saturated"]] == B - 1 and correct[planted["saturated"]]
        a, b = planted["tie, label on the first index"], planted["tie, label on the second index"]
        assert conf[a] == conf[b] and correct[a] and correct[b] == with_classes      # top label: the first index wins, so b is wrong
        if k1 == 2:
            assert conf[planted["even"]] == 0.5 and bins[planted["even"]] == B // 2 and (B != 10 or bins[planted["even"]] == 5)


def test_the_case_list_covers_every_axis_value_and_the_planted_half():
    assert {c[0] for c in CASES} == set(K1S) and {c[1] for c in CASES} == set(MS) and {c[2] for c in CASES} == set(BS)
    assert {c[3] for c in CASES} == set(TS) and any(c[0] == 2 and c[2] == 10 and c[1] >= 16 for c in CASES)
    assert any(c[0] == 65 and c[1] > ROWS_PER_BLOCK for c in CASES) and any(c[0] <= 64 and c[1] > ROWS_PER_BLOCK for c in CASES)


def _fraction_of_bound(sums, ref):
    """Largest |device sum - fsum| / (1.01 n_b u fsum |terms|) over the bins and the two sums: any fixed order of n_b terms is within
    (n_b - 1) u sum |terms| to first order; the terms themselves are the device's bits (conf from its own softmax, the Brier term two
    lane-local IEEE operations), and both kinds of term are >= 0, so the restatement's sums are the sums of the absolute terms."""
    worst = 0.0
    for b in range(len(sums)):
        n = int(ref["counts"][b, 0])
        for v in range(2):
            want = float(ref["sums"][b, v])
            err = abs(float(sums[b, v]) - want)
            if n == 0 or want == 0.0:
                assert err == 0.0, (b, v, sums[b, v])
                continue
            worst = max(worst, err / (1.01 * n * U * want))
    return worst


@pytest.mark.parametrize("with_classes", [True, False], ids=["own class", "top label"])
@pytest.mark.parametrize("k1,M,B,T", CASES)
def test_sums_are_within_the_summation_bound(k1, M, B, T, with_classes):
    (_, sums, _), ref, _, _ = _case(k1, M, B, T, with_classes)
    assert sums.dtype == np.float64 and sums.shape == (B, 2)
    f = _fraction_of_bound(sums, ref)
    print(f"K+1={k1} M={M} B={B} T={T} classes={with_classes}: largest |sum - fsum| = {f:.4f} of the bound")
    assert f <= 1.0, f


def test_excluded_rows_appended_change_no_bit():
    """4000 clean rows, then the same with 8 rows appended that must be excluded: ceil(rows / 256) is 16 both times, so the partition of
    the clean rows is the same and the appended rows only ever add nothing - counts and sums keep their bytes."""
    logits, labels, classes, _ = _rows(4, 4000, 77)
    for with_classes in (True, False):
        cuda = lambda *a: [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in a]
        lg, lab, cls = cuda(logits, labels, classes)
        base = raw_logits(lg, lab, cls if with_classes else None, 1.3, 15)
        assert int(base[0][:, 0].sum()) + int(base[2][0]) == 4000
        extra = np.zeros((8, 4), np.float32)
        extra[0, 1], extra[1, 2] = np.nan, np.inf
        xl = np.array([0, 0, -1, 4, 1, 1, -5, 9], np.int32)
        xc = np.array([0, 0, 0, 0, -1, 4, 0, 0], np.int32) if with_classes else np.zeros(8, np.int32)
        if not with_classes:
            extra[4:6, 0] = np.nan
        lg2, lab2, cls2 = cuda(np.concatenate([logits, extra]), np.concatenate([labels, xl]), np.concatenate([classes, xc]))
        got = raw_logits(lg2, lab2, cls2 if with_classes else None, 1.3, 15)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
        assert got[2].tolist() == [int(base[2][0]) + 8, 4008]


# ---- 3. the same input twice gives the same bytes ------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [4097, MAX_BLOCKS * ROWS_PER_BLOCK + 301])
def test_same_input_same_bytes(M):
    """Counts, sums and flags, at one size below and one above the grid cap (1024 workgroups of 256 rows)."""
    from test_reliability_cpu import np_reliability, np_reliability_scores
    logits, labels, classes, _ = _rows(4, M, 5)
    lg, lab, cls = (torch.from_numpy(a).cuda() for a in (logits, labels, classes))
    for c in (cls, None):
        a, b = raw_logits(lg, lab, c, 1.7, 15), raw_logits(lg, lab, c, 1.7, 15)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        ref = np_reliability(device_softmax(lg, 1.7), labels, None if c is None else classes, 15)
        np.testing.assert_array_equal(a[0], ref["counts"])                 # and the capped grid still counts every row once
        assert _fraction_of_bound(a[1], ref) <= 1.0
    rng = np.random.default_rng(M)
    conf = rng.random(M)
    conf[::97] = np.nan
    ok = (rng.random(M) < conf).astype(np.int32)
    cf, okt = torch.from_numpy(conf).cuda(), torch.from_numpy(ok).cuda()
    a, b = raw_scores(cf, okt, 15), raw_scores(cf, okt, 15)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    ref = np_reliability_scores(conf, ok, 15)
    np.testing.assert_array_equal(a[0], ref["counts"])
    assert a[2].tolist() == [len(ref["excluded"]), int(ref["excluded"].max()) + 1] and _fraction_of_bound(a[1], ref) <= 1.0


# ---- 4. scores -----------------------------------------------------------------------------------------------------------------

def _score_rows():
    rng = np.random.default_rng(404)
    M = 4097
    conf = rng.random(M)
    correct = (rng.random(M) < conf).astype(np.int32)
    correct[::5] *= 3                                                       # any non-zero value means correct
    at = rng.choice(M, 15, replace=False)
    conf[at[:11]] = np.arange(11) / 10                                      # the bin edges k / B of B = 10, 0.0 and 1.0 included
    conf[at[11]] = 1.0
    conf[at[12:]] = [np.nan, -0.1, 1.5]
    return conf, correct, at


@pytest.mark.parametrize("B", [10, 15])
def test_scores_against_the_restatement(B):
    from test_reliability_cpu import np_reliability_scores
    conf, correct, at = _score_rows()
    cnt, sums, flags = raw_scores(torch.from_numpy(conf).cuda(), torch.from_numpy(correct).cuda(), B)
    ref = np_reliability_scores(conf, correct, B)
    np.testing.assert_array_equal(cnt, ref["counts"])
    assert sorted(ref["excluded"].tolist()) == sorted(at[12:].tolist()) and flags.tolist() == [3, int(at[12:].max()) + 1]
    f = _fraction_of_bound(sums, ref)
    print(f"scores B={B}: largest |sum - fsum| = {f:.4f} of the bound")
    assert f <= 1.0
    if B == 10:
        used = dict(zip(np.nonzero(~np.isin(np.arange(len(conf)), ref["excluded"]))[0].tolist(), ref["bins"].tolist()))
        want = [min(int(np.float64(k / 10) * np.float64(10)), 9) for k in range(11)]       # the kernel's expression: 1.0 lands in bin 9
        assert [used[int(r)] for r in at[:11]] == want and used[int(at[11])] == 9 and want[0] == 0 and want[5] == 5


# ---- 5. the Python layer -------------------------------------------------------------------------------------------------------

def test_python_layer_reports_what_the_restatement_computes():
    """ece, mce, brier within 1e-12 absolute: at most 64 bins, a few roundings each on numbers <= 1, beside the 1e-13 the device sums
    may differ from fsum by at these sizes."""
    from test_reliability_cpu import np_figures, np_reliability, np_reliability_scores
    from proben_amd import calibration as C
    logits, labels, classes, planted = _rows(4, 4097, 9)
    lg, lab, cls = (torch.from_numpy(a).cuda() for a in (logits, labels, classes))
    for c, T, B in ((cls, 1.0, 15), (None, 2.5, 15), (cls.long(), 0.5, 64), (None, 1.0, 1)):
        got = C.reliability(lg, lab.long(), T, c, bins=B)                   # any integer dtype is taken
        ref = np_reliability(device_softmax(lg, T), labels, None if c is None else classes, B)
        e, m, br, N = np_figures(ref["counts"], ref["sums"])
        assert got["rows"] == N and got["excluded"] == len(ref["excluded"]) > 0 and got["last_excluded"] == int(ref["excluded"].max())
        assert abs(got["ece"] - e) <= 1e-12 and abs(got["mce"] - m) <= 1e-12 and abs(got["brier"] - br) <= 1e-12
        assert [b["count"] for b in got["bins"]] == ref["counts"][:, 0].tolist() and [b["correct"] for b in got["bins"]] == ref["counts"][:, 1].tolist()
        assert len(got["bins"]) == B and all(set(b) == {"count", "correct", "conf_sum", "brier_sum", "accuracy", "confidence"} for b in got["bins"])
    conf, correct, _ = _score_rows()
    got = C.reliability_scores(torch.from_numpy(conf).cuda(), torch.from_numpy(correct).cuda() != 0, bins=15)      # a bool verdict too
    ref = np_reliability_scores(conf, correct, 15)
    e, m, br, N = np_figures(ref["counts"], ref["sums"])
    assert got["rows"] == N and got["excluded"] == 3
    assert abs(got["ece"] - e) <= 1e-12 and abs(got["mce"] - m) <= 1e-12 and abs(got["brier"] - br) <= 1e-12
    empty = C.reliability(lg[:0], lab[:0], 1.0, None, bins=15)
    assert empty["rows"] == 0 and empty["excluded"] == 0 and math.isnan(empty["ece"]) and all(b["count"] == 0 for b in empty["bins"])
    with pytest.raises(ValueError, match="bins"):
        C.reliability(lg, lab, 1.0, None, bins=65)
    with pytest.raises(ValueError, match="not finite and > 0"):
        C.reliability(lg, lab, 0.0)
    with pytest.raises(ValueError, match="labels"):
        C.reliability(lg, lab[:5])


# ---- 6. recovery ---------------------------------------------------------------------------------------------------------------

def test_recovery_on_the_device():
    """The inputs and the three inequalities of tests/test_reliability_cpu.py::test_recovery_inputs_separate_..., on the device; and the
    device's ECE within 1e-12 of the restatement's over the device's own softmax."""
    from test_reliability_cpu import RECOVERY as R, np_figures, np_reliability, recovery_bound, recovery_rows
    from proben_amd import calibration as C
    logits, labels = recovery_rows()
    lg, lab = torch.from_numpy(np.array(logits)).cuda(), torch.from_numpy(np.array(labels)).cuda()
    ece = {}
    for name, T in (("true", R["T_true"]), ("sharp", R["T_true"] / 3), ("flat", 3 * R["T_true"])):
        got = C.reliability(lg, lab, T, None, bins=R["B"])
        ref = np_reliability(device_softmax(lg, T), labels, None, R["B"])
        assert got["rows"] == R["N"] and got["excluded"] == 0
        assert abs(got["ece"] - np_figures(ref["counts"], ref["sums"])[0]) <= 1e-12
        ece[name] = got["ece"]
    print("device ECE at T_true, T_true / 3, 3 T_true:", ece, "bound", recovery_bound())
    assert ece["true"] <= recovery_bound()
    assert ece["sharp"] > recovery_bound() and ece["flat"] > recovery_bound()


# ---- 7. the driver -------------------------------------------------------------------------------------------------------------

def test_driver_end_to_end(tmp_path, capsys):
    """save_predictions x 2 -> fit_temperature --holdout 0.5 --with-variance --with-prior -> calibration_report, by the recipe of
    tests/test_variance_gpu.py::test_drivers_end_to_end (the annotations are rewritten from the detections so that rows match)."""
    from proben_amd import calibration as C
    from proben_amd.cli import calibration_report, fit_temperature, save_predictions
    from proben_amd.late_fusion import late_fusion
    root = tmp_path / "val"
    write_flir(root, 6, 96, 120, (150, 180))
    names = ["thermal_only", "early_fusion"]
    paths = [weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
    pdir = tmp_path / "pred"
    for m, p in zip(names, paths):
        save_predictions.main(["--dataset_path", str(root), "--fusion_method", m, "--model_path", p, "--prediction_path", str(pdir), "--batch", "4"])
    files = [str(pdir / f"val_{m}_predictions.json") for m in names]
    preds = [json.load(open(f)) for f in files]
    val = root / "FLIR_thermal_RGBT_pairs_val.json"
    ds = json.load(open(val))
    anns = []
    for i, iid in enumerate(preds[0]["image_id"]):
        for k, p in enumerate(preds):
            if p["boxes"][i]:
                x1, y1, x2, y2 = p["boxes"][i][0]
                anns.append({"id": len(anns) + 1, "image_id": iid, "category_id": 1 + int(p["classes"][i][0]) % 3,
                             "bbox": [x1 + 0.03 * (1 + k) * (x2 - x1), y1 - 0.02 * (y2 - y1), (x2 - x1) * 1.05, (y2 - y1) * 0.97],
                             "area": (x2 - x1) * (y2 - y1), "iscrowd": 0})
    assert anns
    ds["annotations"] = anns
    json.dump(ds, open(val, "w"))
    order = [im["id"] for im in ds["images"]]

    cal, rep = tmp_path / "cal.json", tmp_path / "report.json"
    fit_temperature.main(["--predictions", *files, "--dataset_path", str(root), "--holdout", "0.5", "--out", str(cal), "--with-variance", "--with-prior"])
    rec = json.load(open(cal))
    held = [i for i in order if i not in set(rec["fitted_image_ids"])]
    assert len(held) == 3 and len(rec["fitted_image_ids"]) == 3
    capsys.readouterr()
    base = ["--dataset_path", str(root), "--predictions", *files, "--calibration", str(cal)]
    report = calibration_report.main(base + ["--out", str(rep)])
    printed = capsys.readouterr().out
    assert "NLL/row" in printed and "fused" in printed and "thermal_only" in printed and "a Gaussian" in printed
    on_disk = json.load(open(rep))
    assert set(on_disk) >= {"images", "detectors", "variance", "fused", "bins", "iou"} and on_disk["images"] == held == report["images"]
    assert on_disk["bins"] == 15 and on_disk["iou"] == 0.5 and set(on_disk["detectors"]) == set(names)

    by_id = {im["id"]: [a for a in anns if a["image_id"] == im["id"]] for im in ds["images"]}
    dets_held = []
    for m, p in zip(names, preds):
        idx = [p["image_id"].index(i) for i in held]
        dets_held.append({k: [v[i] for i in idx] for k, v in p.items()})
        logits, classes, labels = [], [], []
        for i in idx:                                                       # the labels by the CPU route of the fit, image by image
            if not p["boxes"][i]:
                continue
            gt = [[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in by_id[p["image_id"][i]]]
            lab = C.match_labels(p["boxes"][i], p["classes"][i], gt, [a["category_id"] - 1 for a in by_id[p["image_id"][i]]], 0.5, num_classes=3)
            lab[(lab < 0) | (lab > 3)] = 3
            logits += p["class_logits"][i]
            classes += p["classes"][i]
            labels += lab.tolist()
        n = len(logits)
        assert n > 0
        lg = torch.tensor(logits, dtype=torch.float32, device="cuda")
        lab, cls = torch.tensor(labels, dtype=torch.int32, device="cuda"), torch.tensor(classes, dtype=torch.int32, device="cuda")
        d = report["detectors"][m]
        for tag, T in (("before", 1.0), ("after", rec["detectors"][m])):
            assert d[tag]["rows"] == n and d[tag]["T"] == T and d[tag]["excluded"] == 0
            for key, c in (("own", cls), ("top_label", None)):
                want = C.reliability(lg, lab, T, c, bins=15)
                got = d[tag] if key == "own" else d[tag]["top_label"]
                assert (got["rows"], got["ece"], got["mce"], got["brier"]) == (want["rows"], want["ece"], want["mce"], want["brier"]), (m, tag, key)
                assert [b["count"] for b in got["bins"]] == [b["count"] for b in want["bins"]]
            nll, _ = C.temperature_nll(lg, lab, [T])
            assert d[tag]["nll"] == float(nll[0]) / n
        v = report["variance"][m]
        for tag, s in (("before", 1.0), ("after", rec["variance_scales"][m])):
            assert v[tag]["scale"] == s and len(v[tag]["coverage"]) == 2 and v[tag]["rows"] > 0 and math.isfinite(v[tag]["nll"])
            assert all(0.0 <= c <= 1.0 for c in v[tag]["coverage"])
    fused_rows = sum(len(r[1]) for r in late_fusion(dets_held, ["probEn", "v-avg"]) if r is not None)
    assert report["fused"]["before"]["rows"] == fused_rows > 0
    assert report["fused"]["after"]["rows"] + report["fused"]["after"]["excluded"] == fused_rows
    for tag in ("before", "after"):
        assert math.isfinite(report["fused"][tag]["ece"]) and 0.0 <= report["fused"][tag]["brier"] <= 1.0

    everything = calibration_report.main(base + ["--on", "all"])
    assert everything["images"] == order and len(everything["images"]) == 6
    assert calibration_report.main(base + ["--on", "fitted"])["images"] == rec["fitted_image_ids"]
    logp = calibration_report.main(base + ["--score_fusion", "probEn-log"])
    assert logp["method"] == ["probEn-log", "v-avg"] and all(math.isfinite(logp["fused"][t]["ece"]) for t in ("before", "after"))
    full = tmp_path / "cal_full.json"
    fit_temperature.main(["--predictions", *files, "--dataset_path", str(root), "--holdout", "1.0", "--out", str(full)])
    with pytest.raises(ValueError, match="--on"):
        calibration_report.main(["--dataset_path", str(root), "--predictions", *files, "--calibration", str(full)])
