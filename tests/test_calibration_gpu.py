"""Temperature calibration on the GPU: the float64 softmax of pe_proben_pack_logits / pe_calibrated_softmax against NumPy, ProbEn on the
calibrated rows against the oracle on exactly those rows, pack parity with pe_proben_pack_detections, the fit, and the drivers end to
end (save_predictions x 2 -> fit_temperature -> demo_probEn --calibration, two-stage and --one-pass)."""
import json

import numpy as np
import pytest
import torch

from fuse_inputs import detector_rows, logit_rows, weights, write_flir
from fuse_ref import U

pytestmark = pytest.mark.gpu


def _np_softmax(lg32, T):
    z = lg32.astype(np.float64) / T
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


@pytest.mark.parametrize("K", [3, 80])
@pytest.mark.parametrize("T", [0.25, 1.0, 1.7, 8.0])
def test_calibrated_probs_against_numpy_float64(K, T):
    """calibrated_probs (K = 3: lane groups of 4 with xor-butterfly max / sum; K = 80: the serial form) against NumPy's float64
    softmax(logits.astype(f64) / T) on 10^5 rows.

    Bound, derived (u = 2^-53, first order).  z_k = l_k / T, m = max z and z_k - m are single IEEE operations on the same operands on
    both sides: identical.  Each side's e_k = exp(z_k - m) is within 1 ulp of the true value, a relative error <= 2u.  Each side's sum S
    of the K + 1 positive e_j carries the weighted error of its terms (<= 2u) and K additions, each rounding a partial sum <= S
    (<= K u, whatever the order: the device adds over a butterfly or left to right, NumPy pairwise).  The division adds u.  So either
    side is within (2 + 2 + K + 1) u = (K + 5) u of the true p_k, and the two differ by at most 2 (K + 5) u relative (+ 1e-3 of
    that for the second-order terms): 16 u at K = 3, 170 u at K = 80.  The smallest p here is exp(-480): no subnormals.
    Measured on an MI355X (max relative difference): 5.8 u at K = 3, 14.6 u at K = 80 over the four temperatures; the device's
    float64 exp needs no allowance beyond the 1 ulp the derivation gives it."""
    from proben_amd.calibration import calibrated_probs
    rng = np.random.default_rng(100 * K + int(T * 100))
    lg = logit_rows(rng, 100_000, K)
    p, bg = calibrated_probs(torch.from_numpy(lg).cuda(), T)
    got = np.concatenate([p.cpu().numpy(), bg.cpu().numpy()[:, None]], 1)
    want = _np_softmax(lg, T)
    assert got.dtype == np.float64 and got.shape == want.shape
    rel = np.abs(got - want) / want
    bound = 2 * (K + 5) * U * (1 + 1e-3)
    print(f"K={K} T={T}: max relative difference {rel.max() / U:.2f} u (bound {bound / U:.2f} u), smallest p {want.min():.3e}")
    assert rel.max() <= bound, (rel.max() / U, bound / U)
    # ranking: the float32 argmax over the foreground columns stays the calibrated argmax (ties: the first, on both sides)
    cls = lg[:, :K].argmax(1)
    np.testing.assert_array_equal(got[:, :K].argmax(1), cls)
    # sums to one within the K + 1 roundings of the check's own sum and the (K + 5) u of each term
    assert np.abs(got.sum(1) - 1.0).max() <= (2 * K + 6) * U * 2


def test_non_finite_logits_give_nan_rows_like_numpy():
    from proben_amd.calibration import calibrated_probs
    lg = np.array([[1.0, 2.0, 3.0, 4.0], [np.nan, 0.0, 0.0, 0.0], [np.inf, 0.0, 0.0, 0.0], [-np.inf, 0.0, 1.0, 2.0],
                   [-np.inf, -np.inf, -np.inf, -np.inf]], np.float32)
    for K1 in (4, 70):
        rows = np.concatenate([lg, np.zeros((5, K1 - 4), np.float32)], 1) if K1 > 4 else lg
        rows[4] = -np.inf
        p, bg = calibrated_probs(torch.from_numpy(rows).cuda(), 1.5)
        got = np.concatenate([p.cpu().numpy(), bg.cpu().numpy()[:, None]], 1)
        with np.errstate(invalid="ignore"):
            want = _np_softmax(rows, 1.5)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and np.isnan(got[4]).all() and got[3, 0] == 0.0
        np.testing.assert_allclose(got[[0, 3]], want[[0, 3]], rtol=2 * (K1 + 4) * U * 1.001, atol=0)


def _f32_softmax_bound(lg):
    """Per-element relative bound r_k of the box head's float32 softmax against the float64 softmax of the same logits, as
    tests/test_ops_gpu.py::test_boxhead_softmax_against_float64_at_saturation derives it (u = 2^-24): |dx_k| + 2u + sum_j (e_j / S)
    (|dx_j| + 2u) + sum_i |partial_i| u / S + u."""
    u = 2.0 ** -24
    l64 = lg.astype(np.float64)
    x32 = (lg - lg.max(1, keepdims=True)).astype(np.float32)
    dx = np.abs(x32.astype(np.float64) - (l64 - l64.max(1, keepdims=True)))
    e32 = np.exp(x32.astype(np.float64)).astype(np.float32)
    part = np.zeros(len(lg), np.float32)
    round_sum = np.zeros(len(lg))
    for k in range(lg.shape[1]):
        part = (part + e32[:, k]).astype(np.float32)
        round_sum += np.abs(part.astype(np.float64)) * u
    S = part.astype(np.float64)
    wsum = ((e32.astype(np.float64) / S[:, None]) * (dx + 2 * u)).sum(1)
    return dx + 2 * u + (wsum + round_sum / S + u)[:, None]


def _live(det, key):
    cnt = det["counts"].cpu().numpy()
    return np.concatenate([det[key][n, :cnt[n]].cpu().numpy() for n in range(len(cnt))])


def test_at_T_1_the_calibrated_rows_are_the_detectors_prob_score_within_the_float32_bound():
    """p(T = 1) is the float64 softmax of the detector's logits; its prob_score is the float32 one.  Per element they differ by at most
    the float32 bound of tests/test_ops_gpu.py (r_k p_k / ulp32(p_k) + 1e-3 ulps of float32) plus the float64 side's own (K + 5) u."""
    from proben_amd.calibration import calibrated_probs
    for det in detector_rows(3):
        lg, pr = _live(det, "class_logits"), _live(det, "prob_score").astype(np.float64)
        p, _ = calibrated_probs(torch.from_numpy(lg).cuda(), 1.0)
        p = p.cpu().numpy()
        r = _f32_softmax_bound(lg)[:, :3]
        ulp = np.exp2(np.maximum(np.floor(np.log2(p)), -126.0) - 23.0)
        err = np.abs(pr - p) / ulp
        bound = r * p / ulp + 1e-3 + 8 * U * p / ulp
        print(f"{len(lg)} rows: max |prob_score - p(T=1)| {err.max():.3f} ulp32")
        assert (err <= bound).all(), (err.max(), bound[np.unravel_index(np.argmax(err - bound), err.shape)])


@pytest.mark.parametrize("temps", [(1.5, 0.8), (1.0, 1.0), (0.3, 7.0)])
def test_pack_parity_with_pack_detections(temps):
    """Everything but probabilities and scores is pe_proben_pack_detections' output, bit for bit; probabilities and scores are
    calibrated_probs of the same logits, bit for bit (one row arithmetic)."""
    from proben_amd import fusion as F
    from proben_amd.calibration import calibrated_probs
    dets = detector_rows(3)
    ref = F.pack_rows(dets, 2)
    got = F.pack_rows(dets, 2, temps)
    torch.cuda.synchronize()
    cnt = ref[6].cpu().numpy()
    S = len(dets) * dets[0]["scores"].shape[1]
    live = (np.arange(S)[None] < cnt[:, None]).reshape(-1)
    assert live.sum() > 20
    for i in (5, 6, 7):                     # offsets, counts, single-source flags
        assert torch.equal(ref[i], got[i])
    for i in (0, 3, 4):                     # boxes, vars, classes
        assert torch.equal(ref[i][live], got[i][live])
    # rows in detector order: detector d's live rows of image b follow detector d-1's
    want_p, want_s = [], []
    for b in range(len(cnt)):
        for d, T in zip(dets, temps):
            c = int(d["counts"][b])
            lg, cls = d["class_logits"][b, :c], d["classes"][b, :c].long()
            keep = cls <= 2
            p, bg = calibrated_probs(lg[keep], T) if int(keep.sum()) else (torch.zeros((0, 3), dtype=torch.float64, device="cuda"),) * 2
            want_p.append(p)
            want_s.append(p.gather(1, cls[keep, None])[:, 0] if int(keep.sum()) else p[:, 0])
    assert torch.equal(got[2][live], torch.cat(want_p))
    assert torch.equal(got[1][live], torch.cat(want_s))


@pytest.mark.parametrize("temps", [(1.5, 0.8), (1.0, 1.0)])
@pytest.mark.parametrize("method,K", [(("probEn", "v-avg"), 3), (("avg", "s-avg"), 3), (("max", "argmax"), 3), (("probEn_binary", "v-avg"), 1)],
                         ids=lambda v: "/".join(v) if isinstance(v, tuple) else str(v))
def test_fusion_of_the_calibrated_rows_is_the_oracles(method, K, temps):
    """The rows pe_proben_pack_logits wrote are downloaded and fused by oracle.proben image by image; pe_proben_fuse_batch fuses the
    device rows, under both clustering forms (bit matrices at the detectors' bound, the sequential walk at max_rows = 1100).  The
    standard of tests/test_proben_real_rows_gpu.py: same rows per frame, same classes, NaN scores in the same places, finite scores to
    1e-6, the same float32 boxes (parity_map.fused_rows_mismatch); keep / counts identical between the two forms."""
    from oracle import proben as O
    from parity_map import fused_rows_mismatch
    from proben_amd import fusion as F
    dets = detector_rows(K)
    B, D = dets[0]["scores"].shape
    S = 2 * D
    ob, os_, op, ov, oc, ooff, ocnt, osingle = F.pack_rows(dets, 2, temps)
    cnt, single = ocnt.cpu().numpy(), osingle.cpu().numpy()
    hb, hs, hp, hv, hc = (t.cpu().numpy() for t in (ob, os_, op, ov, oc))
    ora = []
    for b in range(B):
        sl = slice(b * S, b * S + cnt[b])
        if cnt[b] == 0:
            continue
        if single[b]:
            bx, sc, cl = hb[sl], hs[sl].astype(np.float32), hc[sl].astype(np.float32)
        else:
            info = {"bbox": hb[sl], "score": hs[sl], "class": hc[sl], "prob": hp[sl], "vars": hv[sl]}
            empty = {"bbox": np.zeros((0, 4)), "score": np.zeros(0), "class": np.zeros(0), "prob": np.zeros((0, K)), "vars": np.zeros(0)}
            bx, sc, cl = O.fusion(list(method), info, empty)
        bx = np.asarray(bx, dtype=np.float64).astype(np.float32).reshape(-1, 4)
        ora += [[b, *bx[j], sc[j], cl[j]] for j in range(len(sc))]
    ora = np.asarray(ora, dtype=np.float32).reshape(-1, 7)
    assert len(ora) > 0 and ((single == 0) & (cnt > 0)).sum() >= 1, "the case needs images where both detectors fired"

    def rows(fused):
        c, bx, sc, cl = fused["counts"].cpu().tolist(), fused["boxes"].float().cpu().numpy(), fused["scores"].cpu().numpy(), fused["classes"].cpu().numpy()
        return np.asarray([[b, *bx[b * S + j], sc[b * S + j], cl[b * S + j]] for b in range(B) for j in range(c[b])], dtype=np.float32).reshape(-1, 7)

    if method == ("max", "argmax"):
        hip = F.fuse_detections(dets, method[0], method[1], temperatures=temps)
        c = hip["counts"].cpu().tolist()
        bx, sc, cl = hip["boxes"].float().cpu().numpy(), hip["scores"].cpu().numpy(), hip["classes"].cpu().numpy()
        got = np.asarray([[b, *bx[b * S + j], sc[b * S + j], cl[b * S + j]] for b in range(B) for j in range(c[b])], dtype=np.float32).reshape(-1, 7)
        assert fused_rows_mismatch(ora, got) is None, fused_rows_mismatch(ora, got)
        return
    outs = [F.fuse_batch(ob, os_, op, ov, oc, ooff, method[0], method[1], max_rows=mr, row_counts=ocnt, passthrough=osingle) for mr in (S, 1100)]
    for out in outs:
        mm = fused_rows_mismatch(ora, rows(out))
        assert mm is None, (method, temps, mm)
    assert torch.equal(outs[0]["counts"], outs[1]["counts"])
    live = (np.arange(S)[None] < outs[0]["counts"].cpu().numpy()[:, None]).reshape(-1)
    assert torch.equal(outs[0]["keep"][live], outs[1]["keep"][live])
    # and the pipeline's own call is the bit-matrix launch
    via = F.fuse_detections(dets, method[0], method[1], temperatures=temps)
    assert torch.equal(via["counts"], outs[0]["counts"]) and torch.equal(via["scores"][live], outs[0]["scores"][live])
    assert torch.equal(via["boxes"][live], outs[0]["boxes"][live])


def test_pipeline_with_temperatures_calls_the_calibrated_pack():
    """FramePairPipeline(temperatures=...) == fuse_detections(..., temperatures) on its own detections; None == the plain route."""
    import proben_amd
    from proben_amd import fusion as F
    from proben_amd.pipeline import FramePairPipeline
    from proben_amd.synthetic import synthetic_images
    models = []
    for seed in (1, 2):
        cfg = proben_amd.get_cfg()
        cfg.MODEL.RESNETS.DEPTH = 50
        cfg.MODEL.ROI_BOX_HEAD.OUTPUT_LOGITS = True
        cfg.MODEL.ROI_HEADS.ENABLE_GAUSSIANNLLOSS = True
        cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 3, 0.5
        cfg.MODEL.WEIGHTS = f"synthetic://{seed}"
        models.append(proben_amd.DefaultPredictor(cfg).model)
    fr = torch.from_numpy(synthetic_images(4, height=256, width=320, seed=5)).cuda()
    for temps in (None, (1.5, 0.8)):
        pipe = FramePairPipeline(models, temperatures=temps)
        dets, fused = pipe([fr, fr], [(256, 320)] * 4, (800, 1000))
        torch.cuda.synchronize()
        want = F.fuse_detections(dets) if temps is None else F.fuse_detections(dets, temperatures=temps)
        torch.cuda.synchronize()
        n = int(want["counts"].sum())
        assert n > 0 and torch.equal(fused["counts"], want["counts"])
        live = (torch.arange(fused["stride"], device="cuda")[None] < want["counts"][:, None]).reshape(-1)
        assert torch.equal(fused["scores"][live], want["scores"][live]) and torch.equal(fused["boxes"][live], want["boxes"][live])


# ---- the fit --------------------------------------------------------------------------------------------------------------------

def _np_nll(lg32, y, T):
    """(nll, d nll / d log T, sum of |row terms| of each) in float64."""
    z = lg32.astype(np.float64) / T
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1)
    zy = z[np.arange(len(y)), y] - m[:, 0]
    nll_i = np.log(s) - zy
    d_i = zy - (e * (z - m)).sum(1) / s
    return nll_i.sum(), d_i.sum(), np.abs(nll_i).sum(), np.abs(d_i).sum()


@pytest.mark.parametrize("T0", [0.5, 2.0, 3.5])
def test_fit_recovers_the_temperature_within_its_statistical_error(T0):
    """Labels are drawn from softmax(logits / T0) of the very float32 logits the fitter sees, so T0 is the true parameter and the fit
    is its maximum-likelihood estimate in x = log T.  Per row d nll_i / dx = z_y - sum_k p_k z_k has variance Var_p(z) over the label,
    so the Fisher information of the sample is I = sum_i Var_{p_i}(z_i) at T0 and the estimator's standard error sigma = I^-1/2;
    |T - T0| / T0 = |x - x0| (first order) must be within 5 sigma.  Nothing here is tuned to the outcome."""
    from proben_amd.calibration import fit_temperature, temperature_nll
    M, K = 200_000, 3
    rng = np.random.default_rng(int(T0 * 10))
    lg = (rng.normal(0.0, 2.0, (M, K + 1)) * T0).astype(np.float32)
    p = _np_softmax(lg, T0)
    y = (rng.random(M)[:, None] > np.cumsum(p, 1)).sum(1).clip(0, K).astype(np.int32)
    z = lg.astype(np.float64) / T0
    var = (p * z * z).sum(1) - (p * z).sum(1) ** 2
    sigma = 1.0 / np.sqrt(var.sum())
    dl, dy = torch.from_numpy(lg).cuda(), torch.from_numpy(y).cuda()
    fit = fit_temperature(dl, dy)
    print(f"T0={T0}: T={fit['T']:.6f}, |T-T0|/T0={abs(fit['T'] - T0) / T0:.2e}, sigma={sigma:.2e}, rounds={fit['rounds']}, "
          f"bracket dnll {fit['bracket_dnll']}, nll {fit['nll_at_1']:.3f} -> {fit['nll']:.3f}")
    assert fit["at_bound"] is None and fit["rows"] == M
    assert abs(fit["T"] - T0) / T0 <= 5 * sigma, (fit["T"], sigma)
    # the derivative changes sign inside the final bracket, which holds T and is narrower than 1e-6 in log T
    lo, hi = fit["bracket"]
    assert lo <= fit["T"] <= hi and np.log(hi / lo) < 1e-6
    assert fit["bracket_dnll"][0] < 0 <= fit["bracket_dnll"][1], fit["bracket_dnll"]
    # no smaller NLL a step away
    near, _ = temperature_nll(dl, dy, [fit["T"] * np.exp(-1e-3), fit["T"], fit["T"] * np.exp(1e-3)])
    assert near[1] <= near[0] and near[1] <= near[2], near
    assert fit["nll"] <= fit["nll_at_1"]
    # NLL and derivative against NumPy float64: relative 1e-12 sqrt(M) of the sum of the rows' absolute terms (for the NLL, whose
    # terms are positive, that is the relative error of the sum itself; the derivative cancels to ~0 at the optimum, so its error is
    # measured against what was added up)
    ts = [0.3, 1.0, T0, fit["T"], 9.0]
    nll, dn = temperature_nll(dl, dy, ts)
    for t, a, b in zip(ts, nll, dn):
        wn, wd, an, ad = _np_nll(lg, y, t)
        tol = 1e-12 * np.sqrt(M)
        print(f"  T={t:.4f}: nll rel err {abs(a - wn) / an:.2e}, dnll rel err {abs(b - wd) / ad:.2e} (tol {tol:.1e})")
        assert abs(a - wn) <= tol * an and abs(b - wd) <= tol * ad, (t, a, wn, b, wd)
    # the same bits on a second call
    nll2, dn2 = temperature_nll(dl, dy, ts)
    assert nll.tobytes() == nll2.tobytes() and dn.tobytes() == dn2.tobytes()


def test_fit_reports_a_minimum_on_the_search_range_and_bad_labels():
    from proben_amd.calibration import fit_temperature, temperature_nll
    rng = np.random.default_rng(3)
    lg = rng.normal(0, 1, (5000, 4)).astype(np.float32)
    y = lg.argmax(1).astype(np.int32)               # always right: the NLL falls all the way to T -> 0
    dl, dy = torch.from_numpy(lg).cuda(), torch.from_numpy(y).cuda()
    fit = fit_temperature(dl, dy)
    assert fit["at_bound"] == "lo" and abs(fit["T"] - 0.05) < 1e-12
    fit = fit_temperature(dl, torch.from_numpy(rng.integers(0, 4, 5000).astype(np.int32)).cuda(), hi=3.0)
    assert fit["at_bound"] == "hi" and abs(fit["T"] - 3.0) < 1e-12      # labels independent of the logits: T -> inf
    y[17], y[4000] = 4, -1
    with pytest.raises(ValueError, match=r"2 of 5000 rows have a label outside \[0, 3\] \(row 4000"):
        temperature_nll(dl, torch.from_numpy(y).cuda(), [1.0, 2.0])


# ---- end to end -----------------------------------------------------------------------------------------------------------------

def test_drivers_end_to_end(tmp_path, capsys):
    from proben_amd import calibration as C
    from proben_amd.cli import demo_probEn, fit_temperature, save_predictions
    root = tmp_path / "val"
    write_flir(root, 6, 96, 120, (150, 180))
    names = ["thermal_only", "early_fusion"]
    paths = [weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
    pdir = tmp_path / "pred"
    for m, p in zip(names, paths):
        save_predictions.main(["--dataset_path", str(root), "--fusion_method", m, "--model_path", p, "--prediction_path", str(pdir), "--batch", "4"])
    files = [str(pdir / f"val_{m}_predictions.json") for m in names]

    def two_stage(tag, extra):
        out = tmp_path / f"out2_{tag}"
        res = demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names),
                                "--outfolder", str(out), "--dataset_name", f"flir_cal2_{tag}"] + extra)
        return out, res

    plain_out, plain = two_stage("plain", [])
    assert "temperatures" not in plain
    cal = tmp_path / "calibration.json"
    fit_temperature.main(["--predictions", *files, "--dataset_path", str(root), "--holdout", "0.5", "--out", str(cal)])
    printed = capsys.readouterr().out
    rec = C.load(cal)
    assert set(rec["detectors"]) == set(names) and rec["fitted_image_ids"] == [10, 11, 12] and rec["holdout"] == 0.5
    for m in names:
        assert f"{m}: T = " in printed and rec["nll"][m]["after"] <= rec["nll"][m]["before"] and rec["rows"][m] > 0
    T = [rec["detectors"][m] for m in names]
    out2, res2 = two_stage("cal", ["--calibration", str(cal)])
    assert "were used to fit the temperatures" in capsys.readouterr().out
    assert res2["temperatures"] == dict(zip(names, T))
    pdir1, out1 = tmp_path / "pred1", tmp_path / "out1_cal"
    res1 = demo_probEn.main(["--one-pass", "--dataset_path", str(root), "--detectors", ",".join(names), "--model_paths", ",".join(paths),
                             "--workers", "2", "--batch", "4", "--write-predictions", "--prediction_path", str(pdir1),
                             "--outfolder", str(out1), "--dataset_name", "flir_cal1", "--calibration", str(cal)])
    assert res1["temperatures"] == res2["temperatures"]
    for m in names:
        f = f"val_{m}_predictions.json"
        assert (pdir1 / f).read_bytes() == (pdir / f).read_bytes(), f
    # the evaluation file, byte for byte.  The evaluator's dump of its input rows (coco_instances_results.json) is not one of the
    # routes' outputs to compare bytewise: the two-stage driver hands the fused boxes over as float32 Instances, the one-pass route as
    # float64 rows, with or without temperatures (tests/test_stream_gpu.py compares them to 1e-6 for that reason).  Ids, categories and
    # the calibrated scores in it are identical.
    assert (out1 / "FLIR_probEn_eval.json").read_bytes() == (out2 / "FLIR_probEn_eval.json").read_bytes()
    r1, r2 = json.load(open(out1 / "coco_instances_results.json")), json.load(open(out2 / "coco_instances_results.json"))
    assert len(r1) == len(r2) > 0
    assert [(r["image_id"], r["category_id"], r["score"]) for r in r1] == [(r["image_id"], r["category_id"], r["score"]) for r in r2]
    np.testing.assert_allclose([r["bbox"] for r in r1], [r["bbox"] for r in r2], rtol=1e-6, atol=1e-4)
    # the calibrated run is another result than the plain one (T != 1), by position or by name the same as by file
    rp = json.load(open(plain_out / "coco_instances_results.json"))
    assert [r["score"] for r in rp] != [r["score"] for r in r2]
    out3, res3 = two_stage("pos", ["--temperatures", ",".join(repr(t) for t in T)])
    out4, res4 = two_stage("name", ["--temperatures", ",".join(f"{m}={t!r}" for m, t in reversed(list(zip(names, T))))])
    for o in (out3, out4):
        assert (o / "coco_instances_results.json").read_bytes() == (out2 / "coco_instances_results.json").read_bytes()
    # without the flag nothing moved: the same bytes as the run made before any calibration
    again_out, again = two_stage("again", [])
    for f in ("FLIR_probEn_eval.json", "coco_instances_results.json"):
        assert (again_out / f).read_bytes() == (plain_out / f).read_bytes(), f
    # a file without logits is refused by name
    d = json.load(open(files[0]))
    d["class_logits"] = [[[] for _ in rows] for rows in d["boxes"]]
    json.dump(d, open(files[0], "w"))
    with pytest.raises(ValueError, match=r"val_thermal_only_predictions\.json: no class_logits"):
        two_stage("nologits", ["--calibration", str(cal)])
