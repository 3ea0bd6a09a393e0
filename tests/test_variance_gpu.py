"""Variance calibration on the GPU, through the C-ABI (calibration.py / fusion.py are thin ctypes callers): pe_match_ground_truth against
calibration.match_labels / finetune.pairwise_iou image by image (bit for bit), pe_variance_stats against the NumPy float64
restatement of tests/test_variance_cpu.py within a derived bound, recovery of a known scale, pe_proben_pack_calibrated against the
three pack entry points, v-avg on the scaled variances against the oracle, and the drivers end to end."""
import json
import math

import numpy as np
import pytest
import torch

from fuse_inputs import weights, write_flir
from fuse_ref import U

pytestmark = pytest.mark.gpu


# ---- 1. matching -------------------------------------------------------------------------------------------------------------

def _match_images(rng):
    """List of (det [n,4], gt [g,4], classes [g], crowd [g]) covering the cases of the issue."""
    def rand_image(n_gt, n_det, crowd_p=0.15):
        x, y = rng.uniform(0, 500, n_gt), rng.uniform(0, 400, n_gt)
        gt = np.stack([x, y, x + rng.uniform(5, 150, n_gt), y + rng.uniform(5, 150, n_gt)], 1)
        src = rng.integers(0, n_gt, n_det)
        det = gt[src] + rng.normal(0, 6.0, (n_det, 4))
        far = rng.random(n_det) < 0.2
        det[far] += 1000.0                                         # detections that overlap nothing
        return det, gt, rng.integers(0, 5, n_gt), (rng.random(n_gt) < crowd_p).astype(np.int32)     # classes 3, 4 are outside [0, 3]: passed on

    z4 = np.zeros((0, 4))
    images = [rand_image(7, 30), rand_image(40, 90)]
    images.append((z4, rand_image(5, 1)[1], np.arange(5) % 3, np.zeros(5, np.int32)))                       # no detections
    images.append((rand_image(3, 6)[0], z4, np.zeros(0, np.int64), np.zeros(0, np.int32)))                  # no ground truth
    images.append((z4, z4, np.zeros(0, np.int64), np.zeros(0, np.int32)))                                   # neither
    # a crowd box that would win (the perfect match), and an image whose every box is a crowd box
    images.append((np.array([[0.0, 0, 10, 10]]), np.array([[0.0, 0, 10, 10], [0, 0, 10, 7]]), np.array([0, 2]), np.array([1, 0], np.int32)))
    images.append((np.array([[0.0, 0, 10, 10]]), np.array([[0.0, 0, 10, 10], [0, 0, 10, 7]]), np.array([0, 2]), np.array([1, 1], np.int32)))
    # exactly tied maxima: duplicated ground-truth boxes with different classes, and two halves with IoU 50 / 100 each
    images.append((np.array([[3.0, 4, 50, 60], [0, 0, 10, 10]]),
                   np.array([[100.0, 100, 120, 120], [3, 4, 49, 61], [3, 4, 49, 61], [0, 5, 10, 10], [0, 0, 10, 5], [3, 4, 49, 61]]),
                   np.array([0, 2, 1, 1, 2, 0]), np.zeros(6, np.int32)))
    # IoU exactly at the threshold: inter 8 x 4 = 32, union 32 + 64 - 32 = 64 -> 0.5; one unit less overlap -> 28 / 64 < 0.5
    images.append((np.array([[0.0, 0, 8, 4], [0, 0, 7, 4], [100, 100, 110, 110]]), np.array([[0.0, 0, 8, 8]]), np.array([1]), np.zeros(1, np.int32)))
    # more ground truth than one LDS chunk (512): three chunks, a tie across a chunk boundary (index 100 and 600), the best of some
    # detections in the last chunk; and more detections than one tile of 256 threads
    det, gt, cls, crowd = rand_image(1300, 700, crowd_p=0.05)
    gt[100], gt[1299] = [200.0, 200.0, 300.0, 320.0], [50.0, 60.0, 150.0, 160.0]
    gt[600] = gt[100]
    cls[100], cls[600] = 1, 2
    crowd[100] = crowd[600] = 0
    det[0] = gt[100] + np.array([1.0, 0.5, -1.0, 0.25])
    det[1] = gt[1299] + np.array([0.5, 0.5, 0.5, 0.5])
    crowd[1299] = 0
    images.append((det, gt, cls, crowd))
    images.append(rand_image(2, 300, crowd_p=0.0))
    return images


def _match_reference(det, gt, cls, crowd, thresh, K):
    """(labels by calibration.match_labels; match index and IoU by finetune.pairwise_iou, the lowest index among equal maxima)."""
    from proben_amd.calibration import match_labels
    from proben_amd.finetune import pairwise_iou
    n = len(det)
    labels = match_labels(det, [0] * n, gt, cls, thresh, gt_crowd=crowd, num_classes=K).numpy()
    match, best = np.full(n, -1, np.int32), np.zeros(n)
    live = np.nonzero(np.asarray(crowd) == 0)[0]
    if n and len(live):
        iou = pairwise_iou(torch.from_numpy(np.asarray(det, np.float64).reshape(-1, 4)), torch.from_numpy(np.asarray(gt, np.float64)[live]))
        best = iou.max(dim=1).values
        first = (iou == best[:, None]).int().argmax(dim=1).numpy()
        best = best.numpy()
        hit = best >= thresh
        match[hit] = live[first[hit]]
    return labels, match, best


@pytest.mark.parametrize("thresh", [0.5, 0.3])
def test_match_ground_truth_is_match_labels_image_by_image(thresh):
    """Labels and match indices exact, IoU bit-equal: both sides evaluate the same IEEE float64 operations, so there is no tolerance."""
    from proben_amd.calibration import match_rows_device
    images = _match_images(np.random.default_rng(11))
    K = 3
    doff = np.cumsum([0] + [len(i[0]) for i in images]).astype(np.int32)
    goff = np.cumsum([0] + [len(i[1]) for i in images]).astype(np.int32)
    cat = lambda k, dt: torch.from_numpy(np.concatenate([np.asarray(i[k], dt).reshape((-1, 4) if k < 2 else (-1,)) for i in images])).cuda()
    for with_crowd in (True, False):
        lab, mat, iou = match_rows_device(cat(0, np.float64), torch.from_numpy(doff).cuda(), cat(1, np.float64), torch.from_numpy(goff).cuda(),
                                          cat(2, np.int32), cat(3, np.int32) if with_crowd else None, thresh, K)
        lab, mat, iou = lab.cpu().numpy(), mat.cpu().numpy(), iou.cpu().numpy()
        assert lab.dtype == np.int32 and mat.dtype == np.int32 and iou.dtype == np.float64
        matched = 0
        for b, (det, gt, cls, crowd) in enumerate(images):
            crowd_b = crowd if with_crowd else np.zeros(len(gt), np.int32)
            wl, wm, wi = _match_reference(det, gt, cls, crowd_b, thresh, K)
            sl = slice(doff[b], doff[b + 1])
            np.testing.assert_array_equal(lab[sl], wl, err_msg=f"labels of image {b}")
            np.testing.assert_array_equal(mat[sl], np.where(wm >= 0, wm + goff[b], -1), err_msg=f"match of image {b}")
            assert iou[sl].tobytes() == wi.astype(np.float64).tobytes(), f"IoU bits of image {b}"
            matched += int((wm >= 0).sum())
        assert matched > 300
    # the hand-made cases say what they are meant to say (with crowd flags; image order of _match_images)
    lab, mat, iou = match_rows_device(cat(0, np.float64), torch.from_numpy(doff).cuda(), cat(1, np.float64), torch.from_numpy(goff).cuda(),
                                      cat(2, np.int32), cat(3, np.int32), 0.5, K)
    lab, mat, iou = lab.cpu().numpy(), mat.cpu().numpy(), iou.cpu().numpy()
    assert lab[doff[5]] == 2 and mat[doff[5]] == goff[5] + 1 and iou[doff[5]] == 0.7            # the crowd box would have been IoU 1
    assert lab[doff[6]] == K and mat[doff[6]] == -1 and iou[doff[6]] == 0.0
    assert mat[doff[7]] == goff[7] + 1 and lab[doff[7]] == 2 and mat[doff[7] + 1] == goff[7] + 3 and iou[doff[7] + 1] == 0.5
    assert lab[doff[8]:doff[9]].tolist() == [1, K, K] and iou[doff[8]] == 0.5 and mat[doff[8]] == goff[8]
    assert mat[doff[9]] == goff[9] + 100 and lab[doff[9]] == 1 and mat[doff[9] + 1] == goff[9] + 1299


# ---- 2. statistics -----------------------------------------------------------------------------------------------------------

def _stat_rows(rng, M, G, spoil=True):
    x, y = rng.uniform(0, 500, G), rng.uniform(0, 400, G)
    gt = np.stack([x, y, x + rng.uniform(10, 200, G), y + rng.uniform(10, 200, G)], 1)
    match = rng.integers(0, G, M).astype(np.int32)
    det = gt[match] + rng.normal(0, 4.0, (M, 4))
    det[:, 2:] = np.maximum(det[:, 2:], det[:, :2] + 1.0)
    var = 10.0 ** rng.uniform(-3, 0, M)
    if spoil and M >= 64:
        idx = rng.choice(M, 7 * max(M // 200, 1), replace=False).reshape(7, -1)
        match[idx[0]] = -1                                   # unmatched
        det[idx[1], 2] = det[idx[1], 0]                      # detection of width 0
        det[idx[2], 3] = det[idx[2], 1] - 2.0                # detection of negative height
        var[idx[3]] = 0.0
        var[idx[4]] = np.nan
        var[idx[5]] = np.inf
        var[idx[6]] = -0.5
        gt[0, 2] = gt[0, 0]                                  # a degenerate ground-truth box: every row matched to it is excluded
    return det, match, gt, var


def _depth_bound(rows, term_error):
    """(c1 + c2 log2(rows)) u sum |terms| with c2 = 1 (the two stride-halving trees add a term at most
    ceil(log2(rows)) times with a rounding, for rows <= 2^18: zero slots add exactly) and c1 = 1 (the ceiling) + term_error + 1
    (fsum's own rounding and the second-order terms).  term_error: the device log and NumPy's are each within 1 ulp <= 2u of the true
    logarithm, so the two differ by <= 4u: that is the whole difference of a log var term (4).  A log coordinate's residual w * log
    then differs by 4u + 2u (each side rounds its own product), its square by 12u + 2u, the quotient by var by 2u more (the division
    itself is correctly rounded on both sides: it adds its rounding of different operands, nothing else) and the three additions of
    a row's four quotients by 6u: 22 for q.  Above 2^18 rows a thread adds ceil(rows / 2^18) rows serially: that many more."""
    serial = max(math.ceil(rows / 2 ** 18) - 1, 0)
    return (1 + term_error + 1 + serial + math.log2(max(rows, 2))) * U


@pytest.mark.parametrize("M,G", [(1, 1), (255, 9), (50_000, 300), (300_000, 1000)])
def test_variance_stats_against_the_restatement(M, G):
    from test_variance_cpu import np_stats
    from proben_amd.calibration import variance_stats
    rng = np.random.default_rng(M + G)
    det, match, gt, var = _stat_rows(rng, M, G)
    dev = [torch.from_numpy(a).cuda() for a in (det, match, gt, var)]
    for s in (1.0, 0.37):
        got = variance_stats(*dev, scale=s)
        with np.errstate(invalid="ignore", divide="ignore"):
            n, sq, sl, c1, c2, bad, aq, al = np_stats(det, match, gt, var, s)
        assert (got["n"], got["cover1"], got["cover2"]) == (n, c1, c2)
        assert got["excluded"] == len(bad) == M - n and got["last_excluded"] == (int(bad.max()) if len(bad) else -1)
        fq = abs(got["sum_q"] - sq) / (_depth_bound(M, 22) * aq) if aq else 0.0
        fl = abs(got["sum_log_var"] - sl) / (_depth_bound(M, 4) * al) if al else 0.0
        print(f"M={M} s={s}: n={n} excluded={len(bad)}  |sum q - fsum| = {fq:.3f} of the bound, |sum log var - fsum| = {fl:.3f} of the bound")
        assert fq <= 1.0 and fl <= 1.0, (fq, fl)
        again = variance_stats(*dev, scale=s)
        assert again == got, "two calls on the same input must give the same bits"
    if M >= 64:
        assert M - n >= 7, "every cause of exclusion is in the set"


def test_each_cause_of_exclusion_adds_nothing_and_is_counted():
    from proben_amd.calibration import variance_stats
    rng = np.random.default_rng(5)
    det, match, gt, var = _stat_rows(rng, 2000, 40, spoil=False)
    cuda = lambda *a: [torch.from_numpy(x).cuda() for x in a]
    base = variance_stats(*cuda(det, match, gt, var))
    assert base["excluded"] == 0 and base["n"] == 2000 and base["last_excluded"] == -1
    # append rows that must be excluded: the sums keep their bits (appended rows fall to other threads' tails: only zeros are added)
    def with_extra(d, m, v):
        return variance_stats(*cuda(np.concatenate([det, d]), np.concatenate([match, m]).astype(np.int32), gt, np.concatenate([var, v])))
    good = np.array([[10.0, 10, 50, 60]])
    causes = {"unmatched": (good, [-1], [0.1]), "beyond the table": (good, [40], [0.1]), "zero width": (np.array([[10.0, 10, 10, 60]]), [3], [0.1]),
              "negative height": (np.array([[10.0, 10, 50, 5]]), [3], [0.1]), "variance 0": (good, [3], [0.0]),
              "variance NaN": (good, [3], [np.nan]), "variance inf": (good, [3], [np.inf]), "variance < 0": (good, [3], [-1.0])}
    for what, (d, m, v) in causes.items():
        got = with_extra(d, np.array(m), np.array(v, np.float64))
        assert got["excluded"] == 1 and got["last_excluded"] == 2000, what
        assert {k: got[k] for k in ("n", "sum_q", "sum_log_var", "cover1", "cover2")} == {k: base[k] for k in ("n", "sum_q", "sum_log_var", "cover1", "cover2")}, what
    gt2 = gt.copy()
    gt2[7, 3] = gt2[7, 1]                                       # a ground-truth box of height 0
    got = variance_stats(*cuda(det, match, gt2, var))
    assert got["excluded"] == int((match == 7).sum()) > 0 and got["n"] == 2000 - got["excluded"]
    from proben_amd.calibration import fit_variance_scale
    with pytest.raises(ValueError, match="no usable row"):
        fit_variance_scale(*cuda(det[:5], np.full(5, -1, np.int32), gt, var[:5]))


# ---- 3. recovery -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s_true", [0.25, 1.0, 4.0])
def test_fit_recovers_the_scale_within_its_statistical_error(s_true):
    """Rows as tests/test_variance_cpu.py::gaussian_rows builds them (get_deltas(detection, gt) Gaussian with variance s_true var_i by
    construction), the matches passed in directly so no IoU gate truncates the residuals.  4 n s_hat / s_true is chi-square with 4 n
    degrees of freedom: |s_hat / s_true - 1| <= 5 sqrt(2 / (4 n)) (1.6 % at 50 000 rows); coverage after the fit within 5 binomial
    standard errors of 0.6827 / 0.9545."""
    from test_variance_cpu import gaussian_rows
    from proben_amd.calibration import fit_variance_scale
    n = 50_000
    det, gt, var = gaussian_rows(np.random.default_rng(int(s_true * 100) + 7), n, s_true)
    fit = fit_variance_scale(torch.from_numpy(det).cuda(), torch.arange(n, dtype=torch.int32, device="cuda"), torch.from_numpy(gt).cuda(),
                             torch.from_numpy(var).cuda())
    print(f"s_true {s_true}: s_hat {fit['scale']:.6f}  ({(fit['scale'] / s_true - 1) / math.sqrt(2 / (4 * n)):+.2f} sigma)  "
          f"coverage {fit['coverage_before']} -> {fit['coverage_after']}  NLL {fit['nll_before']:.3f} -> {fit['nll_after']:.3f}")
    assert fit["rows"] == n and fit["excluded"] == 0
    assert abs(fit["scale"] / s_true - 1) <= 5 * math.sqrt(2 / (4 * n))
    assert fit["nll_after"] <= fit["nll_before"]
    for c, p in zip(fit["coverage_after"], (0.682689492137086, 0.954499736103642)):
        assert abs(c - p) <= 5 * math.sqrt(p * (1 - p) / (4 * n)), (c, p)


# ---- 4. pack -----------------------------------------------------------------------------------------------------------------

def synthetic_dets(nd, B=8, D=48, K=3, seed=0):
    """forward_batch-shaped dicts of `nd` detectors that see the same objects: boxes f32 [B,D,4], classes i32, class_logits f32
    [B,D,K+1], prob_score f32 [B,D,K] / scores f32 (the float32 softmax), vars f32, counts i32.  Image 0: detector 0 alone (the
    single-source passthrough); image 1: nothing."""
    rng = np.random.default_rng(seed)
    out = [{k: np.zeros(s, dt) for k, s, dt in (("boxes", (B, D, 4), np.float32), ("classes", (B, D), np.int32), ("class_logits", (B, D, K + 1), np.float32),
                                                ("vars", (B, D), np.float32), ("counts", (B,), np.int32))} for _ in range(nd)]
    for b in range(B):
        n_obj = int(rng.integers(6, 30))
        x, y = rng.uniform(20, 500, n_obj), rng.uniform(20, 400, n_obj)
        obj = np.stack([x, y, x + rng.uniform(30, 120, n_obj), y + rng.uniform(30, 120, n_obj)], 1)
        ocls = rng.integers(0, K, n_obj)
        for d in range(nd):
            if b == 1 or (b == 0 and d > 0):
                continue
            seen = np.nonzero(rng.random(n_obj) < 0.8)[0][:D]
            c = len(seen)
            out[d]["counts"][b] = c
            out[d]["boxes"][b, :c] = obj[seen] + rng.normal(0, 2.5, (c, 4))
            cls = np.where(rng.random(c) < 0.85, ocls[seen], rng.integers(0, K, c))
            lg = rng.normal(0, 1.0, (c, K + 1))
            lg[np.arange(c), cls] += rng.uniform(2.0, 6.0, c)
            out[d]["classes"][b, :c] = cls
            out[d]["class_logits"][b, :c] = lg
            out[d]["vars"][b, :c] = 10.0 ** rng.uniform(-3, -1, c)
    dets = []
    for o in out:
        t = {k: torch.from_numpy(v).cuda() for k, v in o.items()}
        p = torch.softmax(t["class_logits"], dim=2)
        t["prob_score"] = p[..., :K].contiguous()
        t["scores"] = p.gather(2, t["classes"].long().unsqueeze(2))[..., 0].contiguous()
        dets.append(t)
    return dets


def _row_detectors(dets, max_class):
    """Per image, the detector of every packed row (rows in detector order, classes > max_class dropped) and its float32 variance."""
    B = dets[0]["counts"].numel()
    who, var = [], []
    for b in range(B):
        w, v = [], []
        for k, d in enumerate(dets):
            c = int(d["counts"][b])
            keep = (d["classes"][b, :c] <= max_class).cpu().numpy()
            w += [k] * int(keep.sum())
            v += d["vars"][b, :c].cpu().numpy()[keep].tolist()
        who.append(np.asarray(w, np.int64))
        var.append(np.asarray(v, np.float32))
    return who, var


@pytest.mark.parametrize("route", ["probabilities", "logits", "log_posteriors"])
@pytest.mark.parametrize("scales,max_class", [((0.25, 3.5), 2), ((0.6, 1.0, 7.25), 2), ((1.7, 0.3), 1)])
def test_pack_calibrated_scales_the_variances_and_nothing_else(route, scales, max_class):
    from proben_amd import fusion as F
    nd = len(scales)
    dets = synthetic_dets(nd, seed=nd)
    temps = None if route == "probabilities" else [1.3, 0.7, 2.0][:nd]
    kw = dict(temperatures=temps, log_posteriors=route == "log_posteriors")
    ref = F.pack_rows(dets, max_class, **kw)                                     # the existing entry point
    got = F.pack_rows(dets, max_class, variance_scales=scales, **kw)             # pe_proben_pack_calibrated
    one = F.pack_rows(dets, max_class, variance_scales=[1.0] * nd, **kw)
    torch.cuda.synchronize()
    assert len(got) == len(ref) == (9 if route == "log_posteriors" else 8)
    cnt = ref[6].cpu().numpy()
    S = nd * dets[0]["scores"].shape[1]
    live = torch.from_numpy((np.arange(S)[None] < cnt[:, None]).reshape(-1)).cuda()
    assert int(live.sum()) > 50
    for i in (5, 6, 7):                                                          # offsets, counts, single-source flags
        assert torch.equal(ref[i], got[i]) and torch.equal(ref[i], one[i])
    for i in [0, 1, 2, 4] + ([8] if route == "log_posteriors" else []):          # boxes, scores, probabilities, classes, log-posteriors
        assert got[i][live].cpu().numpy().tobytes() == ref[i][live].cpu().numpy().tobytes(), i
        assert one[i][live].cpu().numpy().tobytes() == ref[i][live].cpu().numpy().tobytes(), i
    assert one[3][live].cpu().numpy().tobytes() == ref[3][live].cpu().numpy().tobytes()        # all scales 1.0: the same bits
    who, var = _row_detectors(dets, max_class)
    gv = got[3].cpu().numpy()
    dropped = sum(int(d["counts"].sum()) for d in dets) - int(cnt.sum())
    assert (dropped > 0) == (max_class < 2)
    for b in range(len(cnt)):
        assert len(who[b]) == cnt[b]
        want = var[b].astype(np.float64) * np.asarray(scales, np.float64)[who[b]]
        assert gv[b * S:b * S + cnt[b]].tobytes() == want.tobytes(), f"vars of image {b}"


# ---- 5. fusion ---------------------------------------------------------------------------------------------------------------

def _fused_rows(fused, S):
    c = fused["counts"].cpu().tolist()
    bx, sc, cl = fused["boxes"].cpu().numpy(), fused["scores"].cpu().numpy(), fused["classes"].cpu().numpy()
    return [(bx[b * S:b * S + c[b]], sc[b * S:b * S + c[b]], cl[b * S:b * S + c[b]]) for b in range(len(c))]


@pytest.mark.parametrize("score_fusion", ["probEn", "avg", "probEn-log"])
@pytest.mark.parametrize("scales", [(0.25, 3.5), (2.0, 0.5, 6.0)])
def test_vavg_on_the_scaled_variances_is_the_oracles(score_fusion, scales):
    """fuse_detections(..., "v-avg", variance_scales) against oracle.proben fed (double)var * s_d, at the tolerances of
    tests/test_proben_gpu.py: classes exact, scores rtol 1e-6, boxes rtol 1e-9 + atol 1e-9.  "probEn-log" is not in the oracle: its
    clusters are those of "probEn" on the T = 1 rows (the clustering order is the calibrated score's in both), so its boxes are
    compared with the oracle's "probEn" boxes on those rows, and its scores and classes with the unscaled run's (variances do not
    enter a score), bit for bit."""
    from oracle import proben as O
    from proben_amd import fusion as F
    nd = len(scales)
    dets = synthetic_dets(nd, seed=10 + nd)
    B, D = dets[0]["scores"].shape
    S, K = nd * D, 3
    logp = score_fusion == "probEn-log"
    temps = [1.0] * nd if logp else None
    got = F.fuse_detections(dets, score_fusion, "v-avg", variance_scales=scales, temperatures=temps)
    plain = F.fuse_detections(dets, score_fusion, "v-avg", temperatures=temps)
    ob, os_, op, ov, oc, ooff, ocnt, osingle = F.pack_rows(dets, 2, temps)[:8]
    torch.cuda.synchronize()
    cnt, single = ocnt.cpu().numpy(), osingle.cpu().numpy()
    hb, hs, hp, hv, hc = (t.cpu().numpy() for t in (ob, os_, op, ov, oc))
    who, _ = _row_detectors(dets, 2)
    rows, rows_plain = _fused_rows(got, S), _fused_rows(plain, S)
    moved, fused_images = 0.0, 0
    for b in range(B):
        sl = slice(b * S, b * S + cnt[b])
        bx, sc, cl = rows[b]
        if cnt[b] == 0:
            assert len(sc) == 0
            continue
        if single[b]:
            np.testing.assert_array_equal(bx, hb[sl])
            np.testing.assert_array_equal(sc, hs[sl].astype(np.float32))
            continue
        info = {"bbox": hb[sl], "score": hs[sl], "class": hc[sl], "prob": hp[sl], "vars": hv[sl] * np.asarray(scales)[who[b]]}
        empty = {"bbox": np.zeros((0, 4)), "score": np.zeros(0), "class": np.zeros(0), "prob": np.zeros((0, K)), "vars": np.zeros(0)}
        wb, ws, wc = O.fusion(["probEn" if logp else score_fusion, "v-avg"], info, empty)
        wb = np.asarray(wb, np.float64).reshape(-1, 4)
        assert len(ws) == len(sc), f"image {b}: {len(ws)} / {len(sc)} fused rows"
        np.testing.assert_allclose(bx, wb, rtol=1e-9, atol=1e-9, err_msg=f"boxes of image {b}")
        if logp:
            assert sc.tobytes() == rows_plain[b][1].tobytes() and cl.tobytes() == rows_plain[b][2].tobytes()
        else:
            np.testing.assert_array_equal(cl, np.asarray(wc, np.float32))
            np.testing.assert_allclose(sc, np.asarray(ws, np.float32), rtol=1e-6, atol=0)
        moved = max(moved, float(np.abs(bx - rows_plain[b][0]).max()))
        fused_images += 1
    assert fused_images >= 4 and moved > 1e-3, "unequal scales must move some v-avg box"


@pytest.mark.parametrize("method", [("probEn", "s-avg"), ("avg", "avg"), ("probEn", "argmax"), ("max", "argmax"), ("probEn-log", "s-avg")],
                         ids=lambda m: "/".join(m))
def test_scales_change_no_bit_outside_vavg(method):
    from proben_amd import fusion as F
    dets = synthetic_dets(2, seed=21)
    temps = [1.2, 0.9] if method[0] == "probEn-log" else None
    a = F.fuse_detections(dets, method[0], method[1], temperatures=temps)
    b = F.fuse_detections(dets, method[0], method[1], temperatures=temps, variance_scales=[0.2, 9.0])
    torch.cuda.synchronize()
    assert torch.equal(a["counts"], b["counts"]) and int(a["counts"].sum()) > 20
    S = a["stride"]
    live = (torch.arange(S, device="cuda")[None] < a["counts"][:, None]).reshape(-1)
    for k in ("boxes", "scores", "classes"):
        assert a[k][live].cpu().numpy().tobytes() == b[k][live].cpu().numpy().tobytes(), k


def _j1_of(det, max_class=2):
    """A forward_batch-shaped dict as the J1 prediction dict the file route reads (float32 values as Python floats: exact)."""
    B = det["counts"].numel()
    out = {k: [] for k in ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")}
    for b in range(B):
        c = int(det["counts"][b])
        keep = (det["classes"][b, :c] <= max_class).cpu().numpy()
        f = lambda k: det[k][b, :c].cpu().numpy()[keep]
        out["image"].append(f"{b}.jpeg")
        out["image_id"].append(b)
        out["boxes"].append(f("boxes").tolist())
        out["scores"].append(f("scores").tolist())
        out["classes"].append(f("classes").tolist())
        out["class_logits"].append(f("class_logits").tolist())
        out["probs"].append(f("prob_score").tolist())
        out["vars"].append([[float(v)] for v in f("vars")])
    return out


@pytest.mark.parametrize("method,temps", [(("probEn", "v-avg"), None), (("avg", "v-avg"), (1.4, 0.8)), (("probEn-log", "v-avg"), None)],
                         ids=lambda v: "/".join(v) if isinstance(v, tuple) and isinstance(v[0], str) else str(v))
def test_file_route_and_device_route_give_the_same_rows(method, temps):
    """late_fusion / fusion() on the J1 form of the detectors' rows with variance_scales, against fuse_detections on the device
    tensors: the same variances ((double)var * s on both), so the same fused rows - bit for bit (one kernel, the same inputs)."""
    from proben_amd import fusion as F
    from proben_amd.late_fusion import late_fusion
    dets = synthetic_dets(2, seed=33)
    scales = [0.3, 2.5]
    dev = F.fuse_detections(dets, method[0], method[1], temperatures=temps, variance_scales=scales)
    torch.cuda.synchronize()
    S = dev["stride"]
    rows = _fused_rows(dev, S)
    j1 = [_j1_of(d) for d in dets]
    res = late_fusion(j1, list(method), temperatures=temps, variance_scales=scales)
    unscaled = late_fusion(j1, list(method), temperatures=temps)
    differs = False
    for b, r in enumerate(res):
        if r is None:
            assert len(rows[b][1]) == 0
            continue
        bx, sc, cl = r
        assert np.asarray(bx, np.float64).tobytes() == rows[b][0].tobytes(), f"boxes of image {b}"
        assert sc.numpy().tobytes() == rows[b][1].tobytes() and cl.numpy().tobytes() == rows[b][2].tobytes(), f"image {b}"
        differs |= np.asarray(unscaled[b][0]).tobytes() != np.asarray(bx).tobytes()
    assert differs
    # the one-image form
    b = 3
    info = lambda d: {"img_name": d["image"][b], "bbox": d["boxes"][b], "score": d["scores"][b], "class": d["classes"][b],
                      "class_logits": d["class_logits"][b], "prob": d["probs"][b], "vars": d["vars"][b]}
    fb, fs, fc = F.fusion(list(method), info(j1[0]), info(j1[1]), temperatures=temps, variance_scales=scales)
    assert np.asarray(fb, np.float64).reshape(-1, 4).tobytes() == rows[b][0].tobytes() and fs.numpy().tobytes() == rows[b][1].tobytes()


# ---- 6. drivers --------------------------------------------------------------------------------------------------------------

def test_drivers_end_to_end(tmp_path, capsys):
    """save_predictions x 2 -> fit_temperature --with-variance -> demo_probEn --calibration (two-stage and --one-pass) and
    --variance_scales.  The dataset's annotations are rewritten after the predictions exist, as displaced copies of each detector's
    first detection per image, so that every detector has matched rows with non-zero residuals whatever the synthetic weights find."""
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
                             "area": (x2 - x1) * (y2 - y1), "iscrowd": 0})        # displaced relative to the box: IoU > 0.8 at any size
    assert anns
    ds["annotations"] = anns
    json.dump(ds, open(val, "w"))

    cal0, cal = tmp_path / "cal_plain.json", tmp_path / "cal_var.json"
    fit_temperature.main(["--predictions", *files, "--dataset_path", str(root), "--holdout", "0.5", "--out", str(cal0)])
    capsys.readouterr()
    fit_temperature.main(["--predictions", *files, "--dataset_path", str(root), "--holdout", "0.5", "--out", str(cal), "--with-variance"])
    printed = capsys.readouterr().out
    r0, r1 = json.load(open(cal0)), json.load(open(cal))
    assert set(r0) == {"detectors", "nll", "rows", "holdout", "fitted_image_ids", "at_bound"}          # the parent's keys, no more
    assert {k: r1[k] for k in r0} == r0
    assert set(r1) - set(r0) == {"variance_scales", "variance_nll", "variance_rows", "variance_excluded", "variance_coverage"}
    assert C.load_variance(cal0) is None
    sc = C.load_variance(cal)
    for m in names:
        assert f"{m}: variance scale = " in printed
        assert sc[m] > 0 and r1["variance_rows"][m] > 0 and r1["variance_nll"][m]["after"] <= r1["variance_nll"][m]["before"]
        assert len(r1["variance_coverage"][m]["after"]) == 2 and r1["variance_excluded"][m] >= 0
    T = [r1["detectors"][m] for m in names]
    s = [sc[m] for m in names]

    def two_stage(tag, extra):
        out = tmp_path / f"out2_{tag}"
        res = demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names),
                                "--outfolder", str(out), "--dataset_name", f"flir_var2_{tag}"] + extra)
        return out, res

    out2, res2 = two_stage("cal", ["--calibration", str(cal)])
    said = capsys.readouterr().out
    assert f"variance scales of {cal}" in said
    assert res2["variance_scales"] == dict(zip(names, s)) and res2["temperatures"] == dict(zip(names, T))
    tflag = ["--temperatures", ",".join(repr(t) for t in T)]
    out3, res3 = two_stage("pos", tflag + ["--variance_scales", ",".join(repr(x) for x in s)])
    out4, res4 = two_stage("name", tflag + ["--variance_scales", ",".join(f"{m}={x!r}" for m, x in reversed(list(zip(names, s))))])
    for o in (out3, out4):
        assert (o / "coco_instances_results.json").read_bytes() == (out2 / "coco_instances_results.json").read_bytes()
    # a file without the key, and no flag: nothing changes, and the run does not speak of scales
    capsys.readouterr()
    out5, res5 = two_stage("plaincal", ["--calibration", str(cal0)])
    out6, res6 = two_stage("temps", tflag)
    assert "variance scales" not in capsys.readouterr().out and "variance_scales" not in res5 and "variance_scales" not in res6
    assert (out5 / "coco_instances_results.json").read_bytes() == (out6 / "coco_instances_results.json").read_bytes()
    # the scales reach the fusion: a second detector that is the first one displaced by 4 % of each box's size (every detection in a cluster of two
    # with equal variances), fused with very unequal scales, gives other boxes than fused with none
    sdir = tmp_path / "pred_skew"
    sdir.mkdir()
    (sdir / f"val_{names[0]}_predictions.json").write_bytes((pdir / f"val_{names[0]}_predictions.json").read_bytes())
    twin = json.loads(json.dumps(preds[0]))
    twin["boxes"] = [[[x1 + 0.04 * (x2 - x1), y1 + 0.04 * (y2 - y1), x2 + 0.04 * (x2 - x1), y2 + 0.04 * (y2 - y1)] for x1, y1, x2, y2 in rows]
                     for rows in twin["boxes"]]                     # IoU 0.73 with the original at any size
    json.dump(twin, open(sdir / f"val_{names[1]}_predictions.json", "w"))
    assert sum(len(r) for r in twin["boxes"]) > 0

    def skew(tag, extra):
        out = tmp_path / f"out_skew_{tag}"
        demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(sdir), "--detectors", ",".join(names),
                          "--outfolder", str(out), "--dataset_name", f"flir_var_skew_{tag}"] + extra)
        return json.load(open(out / "coco_instances_results.json"))
    even, tilted = skew("even", []), skew("tilted", ["--variance_scales", "0.01,100"])
    assert len(even) == len(tilted) > 0 and [(r["image_id"], r["category_id"]) for r in even] == [(r["image_id"], r["category_id"]) for r in tilted]
    be, bt = np.asarray([r["bbox"] for r in even]), np.asarray([r["bbox"] for r in tilted])
    # equal weights put a pair's box at its midpoint, 2 % of the size from either member; weights 10^4 : 1 put it on the first detector's
    shift = np.abs(be[:, :2] - bt[:, :2]) / np.maximum(be[:, 2:], 1e-9)
    print("largest move of a fused corner under scales 0.01 / 100:", float(shift.max()), "of the box size")
    assert shift.max() > 0.01, shift.max()
    # --one-pass: the standard of tests/test_calibration_gpu.py::test_drivers_end_to_end (the two-stage driver hands float32 boxes to
    # the evaluator, the one-pass route float64 rows): the evaluation file byte for byte, ids / categories / scores identical, boxes 1e-6
    out1 = tmp_path / "out1_cal"
    res1 = demo_probEn.main(["--one-pass", "--dataset_path", str(root), "--detectors", ",".join(names), "--model_paths", ",".join(paths),
                             "--workers", "2", "--batch", "4", "--outfolder", str(out1), "--dataset_name", "flir_var1", "--calibration", str(cal)])
    assert res1["variance_scales"] == res2["variance_scales"] and f"variance scales of {cal}" in capsys.readouterr().out
    assert (out1 / "FLIR_probEn_eval.json").read_bytes() == (out2 / "FLIR_probEn_eval.json").read_bytes()
    a, b = json.load(open(out1 / "coco_instances_results.json")), json.load(open(out2 / "coco_instances_results.json"))
    assert len(a) == len(b) > 0
    assert [(r["image_id"], r["category_id"], r["score"]) for r in a] == [(r["image_id"], r["category_id"], r["score"]) for r in b]
    np.testing.assert_allclose([r["bbox"] for r in a], [r["bbox"] for r in b], rtol=1e-6, atol=1e-4)
