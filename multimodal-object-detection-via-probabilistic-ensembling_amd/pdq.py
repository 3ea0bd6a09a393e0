"""Probability-based Detection Quality (PDQ; Hall et al., WACV 2020) of a prediction file: DESIGN.md section 30.

AP ranks detections by score and never reads a variance; PDQ scores a detection as the probabilistic prediction it is.  Every detection is
matched one-to-one with the ground truth of its image by an optimal assignment over the pair quality q = sqrt(Q_S * Q_L): Q_L the
probability the row's label distribution gives the true class, Q_S the spatial quality - the row's per-pixel probability integrated over the
ground-truth box (foreground) and over what it claims outside it (background).  PDQ = sum q / (TP + FP + FN).  The rule is restated from
the paper (include/proben_hip.h states it; tests/pdq_ref.py restates it in NumPy): box ground truth, one scalar variance per box.

    pair_quality(...)            q, exp(FG), exp(BG), Q_L of every (ground truth, detection) pair, one launch (pe_pdq_pair_quality)
    assign(...)                  the optimal one-to-one assignment per image, on the host (pe_pdq_assign)
    pdq_from_predictions(...)    per-image records and the dataset summary of a prediction file, per score threshold
    summarise(per_image)         the dataset figures of (a weighting of) the per-image records
    bootstrap_pdq(...)           percentile intervals over resampled images, and the paired difference of two files
"""
import ctypes

import numpy as np
import torch

from . import _lib, bootstrap, calibration

BBOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
MAX_TABLE = 4096                  # PE_PDQ_MAX_TABLE: W + H of an image
DEFAULT_CLASSES = 3               # the prediction schema keeps classes 0..2 (late_fusion.predictions_to_j1)
RECORD = ("sum_q", "tp", "fp", "fn", "sum_spatial", "sum_label", "sum_fg", "sum_bg")      # the columns of a per-image record


def _offsets(x, what):
    o = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.int64).reshape(-1)
    if o.size < 1 or o[0] != 0 or (np.diff(o) < 0).any():
        raise ValueError(f"{what} {o.tolist()[:8]}... do not start at 0 and rise")
    return o


def pair_offsets(det_offsets, gt_offsets):
    """int64 [B + 1]: image b's block of G_b * M_b pairs starts at [b]; pair (g, d) is at [b] + g_local * M_b + d_local."""
    return np.concatenate([[0], np.cumsum(np.diff(gt_offsets) * np.diff(det_offsets))]).astype(np.int64)


def pair_quality(det_boxes, det_vars, det_log_probs, det_offsets, gt_boxes, gt_classes, gt_crowd, gt_offsets, image_hw, tau=0.0027,
                 bbox_reg_weights=BBOX_REG_WEIGHTS):
    """One pe_pdq_pair_quality launch over flat device tensors (include/proben_hip.h): det_boxes [M,4] XYXY, det_vars [M], det_log_probs
    [M,K+1] with det_offsets [B+1]; gt_boxes [G,4], gt_classes [G], gt_crowd [G] with gt_offsets [B+1]; image_hw [B,2] = (H, W).
    Returns device tensors "q", "fg", "bg", "label" f64 [pairs] and "gt_live" i32 [G], the host "pair_offsets" i64 [B+1] and the counts
    "excluded_detections" / "ignored_ground_truths" with "last_excluded" / "last_ignored" (an index, -1 when none); synchronises."""
    doff, goff = _offsets(det_offsets, "pair_quality: det_offsets"), _offsets(gt_offsets, "pair_quality: gt_offsets")
    _lib.require_cuda(det_boxes, det_vars, det_log_probs, gt_boxes, gt_classes, gt_crowd, image_hw)
    dev = det_boxes.device
    det_boxes = det_boxes.reshape(-1, 4).contiguous().double()
    det_vars = det_vars.reshape(-1).contiguous().double()
    det_log_probs = det_log_probs.contiguous().double()
    gt_boxes = gt_boxes.reshape(-1, 4).contiguous().double()
    gt_classes = gt_classes.reshape(-1).contiguous().to(torch.int32)
    gt_crowd = gt_crowd.reshape(-1).contiguous().to(torch.int32)
    image_hw = image_hw.reshape(-1, 2).contiguous().to(torch.int32)
    M, G, B = det_boxes.shape[0], gt_boxes.shape[0], image_hw.shape[0]
    if det_log_probs.dim() != 2 or det_log_probs.shape[0] != M or det_log_probs.shape[1] < 2 or det_vars.numel() != M:
        raise ValueError(f"pair_quality: {tuple(det_log_probs.shape)} log-probabilities and {det_vars.numel()} variances for {M} detections")
    if doff.size != B + 1 or goff.size != B + 1 or doff[-1] != M or goff[-1] != G or gt_classes.numel() != G or gt_crowd.numel() != G:
        raise ValueError(f"pair_quality: offsets of {doff.size - 1} / {goff.size - 1} images ending at {doff[-1]} / {goff[-1]} for {B} images, "
                         f"{M} detections, {G} ground truths ({gt_classes.numel()} classes, {gt_crowd.numel()} crowd flags)")
    w = [float(x) for x in bbox_reg_weights]
    if len(w) != 4:
        raise ValueError(f"pair_quality: bbox_reg_weights {bbox_reg_weights!r} is not 4 numbers")
    hw = image_hw.cpu().numpy().astype(np.int64)
    table = int((hw[:, 0] + hw[:, 1]).max()) if B else 0
    poff = pair_offsets(doff, goff)
    pairs = int(poff[-1])
    out = {k: torch.zeros((pairs,), dtype=torch.float64, device=dev) for k in ("q", "fg", "bg", "label")}
    live = torch.zeros((G,), dtype=torch.int32, device=dev)
    flags = torch.zeros((4,), dtype=torch.int32, device=dev)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)      # noqa: E731
    d_doff, d_goff, d_poff = i32(doff), i32(goff), torch.from_numpy(poff).to(dev)
    ptr = lambda t: _lib.ptr(t) if t.numel() else None      # noqa: E731
    with torch.cuda.device(dev):
        st = _lib.lib().pe_pdq_pair_quality(ptr(det_boxes), ptr(det_vars), ptr(det_log_probs), ptr(d_doff), ptr(gt_boxes), ptr(gt_classes),
                                            ptr(gt_crowd), ptr(d_goff), ptr(image_hw), ptr(d_poff), B, det_log_probs.shape[1] - 1, M, G, pairs,
                                            table, (ctypes.c_float * 4)(*w), float(tau), ptr(out["q"]), ptr(out["fg"]), ptr(out["bg"]),
                                            ptr(out["label"]), ptr(live), _lib.ptr(flags), _lib.stream())
    _lib.check(st, "pe_pdq_pair_quality")
    f = flags.cpu().tolist()
    out.update(gt_live=live, pair_offsets=poff, excluded_detections=f[0], last_excluded=f[1] - 1, ignored_ground_truths=f[2], last_ignored=f[3] - 1)
    return out


def assign(q, gt_live, det_offsets, gt_offsets, det_take=None):
    """pe_pdq_assign over host arrays: q f64 [pairs] (pair_quality's layout), gt_live i32 [G], det_take [M] or None (every detection takes
    part).  Returns match i32 [G]: the row index of the ground truth's detection, -1 when it has none (or is not live)."""
    doff, goff = _offsets(det_offsets, "assign: det_offsets"), _offsets(gt_offsets, "assign: gt_offsets")
    if goff.size != doff.size:
        raise ValueError(f"assign: offsets of {doff.size - 1} and {goff.size - 1} images")
    poff = pair_offsets(doff, goff)
    q = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
    live = np.ascontiguousarray(gt_live, dtype=np.int32).reshape(-1)
    take = None if det_take is None else np.ascontiguousarray(det_take, dtype=np.int32).reshape(-1)
    M, G, B = int(doff[-1]), int(goff[-1]), doff.size - 1
    if q.size != poff[-1] or live.size != G or (take is not None and take.size != M):
        raise ValueError(f"assign: {q.size} pair qualities, {live.size} live flags{'' if take is None else f', {take.size} take flags'} for "
                         f"{poff[-1]} pairs, {G} ground truths, {M} detections")
    match = np.full((G,), -1, dtype=np.int32)
    d32, g32 = doff.astype(np.int32), goff.astype(np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None      # noqa: E731
    st = _lib.lib().pe_pdq_assign(p(q), p(live), p(take), p(d32), p(g32), p(poff), B, M, G, int(poff[-1]), p(match))
    _lib.check(st, "pe_pdq_assign")
    return match


def label_spread(scores, classes, num_classes):
    """The label distribution of a conventional detector's rows, as log-probabilities f64 [n, K+1]: the score on the row's class,
    (1 - score) / K on each other column (background included).  A class outside [0, K] or a score outside [0, 1] gives a NaN row."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    c = np.asarray(classes, dtype=np.int64).reshape(-1)
    K = int(num_classes)
    ok = (c >= 0) & (c <= K) & (s >= 0.0) & (s <= 1.0)
    p = np.where(ok[:, None], np.repeat(((1.0 - s) / K)[:, None], K + 1, axis=1), np.nan)
    p[np.nonzero(ok)[0], c[ok]] = s[ok]
    with np.errstate(divide="ignore"):
        return np.log(p)


def _rows(pred, i, temperature, variance_scale, num_classes, device):
    """(boxes [n,4], vars [n], log_probs [n,K+1], scores [n]) of image i of a prediction dict."""
    boxes = np.asarray(pred["boxes"][i], dtype=np.float64).reshape(-1, 4)
    n = boxes.shape[0]
    scores = np.asarray(pred["scores"][i], dtype=np.float64).reshape(-1)
    classes = np.asarray(pred["classes"][i], dtype=np.int64).reshape(-1)
    logits = pred.get("class_logits")
    logits = logits[i] if logits is not None else [[] for _ in range(n)]
    has_logits = n > 0 and all(len(r) == num_classes + 1 for r in logits)
    if n and not has_logits and any(len(r) for r in logits):
        raise ValueError(f"image {pred['image'][i]}: class_logits of {sorted({len(r) for r in logits})} columns, expected {num_classes + 1} or none")
    probs = pred.get("probs")
    headless = not has_logits and (probs is None or all(len(r) == 0 for r in probs[i]))
    if has_logits:
        lp = calibration.log_posterior_rows(logits, temperature, device)
        ok = (classes >= 0) & (classes <= num_classes)
        # the row's own calibrated p[class]; a row whose class names no column keeps the file's score and takes part with it
        scores = np.where(ok, np.exp(lp[np.arange(n), np.clip(classes, 0, num_classes)]), scores)
    else:
        lp = label_spread(scores, classes, num_classes)
    var = pred.get("vars")
    # a row without logits and probabilities comes from a detector without those heads: its vars entry is the schema's placeholder
    # [1.0] (late_fusion.predictions_to_j1), not a variance
    if var is None or headless:
        v = np.zeros(n)
    else:
        if len(var[i]) != n or any(len(np.atleast_1d(x)) == 0 for x in var[i]):
            raise ValueError(f"image {pred['image'][i]}: {len(var[i])} vars entries (or empty ones) for {n} detections")
        v = np.asarray([np.atleast_1d(x)[0] for x in var[i]], dtype=np.float64) * float(variance_scale)
    return boxes, v, lp.reshape(n, num_classes + 1), scores


def infer_num_classes(pred):
    """K of a prediction dict from its class_logits (K + 1 columns) or probs (K columns); None when it carries neither."""
    for key, extra in (("class_logits", 1), ("probs", 0)):
        for rows in pred.get(key) or []:
            for r in rows:
                if len(r):
                    return len(r) - extra
    return None


def summarise(rec):
    """The dataset figures of per-image records [..., N, 8] (or of sums [..., 8]) in RECORD order: PDQ = sum q / (TP + FP + FN) and the mean
    pair, spatial, label, foreground and background quality over the true positives (nan without any)."""
    s = np.asarray(rec, dtype=np.float64)
    s = s.sum(-2) if s.ndim >= 2 else s
    n, tp = s[..., 1] + s[..., 2] + s[..., 3], s[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        per_tp = lambda k: np.where(tp > 0, s[..., k] / tp, np.nan)      # noqa: E731
        return {"pdq": np.where(n > 0, s[..., 0] / n, np.nan), "pair_quality": per_tp(0), "spatial": per_tp(4), "label": per_tp(5),
                "foreground": per_tp(6), "background": per_tp(7), "tp": tp, "fp": s[..., 2], "fn": s[..., 3]}


def pdq_from_predictions(records, pred, temperature=1.0, variance_scale=1.0, score_thresh=(0.5,), support=0.0027, device="cuda",
                         num_classes=None, bbox_reg_weights=BBOX_REG_WEIGHTS):
    """PDQ of a prediction dict (late_fusion J1 schema) over the dataset dicts `records` (data.load_coco_json), every image of `records`
    (one the file does not list has no detections).  A row's label distribution is calibration.log_posterior_rows(class_logits,
    temperature) - its score then the calibrated p[class] - or, without class_logits, label_spread(score, class); its variance is vars *
    variance_scale, or 0 - a hard box - without vars, or when the row has neither logits nor probabilities (vars is then the schema's
    placeholder).  One launch for the rows that pass the smallest threshold, one assignment per threshold.
    Returns {"image_ids", "score_thresh", "per_image" f64 [T, N, 8] in RECORD order, "summary": [per threshold a dict of floats],
    "detections" [T], "live_ground_truths", "flags": the exclusion counts and "unscored_rows" (rows whose score is NaN: they pass no
    threshold and take no part), "num_classes"}.  A vars list that does not match the image's boxes is a ValueError."""
    temperature = calibration.check_temperature(temperature)
    variance_scale = calibration.check_variance_scale(variance_scale)
    thr = sorted({float(t) for t in np.atleast_1d(score_thresh)})
    if not thr or any(not 0.0 <= t <= 1.0 for t in thr):
        raise ValueError(f"pdq_from_predictions: score_thresh {score_thresh!r} is not a list of numbers in [0, 1]")
    if not 0.0 <= float(support) < 1.0:
        raise ValueError(f"pdq_from_predictions: support {support} is not in [0, 1)")
    K = num_classes if num_classes is not None else infer_num_classes(pred)
    K = DEFAULT_CLASSES if K is None else int(K)
    where = {iid: i for i, iid in enumerate(pred["image_id"])}
    known = {r["image_id"] for r in records}
    extra = [i for i in pred["image_id"] if i not in known]
    if extra:
        raise ValueError(f"pdq_from_predictions: {len(extra)} images the dataset does not have (image id {extra[0]} is one)")
    boxes, var, lp, score, doff = [], [], [], [], [0]
    gt, gcls, crowd, goff, hw = [], [], [], [0], []
    unscored = 0
    for r in records:
        hw.append([r["height"], r["width"]])
        if r["height"] + r["width"] > MAX_TABLE:
            raise ValueError(f"pdq_from_predictions: image {r['image_id']} is {r['width']} x {r['height']}: W + H is above {MAX_TABLE}")
        if r["image_id"] in where:
            b, v, l, s = _rows(pred, where[r["image_id"]], temperature, variance_scale, K, device)
            keep = s >= thr[0]
            unscored += int(np.isnan(s).sum())      # a NaN score passes no threshold: counted, not silently dropped
            boxes.append(b[keep]); var.append(v[keep]); lp.append(l[keep]); score.append(s[keep])
        doff.append(doff[-1] + (len(score[-1]) if r["image_id"] in where else 0))
        for a in r["annotations"]:
            x, y, w, h = a["bbox"]                  # COCO XYWH -> XYXY
            gt.append([x, y, x + w, y + h]); gcls.append(a["category_id"]); crowd.append(a.get("iscrowd", 0))
        goff.append(len(gt))
    cat = lambda parts, shape: np.concatenate(parts).reshape(shape) if parts else np.zeros((0,) + tuple(shape[1:]))      # noqa: E731
    boxes, var, lp, score = cat(boxes, (-1, 4)), cat(var, (-1,)), cat(lp, (-1, K + 1)), cat(score, (-1,))
    dev = torch.device(device)
    t = lambda a, dt, shape: torch.as_tensor(np.asarray(a), dtype=dt).reshape(shape).to(dev)      # noqa: E731
    pq = pair_quality(t(boxes, torch.float64, (-1, 4)), t(var, torch.float64, (-1,)), t(lp, torch.float64, (-1, K + 1)), doff,
                      t(gt, torch.float64, (-1, 4)), t(gcls, torch.int32, (-1,)), t(crowd, torch.int32, (-1,)), goff,
                      t(hw, torch.int32, (-1, 2)), support, bbox_reg_weights)
    host = {k: pq[k].cpu().numpy() for k in ("q", "fg", "bg", "label", "gt_live")}
    doff, goff, poff = np.asarray(doff), np.asarray(goff), pq["pair_offsets"]
    N = len(records)
    img_of_det = np.repeat(np.arange(N), np.diff(doff))
    img_of_gt = np.repeat(np.arange(N), np.diff(goff))
    per_image = np.zeros((len(thr), N, len(RECORD)))
    for ti, th in enumerate(thr):
        take = (score >= th).astype(np.int32)
        match = assign(host["q"], host["gt_live"], doff, goff, take)
        hit = np.nonzero(match >= 0)[0]
        b = img_of_gt[hit]
        pair = poff[b] + (hit - goff[b]) * (doff[b + 1] - doff[b]) + (match[hit] - doff[b])
        rec = per_image[ti]
        for col, val in ((0, host["q"][pair]), (1, np.ones(len(hit))), (4, host["fg"][pair] * host["bg"][pair]), (5, host["label"][pair]),
                         (6, host["fg"][pair]), (7, host["bg"][pair])):
            np.add.at(rec[:, col], b, val)
        rec[:, 2] = np.bincount(img_of_det, weights=take, minlength=N) - rec[:, 1]
        rec[:, 3] = np.bincount(img_of_gt, weights=host["gt_live"], minlength=N) - rec[:, 1]
    summ = summarise(per_image)
    return {"image_ids": [r["image_id"] for r in records], "score_thresh": thr, "per_image": per_image, "num_classes": K,
            "summary": [{k: float(v[ti]) for k, v in summ.items()} for ti in range(len(thr))],
            "detections": [int((score >= th).sum()) for th in thr], "live_ground_truths": int(host["gt_live"].sum()),
            "flags": dict({k: pq[k] for k in ("excluded_detections", "last_excluded", "ignored_ground_truths", "last_ignored")},
                          unscored_rows=unscored)}


def replicate_pdq(per_image, mult):
    """PDQ of every replicate: mult [R, N] multiplicities over per-image records [N, 8] -> (mult @ sum_q) / (mult @ (TP + FP + FN)), nan
    where a replicate has neither detections nor ground truth."""
    rec = np.asarray(per_image, dtype=np.float64)
    m = np.asarray(mult, dtype=np.float64)
    num, den = m @ rec[:, 0], m @ (rec[:, 1] + rec[:, 2] + rec[:, 3])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / den, np.nan)


def bootstrap_pdq(per_image_a, per_image_b=None, replicates=2000, seed=0, confidence=0.95):
    """Percentile-bootstrap interval and standard error of PDQ over resampled images from per-image records [N, 8] (no launch), and - with
    a second file over the same images, under the same resamples - the paired difference b - a with its interval and the two-sided
    p-value (bootstrap.paired).  Row 0 of the multiplicities is the dataset itself: the point estimate."""
    if not 0.0 < confidence < 1.0:
        raise ValueError(f"confidence {confidence} is not in (0, 1)")
    if replicates < 2:
        raise ValueError(f"replicates {replicates}: the resamples are rows 1.. (row 0 is the dataset itself), so at least 2")
    a = np.asarray(per_image_a, dtype=np.float64)
    mult = bootstrap.resample_multiplicities(a.shape[0], replicates, seed)
    xa = replicate_pdq(a, mult)
    out = {"a": dict(point=float(xa[0]), **bootstrap._interval(xa[1:], None, confidence))}
    if per_image_b is not None:
        b = np.asarray(per_image_b, dtype=np.float64)
        if b.shape != a.shape:
            raise ValueError(f"bootstrap_pdq: records of {a.shape[0]} and {b.shape[0]} images: a paired bootstrap needs both files over one image set")
        xb = replicate_pdq(b, mult)
        out["b"] = dict(point=float(xb[0]), **bootstrap._interval(xb[1:], None, confidence))
        out["paired"] = bootstrap.paired(xa[1:], xb[1:], xa[0], xb[0], np.isnan, confidence)
    return out
