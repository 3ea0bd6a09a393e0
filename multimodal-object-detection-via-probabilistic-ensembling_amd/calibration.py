"""Temperature calibration of the detectors' class posteriors ahead of ProbEn.

ProbEn multiplies the detectors' posteriors, which is right for calibrated posteriors only.  One scalar T per detector,
    p = softmax(class_logits / T)            (K + 1 columns, background last; float64 on the device, csrc/calibrate.hip)
keeps every detection's argmax and ranking.  This module holds
  calibrated_probs   the row arithmetic of pe_proben_pack_logits over a flat [M, K+1] tensor
  match_labels       detections -> labels in [0, K] from the ground truth
  fit_temperature    T that minimises the negative log-likelihood of the labels (pe_temperature_nll, 64 candidates per launch)
  save / load        the calibration file  {"detectors": {name: T}, "nll": {...}, "rows": {...}[, "class_prior": [K + 1]]}
  log_posteriors     log_softmax(logits / T) over all K + 1 columns (pe_log_softmax): the rows of score_fusion "probEn-log"
  check_class_prior / parse_class_prior      the class prior of that mode (K + 1 probabilities, background last)
  resolve / calibrate_j1 / require_logits   what the drivers (fusion.fusion, late_fusion, cli/demo_probEn) share.

Variance calibration (csrc/variance.hip): one scale s per detector, variance' = s * variance, for the 1 / variance weights of v-avg.
  match_rows_device    detections -> (label, matched ground-truth index, IoU) on the device, batched (pe_match_ground_truth)
  variance_stats / fit_variance_scale      the Gaussian NLL's statistics of the matched rows (pe_variance_stats) and the closed-form fit
  check_variance_scale / parse_variance_scales / resolve_variance_scales / scale_j1_vars
  save_variance / load_variance            the "variance_*" keys of the calibration file (save / load above do not know them)

Reliability of a score on rows the fit did not see (csrc/reliability.hip; the driver is cli/calibration_report):
  reliability / reliability_scores         per-bin counts and sums from pe_reliability_logits / pe_reliability_scores, one launch each
  summarise_reliability                    ECE, MCE and the Brier score from those, on the host

Pooling weights (csrc/pool.hip, csrc/proben.hip): one exponent w per detector inside score_fusion "probEn-log", for detectors that
share evidence.
  pool_nll / fit_pool_weights              the fused posterior's NLL and gradient for up to 64 candidates (pe_pool_nll); the safeguarded fit
  check_pool_weights / parse_pool_weights / resolve_pool_weights
  save / load                              carry the optional key "pool_weights" {name: w}

Presence evidence (csrc/presence.hip, csrc/proben.hip): one row of log-evidence per presence pattern (which detectors put a row into
the cluster) inside score_fusion "probEn-log", added to the fused columns last; clusters of one row and passthrough images included.
  check_presence / presence_table / parse_presence / resolve_presence
  bias_nll / fit_presence                  a table row's NLL and gradient for up to 64 candidates (pe_bias_nll); the per-pattern fit
  save / load                              carry the optional key "presence" {"detectors", "columns", "table", "hi"}

Correlated box fusion (csrc/boxcorr.hip): box_fusion "c-avg", the generalised-least-squares mean of a cluster's boxes under one
correlation per detector pair of the normalised box errors, and the variance that mean really has.
  check_box_correlation / box_correlation_tensor / parse_box_correlation / resolve_box_correlation
  box_pair_stats / fit_box_correlation     the residuals' cross products per detector pair (pe_box_pair_stats); the uncentred estimator
  shrink_to_psd                            the off-diagonal shrink that makes a fitted matrix positive semidefinite
  save / load                              carry the optional key "box_correlation" {"detectors", "matrix", "raw", "shrink", "pairs",
                                           "rows", "excluded", "iou", "box_fusion": "v-avg"}
"""
import ctypes
import json
import math

import numpy as np
import torch

from . import _lib

NLL_CANDIDATES = 64          # pe_temperature_nll's limit: one launch evaluates this many temperatures
NLL_MAX_BLOCKS = 1024        # PE_TEMPERATURE_NLL_MAX_BLOCKS (include/proben_hip.h): sizes the partial-sum workspace
VARIANCE_MAX_BLOCKS = 1024   # PE_VARIANCE_STATS_MAX_BLOCKS: 5 partial values per workgroup
RELIABILITY_MAX_BINS = 64    # PE_RELIABILITY_MAX_BINS
RELIABILITY_MAX_BLOCKS = 1024     # PE_RELIABILITY_MAX_BLOCKS: 4 partial values per workgroup and bin
POOL_MAX_DETECTORS = 8       # PE_POOL_MAX_DETECTORS
POOL_NLL_MAX_BLOCKS = 1024   # PE_POOL_NLL_MAX_BLOCKS: 1 + num_detectors partial values per workgroup and candidate
PRESENCE_MAX_DETECTORS = 4   # PE_PRESENCE_MAX_DETECTORS
BIAS_NLL_MAX_COLUMNS = 16    # PE_BIAS_NLL_MAX_COLUMNS: a lane of pe_bias_nll keeps 1 + (K + 1) accumulators in registers
BIAS_NLL_MAX_BLOCKS = 1024   # PE_BIAS_NLL_MAX_BLOCKS: 1 + (K + 1) partial values per workgroup and candidate
BOX_CORR_MAX_DETECTORS = PRESENCE_MAX_DETECTORS      # PE_BOX_CORR_MAX_DETECTORS
BOX_PAIR_MAX_BLOCKS = 1024   # PE_BOX_PAIR_MAX_BLOCKS: 28 partial values per workgroup
BBOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)      # cfg.MODEL.ROI_BOX_HEAD.BBOX_REG_WEIGHTS: the units the variance head is trained in


def _finite_positive(x, what):
    """The rule for a temperature and for a variance scale."""
    x = float(x)
    if not (math.isfinite(x) and x > 0):
        raise ValueError(f"{what} {x!r} is not finite and > 0")
    return x


def check_temperature(t, what="temperature"):
    return _finite_positive(t, what)


def _statistic(who, nv, work_values, dev, launch):
    """The device side of the six statistic calls (csrc/reduce2.h): allocate [nv result slots | the two int32 flags in one f64 slot]
    as one buffer and a workspace of work_values f64, run launch(work, out, flags, stream) -> status, download once.
    Returns (the nv result slots on the host, excluded items, the last excluded index or -1)."""
    res = torch.empty((nv + 1,), dtype=torch.float64, device=dev)
    work = torch.empty((work_values,), dtype=torch.float64, device=dev)
    st = launch(_lib.ptr(work), _lib.ptr(res), ctypes.c_void_p(res.data_ptr() + 8 * nv), _lib.stream())
    _lib.check(st, who)
    host = res.cpu()
    bad, last = host[nv:].view(torch.int32).tolist()
    return host[:nv], bad, last - 1


# ---- one value per detector, from the command line ('a,b[,c]' by position, 'name=a,name=b' by name) or from a {name: value} table.
# kind = (the noun of the messages, values in the order of names -> the validated list).  Temperatures and variance scales validate
# entry by entry; pool weights validate as a list (the count limits, "all 0").

def _resolve(kind, table, names, source):
    noun, validate = kind
    missing = [n for n in names if n not in table]
    if missing:
        raise ValueError(f"{source} has no {noun} for {','.join(missing)} (it lists {','.join(sorted(table)) or 'nothing'})")
    return validate([table[n] for n in names], names, source)


def _parse(kind, flag, text, names):
    items = [x.strip() for x in text.split(",") if x.strip()]
    named = ["=" in x for x in items]
    if any(named) != all(named):
        raise ValueError(f"{flag} {text!r} mixes positional and name=value entries")
    if not all(named):
        if len(items) != len(names):
            raise ValueError(f"{flag} lists {len(items)} values for {len(names)} --detectors ({','.join(names)})")
        return kind[1](items, names, flag)
    table = {}
    for x in items:
        k, v = x.split("=", 1)
        if k in table:
            raise ValueError(f"{flag} names {k} twice")
        table[k] = v
    return _resolve(kind, table, names, flag)


_TEMPERATURES = ("temperature", lambda vals, names, source: [check_temperature(v, f"temperature of {n}") for v, n in zip(vals, names)])
_VARIANCE_SCALES = ("variance scale",
                    lambda vals, names, source: [check_variance_scale(v, f"variance scale of {n}") for v, n in zip(vals, names)])
_POOL_WEIGHTS = ("pool weight", lambda vals, names, source: check_pool_weights(vals, len(names), source))
_WBF_WEIGHTS = ("wbf weight", lambda vals, names, source: check_wbf_weights(vals, len(names), source))


def calibrated_probs(logits, T):
    """logits: CUDA tensor [M, K+1] (background last), T: one positive float.  Returns (p f64 [M, K], background f64 [M]):
    softmax(logits / T) in float64, the bits pe_proben_pack_logits writes for the same row."""
    _lib.require_cuda(logits)
    if logits.dim() != 2 or logits.shape[1] < 2:
        raise ValueError(f"calibrated_probs: logits must be [M, K+1] with K >= 1, got {tuple(logits.shape)}")
    logits = logits.contiguous().float()
    M, k1 = logits.shape
    out = torch.empty((M, k1), dtype=torch.float64, device=logits.device)
    st = _lib.lib().pe_calibrated_softmax(_lib.ptr(logits), M, k1, float(T), _lib.ptr(out), _lib.stream())
    _lib.check(st, "pe_calibrated_softmax")
    return out[:, :k1 - 1], out[:, k1 - 1]


def log_posteriors(logits, T):
    """logits: CUDA tensor [M, K+1] (background last).  Returns log_softmax(logits / T) f64 [M, K+1], the bits
    pe_proben_pack_log_posteriors writes for the same row."""
    _lib.require_cuda(logits)
    if logits.dim() != 2 or logits.shape[1] < 2:
        raise ValueError(f"log_posteriors: logits must be [M, K+1] with K >= 1, got {tuple(logits.shape)}")
    logits = logits.contiguous().float()
    M, k1 = logits.shape
    out = torch.empty((M, k1), dtype=torch.float64, device=logits.device)
    st = _lib.lib().pe_log_softmax(_lib.ptr(logits), M, k1, float(T), _lib.ptr(out), _lib.stream())
    _lib.check(st, "pe_log_softmax")
    return out


def check_class_prior(prior, num_columns=None, what="class_prior"):
    """K + 1 probabilities (background last) -> float64 ndarray normalised to sum 1.  Every entry must be finite and > 0 (its log
    is subtracted from the cluster's columns); anything else, or a length other than num_columns, raises ValueError."""
    try:
        p = np.asarray(prior, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} {prior!r} is not a list of numbers") from None
    if p.ndim != 1 or p.size < 2:
        raise ValueError(f"{what} must list K + 1 >= 2 probabilities (background last), got shape {p.shape}")
    if num_columns is not None and p.size != num_columns:
        raise ValueError(f"{what} lists {p.size} entries for K + 1 = {num_columns} columns (background last)")
    if not (np.all(np.isfinite(p)) and np.all(p > 0)):
        raise ValueError(f"{what} {p.tolist()} has an entry that is not finite and > 0")
    return p / p.sum()


def parse_class_prior(text):
    """--class_prior value 'a,b,...' (K + 1 numbers, background last) -> normalised float64 ndarray."""
    items = [x.strip() for x in str(text).split(",")]
    try:
        vals = [float(x) for x in items]
    except ValueError:
        raise ValueError(f"--class_prior {text!r} is not a comma separated list of numbers") from None
    return check_class_prior(vals, what="--class_prior")


def match_labels(boxes, classes, gt_boxes, gt_classes, iou_thresh=0.5, gt_crowd=None, num_classes=3):
    """Label of every detection for the fit: the class of the ground-truth box it overlaps most, at IoU >= iou_thresh, whatever
    class the detection itself predicted (`classes` only sizes the result: a confident wrong class is what the NLL must see);
    every other detection is background (label `num_classes`).  Ties go to the lower ground-truth index.  Crowd boxes
    (gt_crowd != 0) take no part, as FLIREvaluator never lets one count as a match for a true positive; annotations with
    `ignore` set are already dropped by data.load_coco_json.  boxes [n,4], gt_boxes [g,4] XYXY; returns int32 [n] (CPU)."""
    from .finetune import pairwise_iou
    boxes = torch.as_tensor(np.asarray(boxes, dtype=np.float64)).reshape(-1, 4)
    n = boxes.shape[0]
    assert len(classes) == n, f"match_labels: {len(classes)} classes for {n} boxes"
    labels = torch.full((n,), int(num_classes), dtype=torch.int32)
    gt_boxes = torch.as_tensor(np.asarray(gt_boxes, dtype=np.float64)).reshape(-1, 4)
    gt_classes = torch.as_tensor(np.asarray(gt_classes, dtype=np.int64)).reshape(-1)
    if gt_crowd is not None:
        keep = torch.as_tensor(np.asarray(gt_crowd)).reshape(-1) == 0
        gt_boxes, gt_classes = gt_boxes[keep], gt_classes[keep]
    if n == 0 or gt_boxes.shape[0] == 0:
        return labels
    iou = pairwise_iou(boxes, gt_boxes)                  # float64 [n, g]
    best = iou.max(dim=1).values
    first = (iou == best[:, None]).int().argmax(dim=1)   # the lowest index among equal maxima
    hit = best >= iou_thresh
    labels[hit] = gt_classes[first[hit]].to(torch.int32)
    return labels


def temperature_nll(logits, labels, temperatures):
    """(nll, d nll / d log T) per candidate, float64 numpy [n_t] each; logits CUDA f32 [M, K+1], labels CUDA i32 [M] in [0, K],
    at most 64 candidates.  One pe_temperature_nll launch; synchronises (the result and the bad-label flag come back together)."""
    _lib.require_cuda(logits, labels)
    logits = logits.contiguous().float()
    labels = labels.contiguous().to(torch.int32)
    M, k1 = logits.shape
    assert labels.shape == (M,), f"temperature_nll: {tuple(labels.shape)} labels for {M} rows"
    ts = [float(t) for t in temperatures]
    n_t = len(ts)
    host, bad, last = _statistic("pe_temperature_nll", 2 * n_t, NLL_MAX_BLOCKS * max(n_t, 1) * 2, logits.device,
                                 lambda work, out, flags, stream: _lib.lib().pe_temperature_nll(
                                     _lib.ptr(logits), _lib.ptr(labels), M, k1, (ctypes.c_double * max(n_t, 1))(*ts), n_t, work, out, flags, stream))
    if bad:
        raise ValueError(f"temperature_nll: {bad} of {M} rows have a label outside [0, {k1 - 1}] (row {last} is one, "
                         f"label {int(labels[last])})")
    out = host.numpy().reshape(n_t, 2)
    return out[:, 0].copy(), out[:, 1].copy()


def fit_temperature(logits, labels, lo=0.05, hi=20.0, tol=1e-6):
    """T in [lo, hi] that minimises sum_i -log softmax(logits_i / T)[label_i], by repeated 64-point bracketing over log T: every round
    evaluates 64 log-spaced candidates in one launch and keeps the interval in which d nll / d log T changes sign, until it is
    narrower than `tol` in log T.  The NLL is convex in 1 / T, so it has one minimum along log T and its derivative one sign change:
    the bracket holds the minimum.  (The derivative, not the NLL values, picks the interval: near the minimum the NLL differs
    between neighbours by less than float64 resolves, the derivative does not.)
    Returns a dict: T (the end of the final bracket with the smaller NLL), nll (at T), nll_at_1, dnll (d nll / d log T at T),
    bracket (T_lo, T_hi), bracket_dnll (the derivative at the two ends), rounds, rows, at_bound: "lo" / "hi" when the NLL still
    falls towards that end of [lo, hi] - the search range, not the data, decided T, which is then that end - else None."""
    lo, hi = check_temperature(lo, "lo"), check_temperature(hi, "hi")
    if not lo < hi:
        raise ValueError(f"fit_temperature: lo {lo} >= hi {hi}")
    a, b = math.log(lo), math.log(hi)
    rounds, at = 0, None
    while True:
        xs = np.linspace(a, b, NLL_CANDIDATES)
        nll, dn = temperature_nll(logits, labels, np.exp(xs))
        rounds += 1
        if not (np.all(np.isfinite(nll)) and np.all(np.isfinite(dn))):
            raise ValueError("fit_temperature: the NLL is not finite (non-finite logits?)")
        up = np.nonzero(dn >= 0)[0]
        j = int(up[0]) if len(up) else NLL_CANDIDATES
        if rounds == 1 and j in (0, NLL_CANDIDATES):       # rising from lo on, or still falling at hi
            at = "lo" if j == 0 else "hi"
            i = 0 if j == 0 else NLL_CANDIDATES - 1
            x, f, d, br, bd = xs[i], nll[i], dn[i], (xs[i], xs[i]), (dn[i], dn[i])
            break
        j = min(max(j, 1), NLL_CANDIDATES - 1)
        a, b = xs[j - 1], xs[j]
        if b - a < tol or rounds >= 32:
            i = j - 1 if nll[j - 1] <= nll[j] else j
            x, f, d, br, bd = xs[i], nll[i], dn[i], (a, b), (dn[j - 1], dn[j])
            break
    n1, _ = temperature_nll(logits, labels, [1.0])
    return {"T": float(math.exp(x)), "nll": float(f), "nll_at_1": float(n1[0]), "dnll": float(d),
            "bracket": (float(math.exp(br[0])), float(math.exp(br[1]))), "bracket_dnll": (float(bd[0]), float(bd[1])),
            "rounds": rounds, "rows": int(logits.shape[0]), "at_bound": at}


def save(path, detectors, nll=None, rows=None, class_prior=None, pool_weights=None, presence=None, box_correlation=None, **extra):
    """Write the calibration file.  detectors {name: T}; nll {name: {"before": .., "after": ..}}; rows {name: fitted rows};
    class_prior (optional, K + 1 probabilities, background last: the prior of score_fusion "probEn-log") is written normalised -
    without it the file has no such key; pool_weights (optional, {name: w}: the pooling weights of "probEn-log") likewise; presence
    (optional, {"detectors": [names in bit order], "columns": K + 1, "table": [2^D][K + 1], "hi": the fit's search bound or None}: the
    presence table of "probEn-log") likewise; box_correlation (optional, {"detectors": [names in matrix order], "matrix": [D][D], and what
    the fit reports: "raw", "shrink", "pairs", "rows", "excluded", "iou", "box_fusion"}: the correlation of box_fusion "c-avg") likewise; extra keys
    (cli/fit_temperature adds "holdout" and "fitted_image_ids") are kept as given."""
    rec = {"detectors": {k: check_temperature(v, f"temperature of {k}") for k, v in detectors.items()},
           "nll": nll or {}, "rows": rows or {}}
    if class_prior is not None:
        rec["class_prior"] = check_class_prior(class_prior).tolist()
    if pool_weights is not None:
        rec["pool_weights"] = _check_pool_table(pool_weights, "pool_weights")
    if presence is not None:
        rec["presence"] = _check_presence_record(presence, "presence")
    if box_correlation is not None:
        rec["box_correlation"] = _check_box_correlation_record(box_correlation, "box_correlation")
    rec.update(extra)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    return rec


def load(path):
    with open(path) as f:
        rec = json.load(f)
    if not isinstance(rec.get("detectors"), dict):
        raise ValueError(f"{path}: not a calibration file (no \"detectors\" table)")
    for k, v in rec["detectors"].items():
        check_temperature(v, f"{path}: temperature of {k}")
    if "class_prior" in rec:
        rec["class_prior"] = check_class_prior(rec["class_prior"], what=f"{path}: class_prior").tolist()
    if "pool_weights" in rec:
        rec["pool_weights"] = _check_pool_table(rec["pool_weights"], f"{path}: pool_weights")
    if "presence" in rec:
        rec["presence"] = _check_presence_record(rec["presence"], f"{path}: presence")
    if "box_correlation" in rec:
        rec["box_correlation"] = _check_box_correlation_record(rec["box_correlation"], f"{path}: box_correlation")
    return rec


def parse_temperatures(text, names):
    """--temperatures value -> [T per name].  'a,b[,c]' is matched by position, 'name=a,name=b' by name; not both."""
    return _parse(_TEMPERATURES, "--temperatures", text, names)


def resolve(table, names, source):
    """{name: T} -> [T per name]; every name must be there."""
    return _resolve(_TEMPERATURES, table, names, source)


def require_logits(det, name):
    """A prediction dict (late_fusion J1 schema) must carry K+1 logits for every detection; `name` = the file it came from."""
    rows = det.get("class_logits")
    if rows is None:
        raise ValueError(f"{name}: no class_logits: temperature calibration needs the detectors' logits "
                         "(write the predictions with cfg.MODEL.ROI_BOX_HEAD.OUTPUT_LOGITS)")
    for i, (lg, bx) in enumerate(zip(rows, det["boxes"])):
        if len(lg) != len(bx) or any(len(r) < 2 for r in lg):
            raise ValueError(f"{name}: no class_logits for the detections of image {i} ({det['image'][i]}): temperature calibration "
                             "needs the detectors' logits (write the predictions with cfg.MODEL.ROI_BOX_HEAD.OUTPUT_LOGITS)")


def calibrate_rows(logits, classes, T, device="cuda"):
    """Python lists of one detector's rows -> (probs f64 ndarray [n, K], scores f64 ndarray [n] = the row's own p_class)."""
    lg = torch.tensor(logits, dtype=torch.float32).reshape(len(logits), -1)
    if lg.shape[0] == 0:
        return np.zeros((0, max(lg.shape[1] - 1, 0))), np.zeros((0,))
    p, bg = calibrated_probs(lg.to(device), T)
    full = torch.cat([p, bg[:, None]], dim=1).cpu()
    cls = torch.tensor(classes, dtype=torch.int64)
    ok = (cls >= 0) & (cls < full.shape[1])
    score = torch.full((len(cls),), float("nan"), dtype=torch.float64)
    score[ok] = full[ok].gather(1, cls[ok, None])[:, 0]
    return full[:, :-1].numpy(), score.numpy()


def log_posterior_rows(logits, T, device="cuda"):
    """Python lists of one detector's rows -> log-posteriors f64 ndarray [n, K+1]."""
    lg = torch.tensor(logits, dtype=torch.float32).reshape(len(logits), -1)
    if lg.shape[0] == 0:
        return np.zeros((0, lg.shape[1]))
    return log_posteriors(lg.to(device), T).cpu().numpy()


def calibrate_j1(det, T, name="prediction file", device="cuda", log_probs=False):
    """A copy of a J1 prediction dict whose probs / scores are the calibrated ones, from its class_logits (one launch over all the
    file's rows).  Scores stay float64 here; they are rounded where the uncalibrated route rounds them.
    log_probs: also "log_probs" [n][K+1] per image, the rows' log-posteriors (score_fusion "probEn-log")."""
    require_logits(det, name)
    flat = [r for rows in det["class_logits"] for r in rows]
    cls = [c for rows in det["classes"] for c in rows]
    out = dict(det)
    if not flat:
        if log_probs:
            out["log_probs"] = [[] for _ in det["class_logits"]]
        return out
    p, s = calibrate_rows(flat, cls, T, device)
    probs, scores, k = [], [], 0
    for rows in det["class_logits"]:
        probs.append(p[k:k + len(rows)].tolist())
        scores.append(s[k:k + len(rows)].tolist())
        k += len(rows)
    out["probs"], out["scores"] = probs, scores
    if log_probs:
        lp = log_posterior_rows(flat, T, device)
        out["log_probs"], k = [], 0
        for rows in det["class_logits"]:
            out["log_probs"].append(lp[k:k + len(rows)].tolist())
            k += len(rows)
    return out


# ---- variance calibration ------------------------------------------------------------------------------------------------------

def check_variance_scale(s, what="variance scale"):
    return _finite_positive(s, what)


def check_variance_scales(scales, num_detectors, who):
    """variance_scales argument of the fusion entry points -> [s per detector] or None."""
    if scales is None:
        return None
    scales = list(scales)
    if len(scales) != num_detectors:
        raise ValueError(f"{who}: {len(scales)} variance scales for {num_detectors} detectors")
    return [check_variance_scale(s, f"variance scale of detector {k + 1}") for k, s in enumerate(scales)]


def match_rows_device(det_boxes, det_offsets, gt_boxes, gt_offsets, gt_classes, gt_crowd=None, iou_thresh=0.5, num_classes=3):
    """match_labels over flat device tensors, all images in one launch (pe_match_ground_truth).  det_boxes [M,4] XYXY with det_offsets
    [B+1], gt_boxes [G,4] with gt_offsets [B+1], gt_classes [G], gt_crowd [G] or None.  Returns (labels i32 [M], match i32 [M]: flat
    index into gt_boxes or -1, iou f64 [M]) on the device.  Labels outside [0, num_classes] are the caller's to fold."""
    _lib.require_cuda(det_boxes, det_offsets, gt_boxes, gt_offsets, gt_classes, gt_crowd)
    dev = det_boxes.device
    det_boxes = det_boxes.reshape(-1, 4).contiguous().double()
    gt_boxes = gt_boxes.reshape(-1, 4).contiguous().double()
    det_offsets = det_offsets.contiguous().to(torch.int32)
    gt_offsets = gt_offsets.contiguous().to(torch.int32)
    gt_classes = gt_classes.reshape(-1).contiguous().to(torch.int32)
    M, G, B = det_boxes.shape[0], gt_boxes.shape[0], det_offsets.numel() - 1
    if B < 0 or gt_offsets.numel() != B + 1 or gt_classes.numel() != G or (gt_crowd is not None and gt_crowd.numel() != G):
        raise ValueError(f"match_rows_device: {det_offsets.numel()} / {gt_offsets.numel()} offsets, {gt_classes.numel()} classes"
                         f"{'' if gt_crowd is None else f', {gt_crowd.numel()} crowd flags'} for {G} ground-truth boxes")
    ends = torch.stack([det_offsets[0], det_offsets[-1], gt_offsets[0], gt_offsets[-1]]).tolist()
    if ends != [0, M, 0, G]:
        raise ValueError(f"match_rows_device: offsets span {ends[:2]} / {ends[2:]} for {M} detections / {G} ground-truth boxes")
    labels = torch.full((M,), int(num_classes), dtype=torch.int32, device=dev)
    match = torch.full((M,), -1, dtype=torch.int32, device=dev)
    iou = torch.zeros((M,), dtype=torch.float64, device=dev)
    if M == 0 or G == 0 or B == 0:
        return labels, match, iou
    crowd = None if gt_crowd is None else gt_crowd.reshape(-1).contiguous().to(torch.int32)
    st = _lib.lib().pe_match_ground_truth(_lib.ptr(det_boxes), _lib.ptr(det_offsets), _lib.ptr(gt_boxes), _lib.ptr(gt_offsets),
                                         _lib.ptr(gt_classes), _lib.ptr(crowd), B, float(iou_thresh), int(num_classes),
                                         _lib.ptr(labels), _lib.ptr(match), _lib.ptr(iou), _lib.stream())
    _lib.check(st, "pe_match_ground_truth")
    return labels, match, iou


def variance_stats(det_boxes, match, gt_boxes, variances, scale=1.0, bbox_reg_weights=BBOX_REG_WEIGHTS):
    """One pe_variance_stats launch over the matched rows (device tensors: det_boxes [M,4], match i32 [M] into gt_boxes [G,4],
    variances [M]).  Returns {"n", "sum_q", "sum_log_var", "cover1", "cover2", "excluded", "last_excluded"}; synchronises."""
    _lib.require_cuda(det_boxes, match, gt_boxes, variances)
    scale = check_variance_scale(scale, "scale")
    det_boxes = det_boxes.reshape(-1, 4).contiguous().double()
    gt_boxes = gt_boxes.reshape(-1, 4).contiguous().double()
    match = match.reshape(-1).contiguous().to(torch.int32)
    variances = variances.reshape(-1).contiguous().double()
    M, G = det_boxes.shape[0], gt_boxes.shape[0]
    if match.numel() != M or variances.numel() != M:
        raise ValueError(f"variance_stats: {match.numel()} matches and {variances.numel()} variances for {M} rows")
    w = [float(x) for x in bbox_reg_weights]
    if len(w) != 4:
        raise ValueError(f"variance_stats: bbox_reg_weights {bbox_reg_weights!r} is not 4 numbers")
    host, bad, last = _statistic("pe_variance_stats", 5, VARIANCE_MAX_BLOCKS * 5, det_boxes.device,
                                 lambda work, out, flags, stream: _lib.lib().pe_variance_stats(
                                     _lib.ptr(det_boxes) if M else None, _lib.ptr(match) if M else None, _lib.ptr(gt_boxes) if G else None,
                                     _lib.ptr(variances) if M else None, M, G, (ctypes.c_float * 4)(*w), scale, work, out, flags, stream))
    n, sq, sl, c1, c2 = host.tolist()
    return {"n": int(n), "sum_q": sq, "sum_log_var": sl, "cover1": int(c1), "cover2": int(c2), "excluded": bad, "last_excluded": last}


def variance_nll(stats, s):
    """0.5 * (4 n log s + 4 sum log var + sum q / s): the Gaussian NLL of the rows at scale s, up to the constant 2 n log(2 pi)."""
    return 0.5 * (4 * stats["n"] * math.log(s) + 4 * stats["sum_log_var"] + stats["sum_q"] / s)


def fit_variance_scale(det_boxes, match, gt_boxes, variances, bbox_reg_weights=BBOX_REG_WEIGHTS):
    """s that minimises the Gaussian NLL of the matched rows' box-delta residuals under variance s * var_i: closed form
    s_hat = sum_i q_i / (4 n).  Two launches: at s = 1 (the sums and the coverage before), at s_hat (the coverage after).
    Returns {"scale", "nll_before", "nll_after", "rows", "excluded", "coverage_before", "coverage_after"}; coverage = the fractions
    of (row, coordinate) pairs within 1 and 2 standard deviations (0.6827 / 0.9545 for a calibrated Gaussian)."""
    a = variance_stats(det_boxes, match, gt_boxes, variances, 1.0, bbox_reg_weights)
    n = a["n"]
    if n == 0:
        raise ValueError(f"fit_variance_scale: no usable row ({a['excluded']} excluded: unmatched, a degenerate box or a variance that "
                         "is not finite and > 0)")
    s_hat = a["sum_q"] / (4 * n)
    if not (math.isfinite(s_hat) and s_hat > 0):
        raise ValueError(f"fit_variance_scale: the fitted scale {s_hat!r} is not finite and > 0 (every residual 0, or non-finite boxes)")
    b = variance_stats(det_boxes, match, gt_boxes, variances, s_hat, bbox_reg_weights)
    return {"scale": s_hat, "nll_before": variance_nll(a, 1.0), "nll_after": variance_nll(a, s_hat), "rows": n,
            "excluded": a["excluded"], "coverage_before": [a["cover1"] / (4 * n), a["cover2"] / (4 * n)],
            "coverage_after": [b["cover1"] / (4 * n), b["cover2"] / (4 * n)]}


def parse_variance_scales(text, names):
    """--variance_scales value -> [s per name].  'a,b[,c]' is matched by position, 'name=a,name=b' by name; not both."""
    return _parse(_VARIANCE_SCALES, "--variance_scales", text, names)


def resolve_variance_scales(table, names, source):
    """{name: s} -> [s per name]; every name must be there."""
    return _resolve(_VARIANCE_SCALES, table, names, source)


def save_variance(path, scales, nll=None, rows=None, excluded=None, coverage=None):
    """Add the variance keys to the calibration file at `path` (written by save): "variance_scales" {name: s}, "variance_nll"
    {name: {"before", "after"}}, "variance_rows", "variance_excluded", "variance_coverage" {name: {"before": [c1, c2], "after": ..}}.
    Everything else in the file stays as it is."""
    with open(path) as f:
        rec = json.load(f)
    if not isinstance(rec.get("detectors"), dict):
        raise ValueError(f"{path}: not a calibration file (no \"detectors\" table)")
    rec["variance_scales"] = {k: check_variance_scale(v, f"variance scale of {k}") for k, v in scales.items()}
    rec["variance_nll"], rec["variance_rows"] = nll or {}, rows or {}
    rec["variance_excluded"], rec["variance_coverage"] = excluded or {}, coverage or {}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
    return rec


def load_variance(path):
    """The calibration file's {name: s}, validated, or None when it carries no "variance_scales" (a file written without
    --with-variance: nothing is scaled)."""
    with open(path) as f:
        rec = json.load(f)
    table = rec.get("variance_scales")
    if table is None:
        return None
    if not isinstance(table, dict):
        raise ValueError(f"{path}: \"variance_scales\" is not a table of detector names")
    return {k: check_variance_scale(v, f"{path}: variance scale of {k}") for k, v in table.items()}


def scale_j1_vars(det, s):
    """A copy of a J1 prediction dict whose vars are s times the file's: float64 (the JSON's numbers are float64 already, and a
    float32 value read back from JSON is that float32 exactly) times s, one multiply - what pe_proben_pack_calibrated does."""
    s = check_variance_scale(s)
    out = dict(det)
    out["vars"] = [(np.asarray(v, dtype=np.float64) * s).tolist() for v in det["vars"]]
    return out


# ---- reliability ---------------------------------------------------------------------------------------------------------------

def summarise_reliability(counts, sums):
    """The per-bin statistics of pe_reliability_logits / pe_reliability_scores -> the figures, float64 on the host, in bin order.
    counts [B, 2] integers (rows, correct rows), sums [B, 2] (sum of conf, sum of the Brier term).  With N = all rows and, per
    non-empty bin, acc_b = correct_b / n_b and conf_b = conf_sum_b / n_b:
        ece = sum_b (n_b / N) |acc_b - conf_b|,   mce = max_b |acc_b - conf_b|,   brier = sum_b brier_sum_b / N;
    empty bins are skipped (their accuracy and confidence are NaN in the table) and N = 0 gives NaN for all three.
    Returns {"rows", "bins": [{"count", "correct", "conf_sum", "brier_sum", "accuracy", "confidence"}], "ece", "mce", "brier"}."""
    counts = np.asarray(counts).reshape(-1, 2)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 2)
    if counts.shape != sums.shape:
        raise ValueError(f"summarise_reliability: counts {counts.shape} and sums {sums.shape} do not list the same bins")
    N = sum(int(c) for c in counts[:, 0])
    nan = float("nan")
    bins, ece, mce, brier = [], 0.0, 0.0, 0.0
    for (n, k), (sc, sb) in zip(counts.tolist(), sums.tolist()):
        n, k = int(n), int(k)
        acc, conf = (k / n, sc / n) if n else (nan, nan)
        bins.append({"count": n, "correct": k, "conf_sum": sc, "brier_sum": sb, "accuracy": acc, "confidence": conf})
        if n:
            gap = abs(acc - conf)
            ece += (n / N) * gap
            mce = max(mce, gap)
            brier += sb / N
    if N == 0:
        ece = mce = brier = nan
    return {"rows": N, "bins": bins, "ece": ece, "mce": mce, "brier": brier}


def _check_bins(bins, who):
    if int(bins) != bins or not 1 <= int(bins) <= RELIABILITY_MAX_BINS:
        raise ValueError(f"{who}: bins {bins!r} is not an integer in [1, {RELIABILITY_MAX_BINS}]")
    return int(bins)


def _reliability_call(who, M, B, dev, launch):
    """The result slots are [counts i64 B x 2 | sums f64 B x 2]; launch(work, counts, sums, flags, stream) -> status."""
    host, bad, last = _statistic(who, 4 * B, RELIABILITY_MAX_BLOCKS * B * 4, dev, lambda work, out, flags, stream: launch(
        work, out, ctypes.c_void_p(out.value + 16 * B), flags, stream))
    out = summarise_reliability(host[:2 * B].view(torch.int64).numpy().reshape(B, 2), host[2 * B:].numpy().reshape(B, 2))
    out["excluded"], out["last_excluded"] = bad, last
    assert out["rows"] + bad == M, f"{who}: {out['rows']} rows binned and {bad} excluded of {M}"
    return out


def reliability(logits, labels, T=1.0, classes=None, bins=15):
    """Reliability of softmax(logits / T) against the labels: logits CUDA f32 [M, K+1] (background last), labels CUDA i32 [M] in
    [0, K].  classes CUDA i32 [M]: the confidence is the row's own p[class] and it is correct when label == class (the score ProbEn
    consumes); classes None: the top label over all K + 1 columns, the first index among equal maxima.  One pe_reliability_logits
    call and one download (synchronises).  Returns summarise_reliability's dict plus "excluded" (rows with a label or class outside
    [0, K], or a NaN confidence: they add nothing; reported, not raised) and "last_excluded" (such a row's index, -1 without one)."""
    _lib.require_cuda(logits, labels, classes)
    T, B = check_temperature(T), _check_bins(bins, "reliability")
    if logits.dim() != 2 or logits.shape[1] < 2:
        raise ValueError(f"reliability: logits must be [M, K+1] with K >= 1, got {tuple(logits.shape)}")
    logits = logits.contiguous().float()
    M, k1 = logits.shape
    labels = labels.reshape(-1).contiguous().to(torch.int32)
    if classes is not None:
        classes = classes.reshape(-1).contiguous().to(torch.int32)
    if labels.numel() != M or (classes is not None and classes.numel() != M):
        raise ValueError(f"reliability: {labels.numel()} labels{'' if classes is None else f' and {classes.numel()} classes'} for {M} rows")
    L = _lib.lib()
    return _reliability_call("pe_reliability_logits", M, B, logits.device, lambda work, cnt, sums, flags, stream: L.pe_reliability_logits(
        _lib.ptr(logits) if M else None, _lib.ptr(labels) if M else None, _lib.ptr(classes) if (M and classes is not None) else None,
        M, k1, T, B, work, cnt, sums, flags, stream))


def reliability_scores(conf, correct, bins=15):
    """The same dict for scores that come with their own verdict: conf CUDA f64 [M] in [0, 1], correct CUDA [M] (non-zero = correct).
    A conf that is NaN or outside [0, 1] excludes the row.  One pe_reliability_scores call and one download."""
    _lib.require_cuda(conf, correct)
    B = _check_bins(bins, "reliability_scores")
    conf = conf.reshape(-1).contiguous().double()
    correct = correct.reshape(-1).contiguous().to(torch.int32)
    M = conf.numel()
    if correct.numel() != M:
        raise ValueError(f"reliability_scores: {correct.numel()} verdicts for {M} scores")
    L = _lib.lib()
    return _reliability_call("pe_reliability_scores", M, B, conf.device, lambda work, cnt, sums, flags, stream: L.pe_reliability_scores(
        _lib.ptr(conf) if M else None, _lib.ptr(correct) if M else None, M, B, work, cnt, sums, flags, stream))


# ---- the fitter of the pooling weights and of the presence rows -------------------------------------------------------------------

def _projected_newton(evaluate, x0, lo, hi, gtol, used, max_rounds):
    """x in [lo, hi]^D that minimises a convex objective known only through evaluate(candidates [n, D]) -> (f [n], gradient [n, D]),
    from x0, by a projected Newton iteration with a line search.  Per round one evaluate gives the gradient at x and at x + h e_d (the
    Hessian's columns by forward differences, h = 1e-4, symmetrised), the ridged Newton system is solved over the coordinates that are
    not held at a bound (a coordinate is held at lo / hi when the gradient pushes it outwards), and a second evaluate tries the 40 step
    lengths 2, 1, 1/2, ... along the clipped direction; the step with the lowest f is taken if it is lower than the current one.  A
    direction that is not a descent direction (a nearly singular Hessian) is replaced by the scaled negative gradient.
    Stops when max_d |pg_d| <= gtol * used (pg_d = the gradient entry, 0 for a held coordinate), when no step length lowers f (float64
    resolution reached), or after max_rounds; one more evaluate at the final point.
    Returns (x, f, gradient, rounds, converged: the gradient criterion was met, at_bound [D]: "lo" / "hi" where f still falls beyond that
    end of [lo, hi], else None)."""
    D, h = len(x0), 1e-4
    x, rounds, converged = x0, 0, False
    while rounds < max_rounds:
        rounds += 1
        fs, gs = evaluate(np.vstack([x] + [x + h * np.eye(D)[d] for d in range(D)]))
        f, g = float(fs[0]), gs[0]
        held = ((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0))
        pg = np.where(held, 0.0, g)
        if np.max(np.abs(pg)) <= gtol * used:
            converged = True
            break
        H = (gs[1:] - g[None, :]) / h
        H = 0.5 * (H + H.T)
        free = ~held
        p = np.zeros(D)
        try:
            Hf = H[np.ix_(free, free)] + 1e-10 * max(np.trace(H), 1.0) * np.eye(int(free.sum()))
            p[free] = -np.linalg.solve(Hf, g[free])
        except np.linalg.LinAlgError:
            p[free] = -g[free]
        if not (np.all(np.isfinite(p)) and p @ g < 0):
            p = np.where(free, -g, 0.0) / max(np.max(np.abs(np.diag(H))), 1e-300)
        steps = 2.0 ** (1 - np.arange(40))
        trial = np.clip(x[None, :] + steps[:, None] * p[None, :], lo, hi)
        ft, _ = evaluate(trial)
        ft = np.where(np.isfinite(ft), ft, np.inf)
        i = int(np.argmin(ft))
        if not ft[i] < f:
            break
        x = trial[i]
    fs, gs = evaluate(x[None, :])
    g = gs[0]
    at = ["lo" if (x[d] <= lo and g[d] > 0) else "hi" if (x[d] >= hi and g[d] < 0) else None for d in range(D)]
    return x, float(fs[0]), g, rounds, converged, at


# ---- pooling weights -----------------------------------------------------------------------------------------------------------

def check_pool_weight(w, what="pool weight"):
    try:
        w = float(w)
    except (TypeError, ValueError):
        raise ValueError(f"{what} {w!r} is not a number") from None
    if not (math.isfinite(w) and w >= 0):
        raise ValueError(f"{what} {w!r} is not finite and >= 0")
    return w


def check_pool_weights(weights, num_detectors, who):
    """pool_weights argument of the fusion entry points -> [w per detector] or None.  Every w finite and >= 0, not all of them 0
    (the pooled posterior would be the prior), one per detector, at most POOL_MAX_DETECTORS."""
    if weights is None:
        return None
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().reshape(-1).tolist()
    weights = list(weights)
    if len(weights) != num_detectors:
        raise ValueError(f"{who}: {len(weights)} pool weights for {num_detectors} detectors")
    if not 1 <= num_detectors <= POOL_MAX_DETECTORS:
        raise ValueError(f"{who}: pool weights for {num_detectors} detectors (1 to {POOL_MAX_DETECTORS})")
    out = [check_pool_weight(w, f"{who}: pool weight of detector {k + 1}") for k, w in enumerate(weights)]
    if not any(w > 0 for w in out):
        raise ValueError(f"{who}: pool weights {out} are all 0")
    return out


WBF_MAX_DETECTORS = 8        # PE_WBF_MAX_DETECTORS


def check_wbf_weights(weights, num_detectors, who):
    """wbf_weights argument of the fusion entry points -> [u per detector] or None: the detector weights of weighted boxes fusion
    (score_fusion / box_fusion "wbf"), s = score * u.  Every u finite and >= 0, not all of them 0, one per detector, at most
    WBF_MAX_DETECTORS."""
    if weights is None:
        return None
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().reshape(-1).tolist()
    weights = list(weights)
    if len(weights) != num_detectors:
        raise ValueError(f"{who}: {len(weights)} wbf weights for {num_detectors} detectors")
    if not 1 <= num_detectors <= WBF_MAX_DETECTORS:
        raise ValueError(f"{who}: wbf weights for {num_detectors} detectors (1 to {WBF_MAX_DETECTORS})")
    out = [check_pool_weight(w, f"{who}: wbf weight of detector {k + 1}") for k, w in enumerate(weights)]
    if not any(w > 0 for w in out):
        raise ValueError(f"{who}: wbf weights {out} are all 0")
    return out


def check_wbf_skip(skip, who):
    """wbf_skip -> the score floor of weighted boxes fusion as a float: finite and >= 0 (rows with score * u below it are skipped)."""
    return check_pool_weight(skip, f"{who}: wbf_skip")


def parse_wbf_weights(text, names):
    """--wbf_weights value -> [u per name].  'a,b[,c]' is matched by position, 'name=a,name=b' by name; not both."""
    return _parse(_WBF_WEIGHTS, "--wbf_weights", str(text), names)


def _check_pool_table(table, what):
    if not isinstance(table, dict) or not table:
        raise ValueError(f"{what} is not a table of detector names")
    out = {k: check_pool_weight(v, f"{what}: pool weight of {k}") for k, v in table.items()}
    if not any(w > 0 for w in out.values()):
        raise ValueError(f"{what}: the pool weights are all 0")
    return out


def parse_pool_weights(text, names):
    """--pool_weights value -> [w per name].  'a,b[,c]' is matched by position, 'name=a,name=b' by name; not both."""
    return _parse(_POOL_WEIGHTS, "--pool_weights", str(text), names)          # as before, anything with a str() is taken


def resolve_pool_weights(table, names, source):
    """{name: w} -> [w per name]; every name must be there."""
    return _resolve(_POOL_WEIGHTS, table, names, source)


def pool_nll(log_probs, row_source, member_rows, cluster_offsets, labels, weights, log_prior=None):
    """One pe_pool_nll launch.  Device tensors: log_probs f64 [N, K+1], row_source i32 [N], the clusters in CSR form (member_rows i32
    [M] row indices, cluster_offsets i32 [C+1]), labels i32 [C] in [0, K], log_prior f64 [K+1] or None.  weights: [n_c, D] candidate
    vectors (n_c <= 64), finite and >= 0.  Returns (nll f64 ndarray [n_c], grad f64 ndarray [n_c, D], excluded clusters,
    last excluded cluster index or -1); an excluded cluster (fewer than 2 rows, a label outside [0, K], a row source outside [0, D))
    adds nothing.  Synchronises (one download)."""
    _lib.require_cuda(log_probs, row_source, member_rows, cluster_offsets, labels, log_prior)
    W = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
    if W.ndim != 2 or W.shape[0] < 1 or W.shape[1] < 1:
        raise ValueError(f"pool_nll: weights must be [candidates, detectors], got {W.shape}")
    n_c, D = W.shape
    if log_probs.dim() != 2 or log_probs.shape[1] < 2:
        raise ValueError(f"pool_nll: log_probs must be [N, K+1] with K >= 1, got {tuple(log_probs.shape)}")
    log_probs = log_probs.contiguous().double()
    N, k1 = log_probs.shape
    row_source = row_source.reshape(-1).contiguous().to(torch.int32)
    member_rows = member_rows.reshape(-1).contiguous().to(torch.int32)
    cluster_offsets = cluster_offsets.reshape(-1).contiguous().to(torch.int32)
    labels = labels.reshape(-1).contiguous().to(torch.int32)
    C, M = labels.numel(), member_rows.numel()
    if row_source.numel() != N or cluster_offsets.numel() != C + 1:
        raise ValueError(f"pool_nll: {row_source.numel()} sources for {N} rows, {cluster_offsets.numel()} offsets for {C} clusters")
    if log_prior is not None:
        log_prior = log_prior.reshape(-1).contiguous().double()
        if log_prior.numel() != k1:
            raise ValueError(f"pool_nll: log_prior lists {log_prior.numel()} entries for K + 1 = {k1} columns")
    host, bad, last = _statistic("pe_pool_nll", n_c * (1 + D), n_c * (D + POOL_NLL_MAX_BLOCKS * (1 + D)), log_probs.device,
                                 lambda work, out, flags, stream: _lib.lib().pe_pool_nll(
                                     _lib.ptr(log_probs) if N else None, _lib.ptr(row_source) if N else None, N, k1,
                                     _lib.ptr(member_rows) if M else None, M, _lib.ptr(cluster_offsets), _lib.ptr(labels) if C else None, C,
                                     _lib.ptr(log_prior), W.ctypes.data_as(ctypes.c_void_p), n_c, D, work, out, flags, stream))
    out = host.numpy().reshape(n_c, 1 + D)
    return out[:, 0].copy(), out[:, 1:].copy(), bad, last


def fit_pool_weights(log_probs, row_source, member_rows, cluster_offsets, labels, num_detectors, log_prior=None, hi=64.0,
                     gtol=1e-7, max_rounds=60):
    """w in [0, hi]^D that minimises the NLL of the pooled posterior against the clusters' labels (pool_nll's inputs).  The NLL is
    convex in w, so a projected Newton iteration with a line search finds its minimum: per round one launch evaluates the gradient at
    w and at w + h e_d (the Hessian's columns by forward differences, h = 1e-4, symmetrised), the Newton system is solved over the
    coordinates that are not held at a bound (a coordinate is held at 0 / hi when the gradient pushes it outwards), and a second
    launch evaluates up to 40 step lengths 2, 1, 1/2, ... along the clipped direction; the step with the lowest NLL is taken if
    it is lower than the current one.  A direction that is not a descent direction (a nearly singular Hessian: two detectors that
    are copies of each other) is replaced by the negative gradient.
    Stops when the projected gradient satisfies max_d |pg_d| <= gtol * clusters used (pg_d = the gradient entry, 0 for a coordinate
    held at a bound), when no step length lowers the NLL (float64 resolution of the NLL reached), or after max_rounds.
    Returns a dict: weights [D], nll (at weights), nll_at_1, grad [D] (at weights), clusters (used), excluded, rounds, converged
    (the gradient criterion was met), at_bound [D]: "lo" / "hi" where the NLL still falls beyond that end of [0, hi], else None."""
    D = int(num_detectors)
    if not 1 <= D <= POOL_MAX_DETECTORS:
        raise ValueError(f"fit_pool_weights: {D} detectors (1 to {POOL_MAX_DETECTORS})")
    hi = check_pool_weight(hi, "hi")
    if not hi > 1.0:
        raise ValueError(f"fit_pool_weights: hi {hi} <= 1 (the start of the search)")
    C = int(labels.numel())
    args = (log_probs, row_source, member_rows, cluster_offsets, labels)
    f1, _, bad, _ = pool_nll(*args, [np.ones(D)], log_prior)
    used = C - bad
    if used <= 0:
        raise ValueError(f"fit_pool_weights: no usable cluster ({bad} of {C} excluded: fewer than 2 rows, a label or a row source "
                         "out of range)")
    if not math.isfinite(f1[0]):
        raise ValueError("fit_pool_weights: the NLL at w = 1 is not finite (non-finite log-posteriors?)")
    w, f, g, rounds, converged, at = _projected_newton(lambda cand: pool_nll(*args, cand, log_prior)[:2], np.ones(D), 0.0, hi, gtol, used,
                                                       max_rounds)
    return {"weights": [float(x) for x in w], "nll": f, "nll_at_1": float(f1[0]), "grad": [float(x) for x in g], "clusters": used,
            "excluded": bad, "rounds": rounds, "converged": converged, "at_bound": at}


# ---- presence evidence ---------------------------------------------------------------------------------------------------------

def check_presence(table, num_detectors=None, num_columns=None, what="presence"):
    """The presence table -> float64 ndarray [2^D, K + 1]: one row of log-evidence per presence pattern P = OR of (1 << detector), row
    0 (no detector: no cluster has it) present and ignored.  1 <= D <= PRESENCE_MAX_DETECTORS, K + 1 >= 2, every entry finite (row 0
    too: it is uploaded with the rest); anything else, or a shape other than the one asked for, raises ValueError."""
    if isinstance(table, torch.Tensor):
        table = table.detach().cpu().numpy()
    try:
        t = np.asarray(table, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} {table!r} is not a table of numbers") from None
    if t.ndim != 2 or t.shape[1] < 2:
        raise ValueError(f"{what} must be a table [2^D][K + 1] with K + 1 >= 2 columns, got shape {t.shape}")
    rows = [2 ** d for d in range(1, PRESENCE_MAX_DETECTORS + 1)]
    if t.shape[0] not in rows:
        raise ValueError(f"{what} has {t.shape[0]} rows: one per presence pattern, row 0 included, is {' / '.join(map(str, rows))} "
                         f"(1 to {PRESENCE_MAX_DETECTORS} detectors)")
    if num_detectors is not None and t.shape[0] != 2 ** int(num_detectors):
        raise ValueError(f"{what} has {t.shape[0]} rows for {num_detectors} detectors ({2 ** int(num_detectors)} patterns, row 0 included)")
    if num_columns is not None and t.shape[1] != num_columns:
        raise ValueError(f"{what} has {t.shape[1]} columns for K + 1 = {num_columns} (background last)")
    if not np.all(np.isfinite(t)):
        r, c = np.argwhere(~np.isfinite(t))[0]
        raise ValueError(f"{what}: entry {t[r, c]!r} (pattern {r}, column {c}) is not finite")
    return np.ascontiguousarray(t)


def presence_table(table, num_detectors, num_columns, device):
    """The presence table (check_presence validates: shape, finite entries, row 0 present and ignored) -> the DEVICE f64 [2^D, K + 1]
    tensor pe_proben_fuse_batch_presence takes.  None -> None.  A CUDA tensor is taken as the result of an earlier call
    (FramePairPipeline uploads once, not per batch); num_detectors None takes D from the table's rows."""
    if table is None:
        return None
    if isinstance(table, torch.Tensor) and table.is_cuda:
        want = (None if num_detectors is None else 2 ** int(num_detectors), num_columns)
        if table.dtype != torch.float64 or table.dim() != 2 or (want[0] is not None and table.shape[0] != want[0]) or table.shape[1] != num_columns \
                or table.shape[0] not in [2 ** d for d in range(1, PRESENCE_MAX_DETECTORS + 1)]:
            raise ValueError(f"presence tensor {tuple(table.shape)} {table.dtype} is not float64 [{want[0] or '2^D'}, {num_columns}]")
        return table.contiguous()
    return torch.from_numpy(check_presence(table, num_detectors, num_columns)).to(device)


def presence_detectors(table):
    """D of a table (host or device) with 2^D rows."""
    return int(table.shape[0]).bit_length() - 1


def _pattern_of(text, names, flag):
    parts = [x.strip() for x in text.split("+")]
    mask = 0
    for n in parts:
        if n not in names:
            raise ValueError(f"{flag}: unknown detector {n!r} in pattern {text!r} (the detectors are {','.join(names)})")
        if mask & (1 << names.index(n)):
            raise ValueError(f"{flag}: pattern {text!r} names {n} twice")
        mask |= 1 << names.index(n)
    return mask


def parse_presence(text, names, num_columns=None):
    """--presence value -> float64 ndarray [2^D, K + 1], D = len(names).  One entry per pattern, 'name[+name...]=v:v:...:v' (K + 1
    numbers, background last), entries separated by commas; a detector's bit is its position in names; patterns not listed get zeros."""
    names = list(names)
    flag = "--presence"
    if not 1 <= len(names) <= PRESENCE_MAX_DETECTORS:
        raise ValueError(f"{flag}: {len(names)} detectors (1 to {PRESENCE_MAX_DETECTORS})")
    rows = {}
    for item in [x.strip() for x in str(text).split(",") if x.strip()]:
        if "=" not in item:
            raise ValueError(f"{flag}: entry {item!r} is not pattern=v:v:...")
        k, v = item.split("=", 1)
        mask = _pattern_of(k, names, flag)
        if mask in rows:
            raise ValueError(f"{flag} lists pattern {'+'.join(n for d, n in enumerate(names) if mask >> d & 1)} twice")
        try:
            vals = [float(x) for x in v.split(":")]
        except ValueError:
            raise ValueError(f"{flag}: entry {item!r} is not a ':' separated list of numbers") from None
        rows[mask] = (vals, k)
    if not rows:
        raise ValueError(f"{flag} {text!r} lists no pattern")
    k1 = num_columns if num_columns is not None else len(next(iter(rows.values()))[0])
    table = np.zeros((2 ** len(names), k1))
    for mask, (vals, k) in rows.items():
        if len(vals) != k1:
            raise ValueError(f"{flag}: pattern {k} lists {len(vals)} entries for K + 1 = {k1} columns (background last)")
        if not all(math.isfinite(x) for x in vals):
            raise ValueError(f"{flag}: pattern {k} has an entry that is not finite ({vals})")
        table[mask] = vals
    return check_presence(table, len(names), k1, flag)


def _check_presence_record(rec, what):
    if not isinstance(rec, dict) or not isinstance(rec.get("detectors"), list) or "table" not in rec:
        raise ValueError(f"{what} is not a presence record (\"detectors\": names in bit order, \"columns\", \"table\")")
    names = [str(n) for n in rec["detectors"]]
    if len(set(names)) != len(names):
        raise ValueError(f"{what}: detectors {names} repeat a name")
    t = check_presence(rec["table"], len(names), rec.get("columns"), f"{what}: table")
    hi = rec.get("hi")
    out = dict(rec)
    out.update({"detectors": names, "columns": int(t.shape[1]), "table": t.tolist(), "hi": None if hi is None else float(hi)})
    return out


def resolve_presence(rec, names, source):
    """The calibration file's "presence" record -> float64 ndarray [2^D, K + 1] with the bits in the order of `names`.  The file's
    detectors must be exactly `names` (in any order): a table over other detectors is a table about other observations."""
    rec = _check_presence_record(rec, f"{source}: presence")
    names = list(names)
    if sorted(rec["detectors"]) != sorted(names):
        raise ValueError(f"{source}: the presence table is over {','.join(rec['detectors'])}, not {','.join(names)}")
    src = np.asarray(rec["table"], dtype=np.float64)
    bit = [names.index(n) for n in rec["detectors"]]          # file bit d -> bit of this run
    out = np.zeros_like(src)
    for p in range(src.shape[0]):
        q = sum(1 << bit[d] for d in range(len(names)) if p >> d & 1)
        out[q] = src[p]
    return out


def bias_nll(base, labels, candidates):
    """One pe_bias_nll launch.  Device tensors: base f64 [C, K+1] (the fused log-posteriors of one pattern's clusters at a zero table),
    labels i32 [C] in [0, K].  candidates: [n_c, K+1] candidate table rows (n_c <= 64), finite.  Returns (nll f64 ndarray [n_c], grad f64
    ndarray [n_c, K+1], excluded clusters, last excluded cluster index or -1); an excluded cluster (a label outside [0, K], a non-finite
    base entry) adds nothing.  K + 1 <= BIAS_NLL_MAX_COLUMNS.  Synchronises (one download)."""
    _lib.require_cuda(base, labels)
    cand = np.ascontiguousarray(np.asarray(candidates, dtype=np.float64))
    if cand.ndim != 2 or cand.shape[0] < 1:
        raise ValueError(f"bias_nll: candidates must be [candidates, K+1], got {cand.shape}")
    n_c, k1 = cand.shape
    if base.dim() != 2 or base.shape[1] != k1:
        raise ValueError(f"bias_nll: base must be [C, {k1}] for candidates of {k1} columns, got {tuple(base.shape)}")
    base = base.contiguous().double()
    labels = labels.reshape(-1).contiguous().to(torch.int32)
    C = base.shape[0]
    if labels.numel() != C:
        raise ValueError(f"bias_nll: {labels.numel()} labels for {C} clusters")
    host, bad, last = _statistic("pe_bias_nll", n_c * (1 + k1), n_c * (k1 + BIAS_NLL_MAX_BLOCKS * (1 + k1)), base.device,
                                 lambda work, out, flags, stream: _lib.lib().pe_bias_nll(
                                     _lib.ptr(base) if C else None, _lib.ptr(labels) if C else None, C, k1,
                                     cand.ctypes.data_as(ctypes.c_void_p), n_c, work, out, flags, stream))
    out = host.numpy().reshape(n_c, 1 + k1)
    return out[:, 0].copy(), out[:, 1:].copy(), bad, last


def _fit_bias(base, labels, hi, gtol, max_rounds):
    """One row of the table: b in [-hi, hi]^K x {0} that minimises bias_nll, by _projected_newton over b[:K]."""
    C, k1 = base.shape
    K = k1 - 1
    b = np.zeros(k1)
    f0, _, bad, _ = bias_nll(base, labels, [b])
    used = C - bad
    rec = {"clusters": used, "excluded": bad, "nll_at_0": float(f0[0]), "nll": float(f0[0]), "rounds": 0, "converged": used == 0,
           "at_bound": [None] * K, "grad": [0.0] * K}
    if used == 0:
        return b, rec
    if not math.isfinite(f0[0]):
        raise ValueError("fit_presence: the NLL at a zero row is not finite")

    def evaluate(cand):          # the background column is pinned at 0
        fs, gs, _, _ = bias_nll(base, labels, np.hstack([cand, np.zeros((len(cand), 1))]))
        return fs, gs[:, :K]
    x, f, g, rounds, converged, at = _projected_newton(evaluate, np.zeros(K), -hi, hi, gtol, used, max_rounds)
    rec.update({"nll": f, "rounds": rounds, "converged": converged, "grad": [float(v) for v in g], "at_bound": at})
    return np.append(x, 0.0), rec


def fit_presence(base, patterns, labels, num_detectors, hi=16.0, gtol=1e-7, max_rounds=60):
    """The presence table that minimises the NLL of softmax(base + presence[pattern]) against the clusters' labels.  Device tensors:
    base f64 [C, K+1] (the fused log-posterior of every cluster at a ZERO table: pe_proben_fuse_batch_presence's out_log_posterior,
    clusters of one and passthrough rows included), patterns i32 [C] (its out_pattern), labels i32 [C] in [0, K].  Patterns do not
    interact: per pattern P in [1, 2^D) its clusters are selected with torch indexing on the device and the row b = presence[P] is a
    bias-only softmax regression, convex, gauge b_K = 0 (background is the reference column), fitted by fit_pool_weights' projected
    Newton scheme over b[:K] in the box [-hi, hi]^K: per round one launch evaluates the gradient at b and at b + h e_j (the Hessian's
    columns by forward differences, h = 1e-4, symmetrised), a second one 40 step lengths 2, 1, 1/2, ...; it stops when the projected
    gradient satisfies max_j |pg_j| <= gtol * clusters used, when no step lowers the NLL, or after max_rounds.  hi is a search domain,
    not a prior: a pattern in which some label never occurs has its minimum at infinity and stops there, reported in at_bound.
    A pattern without clusters (or with every cluster excluded) keeps a zero row.  Clusters whose pattern is outside [1, 2^D) (a row
    with a bad source) belong to no row and are counted in "unassigned".
    Returns {"table": [2^D][K+1], "hi", "unassigned", "patterns": {P: {"clusters", "excluded", "nll_at_0", "nll", "rounds",
    "converged", "at_bound" [K], "grad" [K]}}}."""
    D = int(num_detectors)
    if not 1 <= D <= PRESENCE_MAX_DETECTORS:
        raise ValueError(f"fit_presence: {D} detectors (1 to {PRESENCE_MAX_DETECTORS})")
    hi = float(hi)
    if not (math.isfinite(hi) and hi > 0):
        raise ValueError(f"fit_presence: hi {hi!r} is not finite and > 0")
    _lib.require_cuda(base, patterns, labels)
    if base.dim() != 2 or not 2 <= base.shape[1] <= BIAS_NLL_MAX_COLUMNS:
        raise ValueError(f"fit_presence: base must be [C, K+1] with 2 <= K + 1 <= {BIAS_NLL_MAX_COLUMNS}, got {tuple(base.shape)}")
    C, k1 = base.shape
    patterns, labels = patterns.reshape(-1), labels.reshape(-1)
    if patterns.numel() != C or labels.numel() != C:
        raise ValueError(f"fit_presence: {patterns.numel()} patterns and {labels.numel()} labels for {C} clusters")
    table = np.zeros((2 ** D, k1))
    report = {}
    assigned = 0
    for P in range(1, 2 ** D):
        idx = torch.nonzero(patterns == P).flatten()
        assigned += int(idx.numel())
        b, rec = _fit_bias(base[idx], labels[idx], hi, gtol, max_rounds)
        table[P] = b
        report[P] = rec
    return {"table": table.tolist(), "hi": hi, "unassigned": C - assigned, "patterns": report}


# ---- correlated box fusion ("c-avg") --------------------------------------------------------------------------------------------

BOX_PAIRS = [(a, b) for a in range(BOX_CORR_MAX_DETECTORS) for b in range(a, BOX_CORR_MAX_DETECTORS)]      # pe_box_pair_stats' order


def box_correlation_min_eig(matrix):
    """The smallest eigenvalue of the matrix with its diagonal set to 1: the correlation matrix of a cluster that holds one row of
    every detector."""
    p = np.array(matrix, dtype=np.float64)
    np.fill_diagonal(p, 1.0)
    return float(np.linalg.eigvalsh(p)[0])


def check_box_correlation(matrix, num_detectors=None, what="box_correlation"):
    """The box-error correlation of box_fusion "c-avg" -> float64 ndarray [D, D], 1 <= D <= BOX_CORR_MAX_DETECTORS.  Entry [a][b], a != b:
    the correlation of the normalised box errors of a row of detector a and a row of detector b in one cluster; entry [d][d]: the same
    for two DIFFERENT rows of detector d (not 1: a row's correlation with itself is).  Every entry finite, the matrix symmetric,
    0 <= [d][d] < 1, and the matrix with its diagonal set to 1 - the correlation matrix of a cluster with one row per detector -
    positive semidefinite (numpy.linalg.eigvalsh, smallest eigenvalue >= -1e-12).  Anything else raises ValueError.
    A cluster's correlation matrix is R = diag(1 - [d][d]) + G P G'.  It is positive definite for every cluster with at most one row
    per detector (when the eigenvalue above is > 0); with several rows of one detector it is for every composition only if P itself is
    positive semidefinite, which a zero diagonal beside a non-zero off-diagonal entry never is (two rows of detector a that share
    nothing cannot both share much with a row of b).  pe_box_gls_batch answers a cluster whose R is not positive definite with NaN."""
    if isinstance(matrix, torch.Tensor):
        matrix = matrix.detach().cpu().numpy()
    try:
        p = np.asarray(matrix, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} {matrix!r} is not a matrix of numbers") from None
    if p.ndim != 2 or p.shape[0] != p.shape[1] or not 1 <= p.shape[0] <= BOX_CORR_MAX_DETECTORS:
        raise ValueError(f"{what} must be a square matrix over 1 to {BOX_CORR_MAX_DETECTORS} detectors, got shape {p.shape}")
    if num_detectors is not None and p.shape[0] != int(num_detectors):
        raise ValueError(f"{what} is over {p.shape[0]} detectors, not {num_detectors}")
    if not np.all(np.isfinite(p)):
        r, c = np.argwhere(~np.isfinite(p))[0]
        raise ValueError(f"{what}: entry {p[r, c]!r} ({r}, {c}) is not finite")
    if not np.array_equal(p, p.T):
        r, c = np.argwhere(p != p.T)[0]
        raise ValueError(f"{what} is not symmetric: entry ({r}, {c}) is {p[r, c]!r}, entry ({c}, {r}) is {p[c, r]!r}")
    for d in range(p.shape[0]):
        if not 0.0 <= p[d, d] < 1.0:
            raise ValueError(f"{what}: diagonal entry {d} is {p[d, d]!r}, not in [0, 1): it is the correlation of two different rows of "
                             "one detector")
    low = box_correlation_min_eig(p)
    if low < -1e-12:
        raise ValueError(f"{what} is not positive semidefinite with a unit diagonal (smallest eigenvalue {low:.3g}): no joint distribution "
                         "of one row per detector has these correlations")
    return np.ascontiguousarray(p)


def box_correlation_tensor(matrix, num_detectors, device):
    """The correlation matrix (check_box_correlation validates) -> the DEVICE f64 [D, D] tensor pe_box_gls_batch takes.  None -> None.
    A CUDA tensor is taken as the result of an earlier call (FramePairPipeline uploads once, not per batch); num_detectors None takes
    D from the matrix."""
    if matrix is None:
        return None
    if isinstance(matrix, torch.Tensor) and matrix.is_cuda:
        D = matrix.shape[0] if matrix.dim() == 2 else -1
        if matrix.dtype != torch.float64 or matrix.dim() != 2 or matrix.shape[1] != D or not 1 <= D <= BOX_CORR_MAX_DETECTORS \
                or (num_detectors is not None and D != int(num_detectors)):
            raise ValueError(f"box-correlation tensor {tuple(matrix.shape)} {matrix.dtype} is not float64 "
                             f"[{num_detectors or 'D'}, {num_detectors or 'D'}]")
        return matrix.contiguous()
    return torch.from_numpy(check_box_correlation(matrix, num_detectors)).to(device)


def parse_box_correlation(text, names):
    """--box_correlation value -> float64 ndarray [D, D], D = len(names).  'name:name=value,...': one entry per detector pair (the same
    name twice: the diagonal entry of that detector), pairs not listed get 0.  A bare number stands for the off-diagonal entry of two
    detectors, diagonal 0."""
    names, flag = list(names), "--box_correlation"
    D = len(names)
    if not 1 <= D <= BOX_CORR_MAX_DETECTORS:
        raise ValueError(f"{flag}: {D} detectors (1 to {BOX_CORR_MAX_DETECTORS})")
    items = [x.strip() for x in str(text).split(",") if x.strip()]
    if not items:
        raise ValueError(f"{flag} {text!r} lists no pair")
    p = np.zeros((D, D))
    if len(items) == 1 and "=" not in items[0]:
        if D != 2:
            raise ValueError(f"{flag}: a bare number stands for the one pair of two detectors; with {D} ({','.join(names)}) write name:name=value")
        try:
            p[0, 1] = p[1, 0] = float(items[0])
        except ValueError:
            raise ValueError(f"{flag}: {items[0]!r} is neither a number nor name:name=value") from None
        return check_box_correlation(p, D, flag)
    seen = set()
    for item in items:
        if "=" not in item or item.split("=", 1)[0].count(":") != 1:
            raise ValueError(f"{flag}: entry {item!r} is not name:name=value")
        k, v = item.split("=", 1)
        pair = [x.strip() for x in k.split(":")]
        for n in pair:
            if n not in names:
                raise ValueError(f"{flag}: unknown detector {n!r} in {item!r} (the detectors are {','.join(names)})")
        a, b = sorted(names.index(n) for n in pair)
        if (a, b) in seen:
            raise ValueError(f"{flag} lists the pair {names[a]}:{names[b]} twice")
        seen.add((a, b))
        try:
            p[a, b] = p[b, a] = float(v)
        except ValueError:
            raise ValueError(f"{flag}: entry {item!r} is not name:name=value with a number") from None
    return check_box_correlation(p, D, flag)


def _check_box_correlation_record(rec, what):
    if not isinstance(rec, dict) or not isinstance(rec.get("detectors"), list) or "matrix" not in rec:
        raise ValueError(f"{what} is not a box-correlation record (\"detectors\": names in matrix order, \"matrix\")")
    names = [str(n) for n in rec["detectors"]]
    if len(set(names)) != len(names):
        raise ValueError(f"{what}: detectors {names} repeat a name")
    out = dict(rec)
    out.update({"detectors": names, "matrix": check_box_correlation(rec["matrix"], len(names), f"{what}: matrix").tolist()})
    return out


def resolve_box_correlation(rec, names, source):
    """The calibration file's "box_correlation" record -> float64 ndarray [D, D] in the order of `names`.  The file's detectors must be
    exactly `names` (in any order): a correlation over other detectors is a statement about other errors."""
    rec = _check_box_correlation_record(rec, f"{source}: box_correlation")
    names = list(names)
    if sorted(rec["detectors"]) != sorted(names):
        raise ValueError(f"{source}: the box correlation is over {','.join(rec['detectors'])}, not {','.join(names)}")
    src = np.asarray(rec["matrix"], dtype=np.float64)
    at = [rec["detectors"].index(n) for n in names]
    return np.ascontiguousarray(src[np.ix_(at, at)])


def box_pair_stats(row_boxes, row_vars, row_source, member_rows, cluster_offsets, cluster_match, gt_boxes, num_detectors,
                   bbox_reg_weights=BBOX_REG_WEIGHTS):
    """One pe_box_pair_stats call.  Device tensors: the packed rows (row_boxes f64 [N, 4], row_vars f64 [N], row_source i32 [N]), the
    clusters in CSR form (member_rows i32 [M], cluster_offsets i32 [C+1]), cluster_match i32 [C] (each cluster's ground-truth box in
    gt_boxes [G, 4], -1: none - the cluster adds nothing).  Returns {"pairs": int ndarray [D, D] (N_ab, symmetric), "rows": [M_d],
    "S": f64 ndarray [D, D] (symmetric), "Q": [Q_d], "excluded", "last_excluded"}; synchronises."""
    D = int(num_detectors)
    if not 1 <= D <= BOX_CORR_MAX_DETECTORS:
        raise ValueError(f"box_pair_stats: {D} detectors (1 to {BOX_CORR_MAX_DETECTORS})")
    _lib.require_cuda(row_boxes, row_vars, row_source, member_rows, cluster_offsets, cluster_match, gt_boxes)
    row_boxes = row_boxes.reshape(-1, 4).contiguous().double()
    row_vars = row_vars.reshape(-1).contiguous().double()
    row_source = row_source.reshape(-1).contiguous().to(torch.int32)
    member_rows = member_rows.reshape(-1).contiguous().to(torch.int32)
    cluster_offsets = cluster_offsets.reshape(-1).contiguous().to(torch.int32)
    cluster_match = cluster_match.reshape(-1).contiguous().to(torch.int32)
    gt_boxes = gt_boxes.reshape(-1, 4).contiguous().double()
    N, M, C, G = row_boxes.shape[0], member_rows.numel(), cluster_match.numel(), gt_boxes.shape[0]
    if row_vars.numel() != N or row_source.numel() != N or cluster_offsets.numel() != C + 1:
        raise ValueError(f"box_pair_stats: {row_vars.numel()} variances and {row_source.numel()} sources for {N} rows, "
                         f"{cluster_offsets.numel()} offsets for {C} clusters")
    if C and cluster_offsets[[0, -1]].tolist() != [0, M]:
        raise ValueError(f"box_pair_stats: cluster_offsets span {cluster_offsets[[0, -1]].tolist()} for {M} member rows")
    w = [float(x) for x in bbox_reg_weights]
    if len(w) != 4:
        raise ValueError(f"box_pair_stats: bbox_reg_weights {bbox_reg_weights!r} is not 4 numbers")
    nv = 2 * (len(BOX_PAIRS) + BOX_CORR_MAX_DETECTORS)
    host, bad, last = _statistic("pe_box_pair_stats", nv, 6 * M + (M + 1) // 2 + nv * BOX_PAIR_MAX_BLOCKS, row_boxes.device,
                                 lambda work, out, flags, stream: _lib.lib().pe_box_pair_stats(
                                     _lib.ptr(row_boxes) if N else None, _lib.ptr(row_vars) if N else None, _lib.ptr(row_source) if N else None,
                                     N, _lib.ptr(member_rows) if M else None, M, _lib.ptr(cluster_offsets), _lib.ptr(cluster_match) if C else None,
                                     C, _lib.ptr(gt_boxes) if G else None, G, D, (ctypes.c_float * 4)(*w), work, out, flags, stream))
    counts = host[:nv // 2].view(torch.int64).tolist()
    sums = host[nv // 2:].tolist()
    pairs, S = np.zeros((D, D), dtype=np.int64), np.zeros((D, D))
    for i, (a, b) in enumerate(BOX_PAIRS):
        if b < D:
            pairs[a, b] = pairs[b, a] = counts[i]
            S[a, b] = S[b, a] = sums[i]
    return {"pairs": pairs, "rows": counts[len(BOX_PAIRS):][:D], "S": S, "Q": sums[len(BOX_PAIRS):][:D], "excluded": bad,
            "last_excluded": last}


def shrink_to_psd(raw, tol=1e-9):
    """raw (symmetric) -> (matrix, factor): every off-diagonal entry times the largest factor in [0, 1] at which check_box_correlation's
    eigenvalue (box_correlation_min_eig: the matrix with a unit diagonal) is >= -1e-12.  That eigenvalue is concave in the factor and 1
    at 0, so the factors that work are an interval from 0: bisection to `tol`.  A matrix that passes already is returned as it is,
    factor 1."""
    raw = np.asarray(raw, dtype=np.float64)
    diag = np.diag(np.diag(raw))
    off = raw - diag

    def ok(f):
        return box_correlation_min_eig(diag + f * off) >= -1e-12
    if ok(1.0):
        return raw.copy(), 1.0
    lo, hi = 0.0, 1.0
    while hi - lo > tol:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return diag + lo * off, lo


def box_correlation_estimate(pairs, rows, S, Q):
    """The uncentred correlation of the normalised residuals from pe_box_pair_stats' sums (host arithmetic):
    rho_ab = (S_ab / (4 N_ab)) / sqrt((Q_a / (4 M_a)) * (Q_b / (4 M_b))) - the zero-mean assumption of the variance fit, robust to a
    variance scale that was not fitted.  A pair without member pairs (or a detector without rows) gets 0 and is listed in "empty"; a
    diagonal entry below 0 (or not below 1) is set to 0 and listed in "clamped"; the off-diagonal entries are then shrunk by shrink_to_psd.
    Returns {"matrix", "raw", "shrink", "empty": [[a, b]], "clamped": [d], "stderr": [D][D] sqrt((1 + rho^2) / (4 N_ab)) (None
    without pairs)}."""
    pairs, S = np.asarray(pairs), np.asarray(S, dtype=np.float64)
    D = pairs.shape[0]
    raw, empty, clamped = np.zeros((D, D)), [], []
    stderr = [[None] * D for _ in range(D)]
    for a in range(D):
        for b in range(a, D):
            n = int(pairs[a, b])
            if n == 0 or rows[a] == 0 or rows[b] == 0 or not (Q[a] > 0 and Q[b] > 0):
                empty.append([a, b])
                continue
            raw[a, b] = raw[b, a] = (S[a, b] / (4 * n)) / math.sqrt((Q[a] / (4 * rows[a])) * (Q[b] / (4 * rows[b])))
            stderr[a][b] = stderr[b][a] = math.sqrt((1 + raw[a, b] ** 2) / (4 * n))
    fixed = raw.copy()
    for d in range(D):
        if not 0 <= fixed[d, d] < 1:          # (>= 1 can only come from a handful of pairs: no estimate either)
            fixed[d, d] = 0.0
            clamped.append(d)
    matrix, f = shrink_to_psd(fixed)
    return {"matrix": matrix.tolist(), "raw": raw.tolist(), "shrink": f, "empty": empty, "clamped": clamped, "stderr": stderr}


def fit_box_correlation(row_boxes, row_vars, row_source, member_rows, cluster_offsets, cluster_match, gt_boxes, num_detectors,
                        bbox_reg_weights=BBOX_REG_WEIGHTS):
    """The correlation of the detectors' normalised box errors over the clusters a "v-avg" fusion formed (late_fusion.fused_clusters:
    "row_boxes", "row_vars", "row_source", "member_rows", "cluster_offsets"), each cluster with the ground-truth box its fused box
    matched (cluster_match: match_rows_device's `match` on the clusters' fused boxes; -1: the cluster adds nothing).  One
    pe_box_pair_stats call, then box_correlation_estimate on the host.  Returns its dict plus {"pairs" [D][D], "rows" [D], "excluded"}."""
    st = box_pair_stats(row_boxes, row_vars, row_source, member_rows, cluster_offsets, cluster_match, gt_boxes, num_detectors,
                        bbox_reg_weights)
    out = box_correlation_estimate(st["pairs"], st["rows"], st["S"], st["Q"])
    out.update({"pairs": st["pairs"].tolist(), "rows": list(st["rows"]), "excluded": st["excluded"]})
    return out
