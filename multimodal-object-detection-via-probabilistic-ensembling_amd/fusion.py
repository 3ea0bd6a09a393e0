"""ProbEn late fusion on the GPU - host side.

Mirrors the reference's call surface (demo/FLIR/demo_probEn.py):
  fusion(method, info_1, info_2, info_3='')   :189-196  (one image, Python lists in)
and adds the batched form the MI355X path actually uses:
  fuse_batch(...)                             one launch, one 1024-thread workgroup per image.
The arithmetic lives in csrc/proben.hip behind pe_proben_fuse_batch.

score_fusion "probEn-log" (not in the reference) is ProbEn on the detectors' log-posteriors, log_softmax(class_logits / T) over all
K + 1 columns with the background column kept, normalised by a max-subtracted log-sum-exp (pe_proben_fuse_batch_logp): the same Bayes
rule, defined on saturated rows and large clusters where "probEn" gives NaN, with an optional class prior (`class_prior`).
`pool_weights` (one exponent w_d >= 0 per detector, "probEn-log" only) turns its product into the logarithmic opinion pool
a_j = sum_t w_d(t) log p_t[j] - (W - 1) log prior_j (pe_proben_fuse_batch_pooled); every weight 1 is "probEn-log" bit for bit.
`with_posterior` ("probEn-log" only, with or without pool weights) keeps what the fusion forms and the plain entry points drop: the
fused rows' normalised log-posterior over all K + 1 columns, the variance of the fused box under its box rule and the size of the
cluster (pe_proben_fuse_batch_posterior) - the fused detection as a full prediction, a valid "probEn-log" input itself.
`presence` ("probEn-log" only, with or without pool weights / with_posterior) adds one row of log-evidence per presence pattern - which
detectors put a row into the cluster - to the fused columns, last (pe_proben_fuse_batch_presence); clusters of one row and
passed-through images are fused too, since a silent detector is evidence as well.
box_fusion "c-avg" ("probEn-log" only, with `box_correlation`, one correlation of the normalised box errors per detector pair) is the
generalised-least-squares mean of a cluster's boxes under that correlation and the variance the mean really has: the fusion runs at
"v-avg" and a second launch (pe_box_gls_batch, csrc/boxcorr.hip) overwrites the boxes - and the variances, with_posterior - of the fused
rows whose cluster has two or more rows.  Scores, classes, clusters and rows of one never read the matrix; a zero matrix is "v-avg".
score_fusion "wbf" with box_fusion "wbf" (not in the reference, whose weighted_box_fusion is "s-avg") is weighted boxes fusion
(Solovyev, Wang, Gabruseva 2021), the baseline ProbEn is compared against: every row is matched against the running fused box of each
cluster of its class, a cluster's score is its mean weighted score times min(n, U) / U, and there is no passthrough case split.  A
kernel of its own (pe_wbf_fuse_batch, csrc/wbf.hip), with `wbf_weights` (one per detector) and `wbf_skip`; DESIGN.md section 29.
"""
import numpy as np
import torch

from . import _lib
from . import options as O
from .options import log_class_prior, pool_weight_tensor  # noqa: F401  (their callers know them by this module)

SCORE_MODES = {"probEn": 0, "avg": 1, "max": 2, "probEn_binary": 3, "probEn-log": 4}
LOGP = "probEn-log"
BOX_MODES = {"v-avg": 0, "s-avg": 1, "avg": 2, "argmax": 3}
CAVG = "c-avg"      # not a mode of the fusion kernel: "v-avg" there, then pe_box_gls_batch
WBF = "wbf"         # not a mode of the fusion kernel either: score_fusion and box_fusion together, pe_wbf_fuse_batch (csrc/wbf.hip)
WBF_IOU = 0.55      # the method's published IoU threshold
FRAME_W, FRAME_H = 640.0, 512.0  # class-band shift hard-coded by the reference (demo_probEn.py:100-103)


def _check_mode(score_fusion, class_prior, who, pool_weights=None, with_posterior=False, presence=None, box_fusion=None,
                box_correlation=None, variance_scales=None, wbf_weights=None, wbf_skip=None):
    if WBF in (score_fusion, box_fusion):
        if score_fusion != WBF:
            raise ValueError(f"{who}: box_fusion '{WBF}' belongs to score_fusion '{WBF}' (got {score_fusion!r}): weighted boxes fusion is "
                             "one method, its clusters and its scores come from one walk")
        if box_fusion != WBF:
            raise ValueError(f"{who}: score_fusion '{WBF}' belongs to box_fusion '{WBF}' (got {box_fusion!r}): weighted boxes fusion is "
                             "one method, its clusters and its scores come from one walk")
        owner = f"score_fusion '{LOGP}'"
        refused = [("class_prior belongs", class_prior, owner), ("pool_weights belong", pool_weights, owner),
                   ("presence belongs", presence, owner), ("with_posterior belongs", with_posterior or None, owner),
                   ("box_correlation belongs", box_correlation, f"box_fusion '{CAVG}'"),
                   ("variance_scales belong", variance_scales, f"box_fusion 'v-avg' and '{CAVG}'")]
        for what, value, owner in refused:
            if value is not None:
                raise ValueError(f"{who}: {what} to {owner} (got '{WBF}'): weighted boxes fusion reads no variance, probability or logit")
        return
    if wbf_weights is not None or wbf_skip is not None:
        raise ValueError(f"{who}: {'wbf_weights belong' if wbf_weights is not None else 'wbf_skip belongs'} to score_fusion '{WBF}' with "
                         f"box_fusion '{WBF}' (got {score_fusion!r}, {box_fusion!r})")
    if score_fusion not in SCORE_MODES:
        raise ValueError(f"{who}: unknown score_fusion {score_fusion!r} (one of {', '.join(SCORE_MODES)})")
    if box_fusion == CAVG and score_fusion != LOGP:
        raise ValueError(f"{who}: box_fusion '{CAVG}' belongs to score_fusion '{LOGP}' (got {score_fusion!r}): it finds a cluster's rows "
                         "through the cluster output only that fusion writes")
    if box_fusion == CAVG and box_correlation is None:
        raise ValueError(f"{who}: box_fusion '{CAVG}' needs a box_correlation (zeros give 'v-avg')")
    if box_correlation is not None and box_fusion != CAVG:
        raise ValueError(f"{who}: box_correlation belongs to box_fusion '{CAVG}' (got {box_fusion!r}): no other box rule reads it")
    if with_posterior and score_fusion != LOGP:
        raise ValueError(f"{who}: with_posterior belongs to score_fusion '{LOGP}' (got {score_fusion!r}): the other score fusions "
                         "form no normalised posterior")
    if presence is not None and score_fusion != LOGP:
        raise ValueError(f"{who}: presence belongs to score_fusion '{LOGP}' (got {score_fusion!r}): the other score fusions "
                         "have no log-evidence to add it to")
    if pool_weights is not None and score_fusion != LOGP:
        raise ValueError(f"{who}: pool_weights belong to score_fusion '{LOGP}' (got {score_fusion!r}): the other score fusions "
                         "have no pooled form")
    if class_prior is not None and score_fusion != LOGP:
        raise ValueError(f"{who}: class_prior belongs to score_fusion '{LOGP}' (got {score_fusion!r}): the other score fusions "
                         "have no prior term")


def fuse_batch(boxes, scores, probs, variances, classes, offsets, score_fusion="probEn", box_fusion="v-avg",
               max_rows=None, iou_thresh=None, frame=(FRAME_W, FRAME_H), row_counts=None, passthrough=None, log_probs=None,
               class_prior=None, pool_weights=None, row_source=None, with_posterior=False, presence=None, box_correlation=None,
               options=None, wbf_weights=None, wbf_skip=None, num_classes=None):
    """Fuse B images in one launch.

    boxes f64 [Ntot,4], scores f64 [Ntot], probs f64 [Ntot,K], variances f64 [Ntot],
    classes i32 [Ntot], offsets i32 [B+1] - all CUDA tensors, rows of each image already
    concatenated in detector order.  Returns a dict of device tensors:
      boxes f64 [Ntot,4], scores f32 [Ntot], classes f32 [Ntot], keep i32 [Ntot], counts i32 [B];
    image b's fused rows are [offsets[b], offsets[b]+counts[b]).

    The option keywords, or `options` (an options.FusionOptions, which documents them and the outputs they add; not both), select the
    entry point.  score_fusion "probEn-log": log_probs f64 [Ntot,K+1] (calibration.log_posteriors / pack_rows(log_posteriors=True))
    replaces probs (ignored, may be None).  pool_weights, presence and box_fusion "c-avg" need row_source i32 [Ntot], each row's
    detector index.  Temperatures and variance scales are in the rows already: they are not read here.

      entry point                      when                                  row_source, pool_weights, D   cluster  posterior  pattern
      pe_proben_fuse_batch             any other score_fusion                -                             -        -          -
      pe_proben_fuse_batch_logp        "probEn-log", nothing below           -                             -        -          -
      pe_proben_fuse_batch_pooled      pool_weights, or "c-avg" alone        given (c-avg alone: w = 1.0)  yes      -          -
      pe_proben_fuse_batch_posterior   with_posterior                        given, or NULL / NULL / 0     c-avg    yes        -
      pe_proben_fuse_batch_presence    presence                              row_source, weights or NULL   yes      or NULL    yes
    (first match from the bottom).  "c-avg" runs the chosen entry point at "v-avg" - the pooled one at weights of 1.0, which is
    "probEn-log" bit for bit, when nothing else selects one that writes "cluster" - and then pe_box_gls_batch.

    iou_thresh: None (the signature default) is 0.5, and 0.55 - the method's published threshold - for "wbf".

    score_fusion "wbf" with box_fusion "wbf" (weighted boxes fusion; wbf_weights one per detector - required here unless `options`
    knows the detector count -, wbf_skip): pe_wbf_fuse_batch.  It needs row_source and reads boxes, scores and classes only: probs
    (or num_classes, where probs is None) gives K, variances, log_probs and passthrough are ignored - an image on which one detector
    fired is fused like any other.  Returns boxes f64 [Ntot,4], scores f32, classes f32, counts i32 [B], cluster i32 [Ntot] (the
    image-local output row of the cluster each input row ended in; -1: the row was skipped; -2 where nothing was written), members i32
    [Ntot] (rows in the cluster, indexed like "scores") and skipped i32 [B] (rows skipped: a bad source or class, a non-finite
    coordinate, a score * weight that is not finite, not > 0 or below wbf_skip); no "keep"."""
    opts = O.FusionOptions.of(options, "fuse_batch", None, score_fusion, box_fusion, class_prior=class_prior, pool_weights=pool_weights,
                              with_posterior=with_posterior, presence=presence, box_correlation=box_correlation, wbf_weights=wbf_weights,
                              wbf_skip=wbf_skip)
    if opts.wbf:
        return _wbf_batch(opts, boxes, scores, probs, classes, offsets, max_rows, iou_thresh, row_counts, row_source, num_classes)
    iou_thresh = 0.5 if iou_thresh is None else iou_thresh
    logp, cavg, post = opts.logp, opts.cavg, opts.with_posterior
    pool, pres = opts.pool_weights is not None, opts.presence is not None
    ntot = boxes.shape[0]
    if opts.needs_row_source and (row_source is None or row_source.dim() != 1 or row_source.shape[0] != ntot):
        what = f"box_fusion '{CAVG}' needs" if cavg else "presence needs" if pres else "pool_weights need"
        raise ValueError(f"fuse_batch: {what} row_source [Ntot] for the {ntot} rows, got "
                         f"{None if row_source is None else tuple(row_source.shape)}")
    if logp:
        if log_probs is None or log_probs.dim() != 2 or log_probs.shape[1] < 2 or log_probs.shape[0] != ntot:
            raise ValueError(f"fuse_batch: score_fusion '{LOGP}' needs log_probs [Ntot, K+1] for the {ntot} rows, got "
                             f"{None if log_probs is None else tuple(log_probs.shape)}")
        probs = log_probs
    _lib.require_cuda(boxes, scores, probs, variances, classes, offsets, row_source if opts.needs_row_source else None)
    if opts.score_fusion == "max" and opts.box_fusion == "argmax":
        raise ValueError("('max','argmax') is the class-aware NMS route: use fusion()/nms_fuse_batch")
    B = offsets.numel() - (0 if row_counts is not None else 1)
    K = probs.shape[1] if probs is not None and probs.dim() == 2 else 1
    K -= 1 if logp else 0
    dev = boxes.device
    log_prior, weights, table, corr = opts.on(dev, K + 1) if logp else (None,) * 4
    boxes = boxes.contiguous().double()
    scores = scores.contiguous().double()
    probs = probs.contiguous().double() if probs is not None else None
    variances = variances.reshape(-1).contiguous().double()
    classes = classes.contiguous().to(torch.int32)
    offsets = offsets.contiguous().to(torch.int32)
    if max_rows is None:
        assert row_counts is None, "max_rows must be given with row_counts (avoids a host sync)"
        max_rows = int((offsets[1:] - offsets[:-1]).max().item()) if B > 0 else 1
    max_rows = max(int(max_rows), 1)
    if opts.needs_row_source:
        row_source = row_source.contiguous().to(torch.int32)
    if cavg and not (pool or pres or post):     # no entry point that writes "cluster" is selected: the pooled one at w = 1
        pool, weights = True, torch.ones((corr.shape[0],), dtype=torch.float64, device=dev)
    entry = "_presence" if pres else "_posterior" if post else "_pooled" if pool else "_logp" if logp else ""
    detectors = opts.num_detectors if pres else int(weights.numel()) if pool else 0

    def new(shape, dtype, fill):
        return torch.full(shape, fill, dtype=dtype, device=dev)
    out = {
        "boxes": torch.empty((ntot, 4), dtype=torch.float64, device=dev),
        "scores": torch.empty((ntot,), dtype=torch.float32, device=dev),
        "classes": torch.empty((ntot,), dtype=torch.float32, device=dev),
        "keep": torch.empty((ntot,), dtype=torch.int32, device=dev),
        "counts": torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)[:B],
    }
    # outputs only some entry points write, pre-filled with what "nothing was written here" reads as (padding, counts == -1)
    if pres or pool or cavg:
        out["cluster"] = new((ntot,), torch.int32, -2)
    if post:
        out["log_posterior"] = new((ntot, K + 1), torch.float64, float("nan"))
        out["vars"] = new((ntot,), torch.float64, float("nan"))
        out["members"] = torch.zeros((ntot,), dtype=torch.int32, device=dev)
    if pres:
        out["pattern"] = new((ntot,), torch.int32, -1)
    P = _lib.ptr
    name = "pe_proben_fuse_batch" + entry
    # every field of _lib.FUSE_FIELDS; the entry point takes those it has.  row_source / pool_weights NULL: the unpooled rule; the three
    # posterior outputs are NULL together on a score-only presence run
    values = {"boxes": P(boxes), "scores": P(scores), "probs": P(probs), "vars": P(variances), "classes": P(classes),
              "row_source": P(row_source) if pool or pres else None, "offsets": P(offsets), "row_counts": P(row_counts),
              "passthrough": P(passthrough), "B": B, "K": K, "max_rows": max_rows, "score_mode": SCORE_MODES[opts.score_fusion],
              "box_mode": BOX_MODES["v-avg" if cavg else opts.box_fusion], "thr": float(iou_thresh), "fw": float(frame[0]), "fh": float(frame[1]),
              "log_prior": P(log_prior), "pool_weights": P(weights) if pool else None, "presence": P(table), "num_detectors": detectors,
              "out_boxes": P(out["boxes"]), "out_scores": P(out["scores"]), "out_classes": P(out["classes"]), "out_keep": P(out["keep"]),
              "out_counts": P(out["counts"]), "out_cluster": P(out.get("cluster")), "out_log_posterior": P(out.get("log_posterior")),
              "out_vars": P(out.get("vars")), "out_members": P(out.get("members")), "out_pattern": P(out.get("pattern")),
              "stream": _lib.stream()}
    _lib.check(getattr(_lib.lib(), name)(*[values[f] for f in _lib.FUSE_ORDER[name]]), name)
    if cavg:
        st = _lib.lib().pe_box_gls_batch(P(boxes), P(variances), P(row_source), P(out["cluster"]), P(offsets), P(row_counts),
                                         P(out["counts"]), B, max_rows, P(corr), int(corr.shape[0]), P(out["boxes"]), P(out.get("vars")),
                                         _lib.stream())
        _lib.check(st, "pe_box_gls_batch")
    return out


def _wbf_batch(opts, boxes, scores, probs, classes, offsets, max_rows, iou_thresh, row_counts, row_source, num_classes):
    """fuse_batch for score_fusion / box_fusion "wbf": one pe_wbf_fuse_batch launch, no host synchronisation when max_rows is given."""
    ntot = boxes.shape[0]
    if row_source is None or row_source.dim() != 1 or row_source.shape[0] != ntot:
        raise ValueError(f"fuse_batch: '{WBF}' needs row_source [Ntot] for the {ntot} rows, got "
                         f"{None if row_source is None else tuple(row_source.shape)}")
    if opts.wbf_weights is None:
        raise ValueError(f"fuse_batch: '{WBF}' needs wbf_weights, one per detector (1.0 each is the unweighted method)")
    if num_classes is None:
        if probs is None or probs.dim() != 2:
            raise ValueError(f"fuse_batch: '{WBF}' needs probs [Ntot, K] or num_classes for the class count")
        num_classes = probs.shape[1]
    _lib.require_cuda(boxes, scores, classes, offsets, row_source, row_counts)
    dev = boxes.device
    B = offsets.numel() - (0 if row_counts is not None else 1)
    boxes = boxes.contiguous().double()
    scores = scores.contiguous().double()
    classes = classes.contiguous().to(torch.int32)
    offsets = offsets.contiguous().to(torch.int32)
    row_source = row_source.contiguous().to(torch.int32)
    if max_rows is None:
        assert row_counts is None, "max_rows must be given with row_counts (avoids a host sync)"
        max_rows = int((offsets[1:] - offsets[:-1]).max().item()) if B > 0 else 1
    max_rows = max(int(max_rows), 1)
    weights = opts.wbf_on(dev)
    out = {
        "boxes": torch.empty((ntot, 4), dtype=torch.float64, device=dev),
        "scores": torch.empty((ntot,), dtype=torch.float32, device=dev),
        "classes": torch.empty((ntot,), dtype=torch.float32, device=dev),
        "counts": torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)[:B],
        "cluster": torch.full((ntot,), -2, dtype=torch.int32, device=dev),
        "members": torch.zeros((ntot,), dtype=torch.int32, device=dev),
        "skipped": torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)[:B],
    }
    P = _lib.ptr
    st = _lib.lib().pe_wbf_fuse_batch(P(boxes), P(scores), P(classes), P(row_source), P(offsets), P(row_counts), B, int(num_classes),
                                      max_rows, P(weights), int(weights.numel()), float(WBF_IOU if iou_thresh is None else iou_thresh),
                                      float(opts.wbf_skip), P(out["boxes"]), P(out["scores"]), P(out["classes"]), P(out["counts"]),
                                      P(out["cluster"]), P(out["members"]), P(out["skipped"]), _lib.stream())
    _lib.check(st, "pe_wbf_fuse_batch")
    return out


def pack_infos(per_image_infos, device="cuda", with_log_probs=False, with_sources=False):
    """per_image_infos: list (images) of lists (detectors) of reference-style dicts
    {bbox, score, class, prob, vars}.  Returns the flat device tensors + offsets (with_log_probs: + the rows' "log_prob"
    [n][K+1] as a seventh tensor; with_sources: + each row's position in its image's detector list, i32, as the last)."""
    bb, ss, cc, pp, vv, offs = [], [], [], [], [], [0]
    ll, src = [], []
    K = None
    for infos in per_image_infos:
        for d in infos:
            if d and len(d["prob"]) > 0:
                K = len(d["prob"][0])
                break
        if K:
            break
    K = K or 3
    for infos in per_image_infos:
        n = 0
        for k, d in enumerate(infos):
            if not d or len(d["bbox"]) == 0:
                continue
            bb.append(np.asarray(d["bbox"], dtype=np.float64).reshape(-1, 4))
            ss.append(np.asarray(d["score"], dtype=np.float64).reshape(-1))
            cc.append(np.asarray(d["class"], dtype=np.int32).reshape(-1))
            pp.append(np.asarray(d["prob"], dtype=np.float64).reshape(-1, K))
            vv.append(np.asarray(d["vars"], dtype=np.float64).reshape(-1))
            if with_log_probs:
                ll.append(np.asarray(d["log_prob"], dtype=np.float64).reshape(-1, K + 1))
            src.append(np.full(len(ss[-1]), k, dtype=np.int32))
            n += len(ss[-1])
        offs.append(offs[-1] + n)

    def cat(xs, shape, dt):
        return torch.from_numpy(np.concatenate(xs) if xs else np.zeros(shape, dtype=dt)).to(device)

    out = (cat(bb, (0, 4), np.float64), cat(ss, (0,), np.float64), cat(pp, (0, K), np.float64),
           cat(vv, (0,), np.float64), cat(cc, (0,), np.int32),
           torch.tensor(offs, dtype=torch.int32, device=device))
    out = out + (cat(ll, (0, K + 1), np.float64),) if with_log_probs else out
    return out + (cat(src, (0,), np.int32),) if with_sources else out


def fusion(method, info_1, info_2, info_3="", temperatures=None, class_prior=None, variance_scales=None, pool_weights=None,
           box_correlation=None, options=None):
    """Drop-in for the reference's ``fusion`` (demo_probEn.py:189-196).

    Returns (out_boxes, out_scores, out_class): boxes as a list of float64 ndarrays [4]
    (or a float32 Tensor [n,4] on the ('max','argmax') route), scores / classes as float32
    CPU tensors - the reference's return types.
    The option keywords, or `options` (options.FusionOptions, which documents them; not both), one value per info: the rows' prob /
    score are rebuilt from their class_logits as softmax(logits / T) (calibration.calibrate_rows; an info without logits is refused),
    their vars multiplied by s in float64, and a row's detector is its info's position.
    method ("wbf", "wbf"): weighted boxes fusion at weights of 1.0 and the IoU threshold 0.55 (other weights: `options`)."""
    infos = [info_1, info_2] + ([info_3] if info_3 else [])
    opts = O.FusionOptions.of(options, "fusion", len(infos), method[0], method[1], temperatures=temperatures, class_prior=class_prior,
                              variance_scales=variance_scales, pool_weights=pool_weights, box_correlation=box_correlation)
    if opts.variance_scales is not None:
        infos = [dict(d, vars=(np.asarray(d["vars"], dtype=np.float64) * s).tolist()) for d, s in zip(infos, opts.variance_scales)]
    logp = opts.logp
    if opts.temperatures is not None:
        from . import calibration
        cal = []
        for k, (d, T) in enumerate(zip(infos, opts.temperatures)):
            lg = d.get("class_logits")
            if lg is None or len(lg) != len(d["bbox"]) or any(len(r) < 2 for r in lg):
                raise ValueError(f"fusion: info_{k + 1} ({d.get('img_name', '?')}) carries no class_logits: temperature calibration "
                                 "needs the detector's logits")
            p, s = calibration.calibrate_rows(lg, d["class"], calibration.check_temperature(T, f"temperature of info_{k + 1}"))
            cal.append(dict(d, prob=p, score=s))
            if logp:
                cal[-1]["log_prob"] = calibration.log_posterior_rows(lg, calibration.check_temperature(T, f"temperature of info_{k + 1}"))
        infos = cal
    if method[0] == "max" and method[1] == "argmax":
        from .layers import batched_nms
        boxes = torch.tensor(sum([list(d["bbox"]) for d in infos], []), dtype=torch.float32).reshape(-1, 4)
        scores = torch.tensor(sum([list(d["score"]) for d in infos], []), dtype=torch.float32)
        classes = torch.tensor(sum([list(d["class"]) for d in infos], []), dtype=torch.float32)
        keep = batched_nms(boxes.cuda(), scores.cuda(), classes.cuda(), 0.5).cpu()
        return boxes[keep], scores[keep], classes[keep]
    b, s, p, v, c, offs, *rest = pack_infos([infos], with_log_probs=logp, with_sources=opts.needs_row_source)
    out = fuse_batch(b, s, p, v, c, offs, log_probs=rest[0] if logp else None, row_source=rest[-1] if opts.needs_row_source else None,
                     options=opts)
    m = int(out["counts"][0].item())
    if m < 0:
        raise RuntimeError("fusion: too many rows for one image")
    boxes = out["boxes"][:m].cpu().numpy()
    return [boxes[i] for i in range(m)], out["scores"][:m].cpu(), out["classes"][:m].cpu()


def pack_rows(dets, max_class=2, temperatures=None, log_posteriors=False, variance_scales=None, pool_weights=None, with_sources=False,
              options=None):
    """The detectors' padded outputs -> ProbEn input rows on the device (pe_proben_pack_detections; with temperatures
    pe_proben_pack_logits: probabilities and scores from class_logits as softmax(logits / T_d) in float64).
    Returns (boxes f64 [B*S,4], scores f64, probs f64 [B*S,K], vars f64, classes i32, offsets i32 [B], counts i32 [B],
    single-source flags i32 [B]), S = len(dets) * D.  log_posteriors (needs temperatures): pe_proben_pack_log_posteriors, the
    same eight plus the rows' log-posteriors f64 [B*S,K+1] as a ninth.
    variance_scales (one s per detector): pe_proben_pack_calibrated, whichever of the three routes the other arguments select, with
    vars = (double)var * s_d; None calls the three entry points above as before.
    with_sources (or pool_weights, one w per detector, of which only the presence and the count matter here): pe_proben_pack_pooled,
    the same route with each written row's detector index i32 [B*S] appended as the LAST element of the result.
    options (an options.FusionOptions, instead of the keywords): its temperatures and variance scales, log-posteriors on
    "probEn-log", sources where its fusion needs row_source."""
    import ctypes
    nd = len(dets)
    if options is not None:
        temperatures, variance_scales = options.temperatures, options.variance_scales
        log_posteriors, with_sources = options.logp, options.needs_row_source
    else:
        temperatures = O.checked("temperatures", temperatures, nd, "fuse_detections")   # (the caller these messages have always named)
        variance_scales = O.checked("variance_scales", variance_scales, nd, "pack_rows")
        with_sources = with_sources or O.checked("pool_weights", pool_weights, nd, "pack_rows") is not None
    B, D = dets[0]["scores"].shape
    K = dets[0]["prob_score"].shape[2]
    dev = dets[0]["scores"].device
    S = nd * D

    def arr(key):
        return (ctypes.c_void_p * nd)(*[d[key].data_ptr() for d in dets])
    ob = torch.empty((B * S, 4), dtype=torch.float64, device=dev)
    os_ = torch.empty((B * S,), dtype=torch.float64, device=dev)
    op = torch.empty((B * S, K), dtype=torch.float64, device=dev)
    ov = torch.empty((B * S,), dtype=torch.float64, device=dev)
    oc = torch.empty((B * S,), dtype=torch.int32, device=dev)
    ooff = torch.empty((B,), dtype=torch.int32, device=dev)
    ocnt = torch.empty((B,), dtype=torch.int32, device=dev)
    osingle = torch.empty((B,), dtype=torch.int32, device=dev)
    if log_posteriors and temperatures is None:
        raise ValueError("pack_rows: log_posteriors needs temperatures (1.0 per detector for the uncalibrated logits)")
    if temperatures is not None:
        for d in dets:
            if d["class_logits"].shape != (B, D, K + 1) or d["class_logits"].dtype != torch.float32:
                raise ValueError(f"fuse_detections: class_logits {tuple(d['class_logits'].shape)} is not float32 [{B}, {D}, {K + 1}]")
    logits = temperatures is not None
    olp = torch.empty((B * S, K + 1), dtype=torch.float64, device=dev) if log_posteriors else None
    temps = (ctypes.c_double * nd)(*[float(t) for t in temperatures]) if logits else None
    scores, probs, lg = (None, None, arr("class_logits")) if logits else (arr("scores"), arr("prob_score"), None)
    dims = (nd, B, D, K, max_class, S)
    head, tail = [_lib.ptr(t) for t in (ob, os_, op)], [_lib.ptr(t) for t in (ov, oc, ooff, ocnt, osingle)]
    osrc = torch.empty((B * S,), dtype=torch.int32, device=dev) if with_sources else None
    if variance_scales is not None or osrc is not None:
        name = "pe_proben_pack_pooled" if osrc is not None else "pe_proben_pack_calibrated"
        args = (arr("boxes"), scores, arr("classes"), probs, lg, arr("vars"), arr("counts"), temps,
                (ctypes.c_double * nd)(*variance_scales) if variance_scales is not None else None, *dims, *head, _lib.ptr(olp), *tail,
                *([_lib.ptr(osrc)] if osrc is not None else []))
    elif not logits:
        name = "pe_proben_pack_detections"
        args = (arr("boxes"), scores, arr("classes"), probs, arr("vars"), arr("counts"), *dims, *head, *tail)
    else:
        name = "pe_proben_pack_log_posteriors" if log_posteriors else "pe_proben_pack_logits"
        args = (arr("boxes"), arr("classes"), lg, arr("vars"), arr("counts"), temps, *dims, *head,
                *([_lib.ptr(olp)] if log_posteriors else []), *tail)
    st = getattr(_lib.lib(), name)(*args, _lib.stream())
    _lib.check(st, name)
    return (ob, os_, op, ov, oc, ooff, ocnt, osingle) + ((olp,) if log_posteriors else ()) + ((osrc,) if osrc is not None else ())


def fuse_detections(dets, score_fusion="probEn", box_fusion="v-avg", max_class=2, iou_thresh=None, temperatures=None,
                    class_prior=None, variance_scales=None, pool_weights=None, with_posterior=False, presence=None,
                    box_correlation=None, options=None):
    """Device-to-device stage fusion: `dets` = the result dicts of 2 or 3 detectors run on the SAME batch
    (rcnn.GeneralizedRCNN.forward_batch).  Packs their detections into ProbEn rows (classes <= max_class,
    like the JSON writer demo_FLIR_save_predictions.py:148-155), applies the reference's per-image case
    split (0 detectors -> nothing, 1 -> passthrough, >= 2 -> fusion; demo_probEn.py:237-267) and fuses.
    The option keywords, or `options` (options.FusionOptions, which documents them and the outputs they add; not both), one value per
    detector: with temperatures the rows come from the detectors' class_logits (pe_proben_pack_logits, pe_proben_pack_log_posteriors
    on "probEn-log") instead of the float32 prob_score / scores, with variance_scales through pe_proben_pack_calibrated; where the
    fusion needs each row's detector (pool_weights, presence, box_fusion "c-avg") pe_proben_pack_pooled writes it and the result
    also holds it as "row_source".  With presence, images on which one detector fired are rescored row by row, not copied.
    iou_thresh: None is 0.5, and 0.55 for "wbf" (fuse_batch).  "wbf" has no case split: an image on which one detector fired is fused
    like any other (the single-source flag is not read), and the result holds "cluster", "members" and "skipped" instead of "keep".
    No host synchronisation.  Returns a dict: boxes f64 [B*S,4], scores f32, classes f32, counts i32 [B],
    offsets i32 [B], stride S = len(dets) * D."""
    opts = O.FusionOptions.of(options, "fuse_detections", len(dets), score_fusion, box_fusion, temperatures=temperatures,
                              class_prior=class_prior, variance_scales=variance_scales, pool_weights=pool_weights,
                              with_posterior=with_posterior, presence=presence, box_correlation=box_correlation)
    # the box heads' candidate-cap bookkeeping travels with the result (no kernel here): check_candidate_overflow() looks
    # at it at the consumer's first host synchronisation
    overflow_src = [(d["cand_total"], d["cand_max"]) for d in dets if "cand_total" in d]
    B, D = dets[0]["scores"].shape
    S = len(dets) * D
    dev = dets[0]["scores"].device
    ob, os_, op, ov, oc, ooff, ocnt, osingle, *olp = pack_rows(dets, max_class, options=opts)
    osrc = olp.pop() if opts.needs_row_source else None
    if opts.score_fusion == "max" and opts.box_fusion == "argmax":
        from .layers import nms_batched_raw
        b32 = ob.float().view(B, S, 4)
        keep, kcnt = nms_batched_raw(b32, os_.float().view(B, S), oc.view(B, S), ocnt, None, 0.5 if iou_thresh is None else iou_thresh, 0, S)
        # images where only ONE detector fired are passed through untouched by the reference (demo_probEn.py:239-254)
        single = osingle.bool()
        keep = torch.where(single[:, None], torch.arange(S, dtype=torch.int32, device=dev).expand(B, S), keep)
        kcnt = torch.where(single, ocnt, kcnt)
        # same contract as the ProbEn route: image b's fused rows are [offsets[b], offsets[b] + counts[b]) of the flat
        # arrays (score-descending), so late_fusion.fused_rows_device / comm.all_gather_fused_rows need no special case
        g = (torch.arange(B, device=dev).view(B, 1) * S + keep.clamp(0, S - 1).long()).view(-1)
        return {"boxes": ob[g], "scores": os_.float()[g], "classes": oc.float()[g], "counts": kcnt, "keep": keep,
                "offsets": ooff, "stride": S, "in_counts": ocnt, "nms_route": True, "cand_overflow_src": overflow_src}
    out = fuse_batch(ob, os_, op, ov, oc, ooff, max_rows=S, iou_thresh=iou_thresh, row_counts=ocnt, passthrough=osingle,
                     log_probs=olp[0] if opts.logp else None, row_source=osrc, options=opts)
    if osrc is not None:
        out["row_source"] = osrc
    out["offsets"], out["stride"], out["in_counts"] = ooff, S, ocnt
    out["cand_overflow_src"] = overflow_src
    return out


def check_candidate_overflow(result):
    """Raise if a box head met more (proposal, class) candidates above SCORE_THRESH_TEST than its NMS stage holds
    (rcnn._roi_heads: cand_total > cand_max) - the device-to-device routes (forward_batch -> FramePairPipeline ->
    fuse_detections) would otherwise lose those detections silently, in proposal order, where the reference keeps all.
    `result`: a forward_batch dict or a fuse_detections dict.  Synchronises with the DEVICE (not just the current stream: the
    counters are written on the detectors' side streams of FramePairPipeline, which the caller's stream need not have waited for):
    call it where the consumer reads results anyway (GeneralizedRCNN.to_instances does the same check for the Instances route)."""
    src = result.get("cand_overflow_src")
    if src is None and "cand_total" in result:
        src = [(result["cand_total"], result["cand_max"])]
    if src and any(t.is_cuda for t, _ in src):
        torch.cuda.synchronize(src[0][0].device)
    for tot, cmax in src or []:
        worst = int(tot.max())
        if worst > cmax:
            raise RuntimeError(f"box head: {worst} (proposal, class) candidates pass the score threshold on one image but the "
                               f"NMS stage holds {cmax}: detections would be dropped in proposal order (the reference keeps all). "
                               "Raise SCORE_THRESH_TEST or lower POST_NMS_TOPK_TEST.")
