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
"""
import numpy as np
import torch

from . import _lib

SCORE_MODES = {"probEn": 0, "avg": 1, "max": 2, "probEn_binary": 3, "probEn-log": 4}
LOGP = "probEn-log"
BOX_MODES = {"v-avg": 0, "s-avg": 1, "avg": 2, "argmax": 3}
CAVG = "c-avg"      # not a mode of the fusion kernel: "v-avg" there, then pe_box_gls_batch
FRAME_W, FRAME_H = 640.0, 512.0  # class-band shift hard-coded by the reference (demo_probEn.py:100-103)


def log_class_prior(class_prior, num_columns, device):
    """class_prior (K + 1 probabilities, background last; calibration.check_class_prior validates and normalises) -> the DEVICE
    f64 [K + 1] log-prior pe_proben_fuse_batch_logp takes.  None -> None (uniform).  A CUDA tensor is taken as the result of an
    earlier call (FramePairPipeline uploads once, not per batch)."""
    if class_prior is None:
        return None
    if isinstance(class_prior, torch.Tensor) and class_prior.is_cuda:
        if class_prior.dtype != torch.float64 or tuple(class_prior.shape) != (num_columns,):
            raise ValueError(f"log-prior tensor {tuple(class_prior.shape)} {class_prior.dtype} is not float64 [{num_columns}]")
        return class_prior.contiguous()
    from .calibration import check_class_prior
    return torch.from_numpy(np.log(check_class_prior(class_prior, num_columns))).to(device)


def pool_weight_tensor(pool_weights, num_detectors, device):
    """pool_weights (one exponent per detector; calibration.check_pool_weights validates: finite, >= 0, not all 0) -> the DEVICE f64
    [num_detectors] tensor pe_proben_fuse_batch_pooled takes.  None -> None.  A CUDA tensor is taken as the result of an earlier call
    (FramePairPipeline uploads once, not per batch)."""
    if pool_weights is None:
        return None
    if isinstance(pool_weights, torch.Tensor) and pool_weights.is_cuda:
        if pool_weights.dtype != torch.float64 or tuple(pool_weights.shape) != (num_detectors,):
            raise ValueError(f"pool-weight tensor {tuple(pool_weights.shape)} {pool_weights.dtype} is not float64 [{num_detectors}]")
        return pool_weights.contiguous()
    from .calibration import check_pool_weights
    return torch.tensor(check_pool_weights(pool_weights, num_detectors, "pool_weights"), dtype=torch.float64).to(device)


def _check_mode(score_fusion, class_prior, who, pool_weights=None, with_posterior=False, presence=None, box_fusion=None,
                box_correlation=None):
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
               max_rows=None, iou_thresh=0.5, frame=(FRAME_W, FRAME_H), row_counts=None, passthrough=None, log_probs=None,
               class_prior=None, pool_weights=None, row_source=None, with_posterior=False, presence=None, box_correlation=None):
    """Fuse B images in one launch.

    score_fusion "probEn-log": log_probs f64 [Ntot,K+1] (calibration.log_posteriors / pack_rows(log_posteriors=True)) replaces
    probs (ignored, may be None); class_prior: K + 1 probabilities, background last, or None = uniform.
    pool_weights ("probEn-log" only; one w_d per detector or pool_weight_tensor's device tensor) with row_source i32 [Ntot] (each
    row's detector index): pe_proben_fuse_batch_pooled; the result then also holds "cluster" i32 [Ntot], the output row of the
    cluster each input row ended in (-1: it left the pool without one; -2 where nothing was written: counts == -1, padding).
    with_posterior ("probEn-log" only): pe_proben_fuse_batch_posterior; the result then also holds "log_posterior" f64 [Ntot, K+1]
    (the fused rows' normalised log-posterior), "vars" f64 [Ntot] (the fused boxes' variance under the box rule) and "members" i32
    [Ntot] (rows in the cluster), indexed like "scores"; rows nothing was written to hold NaN / NaN / 0.
    presence ("probEn-log" only; a table [2^D][K+1] or calibration.presence_table's device tensor) with row_source:
    pe_proben_fuse_batch_presence, with or without pool_weights / with_posterior; the fused columns gain presence[P][j], P the OR of
    (1 << source) over the cluster's rows, clusters of one row and passthrough images are fused too; the result then also holds
    "pattern" i32 [Ntot] (the fused rows' P, indexed like "scores"; -1 where nothing was written) and "cluster".
    box_fusion "c-avg" ("probEn-log" only) with box_correlation (a matrix [D][D], calibration.check_box_correlation, or
    calibration.box_correlation_tensor's device tensor) and row_source: the entry point the other arguments select runs at "v-avg"
    (pe_proben_fuse_batch_pooled with weights of 1.0, which is "probEn-log" bit for bit, when they select none that writes "cluster"),
    then pe_box_gls_batch overwrites "boxes" - and "vars", with_posterior - of the fused rows whose cluster has two or more rows; a row
    whose source is outside [0, D) makes its cluster's box and variance NaN.  The result then also holds "cluster".

    boxes f64 [Ntot,4], scores f64 [Ntot], probs f64 [Ntot,K], variances f64 [Ntot],
    classes i32 [Ntot], offsets i32 [B+1] - all CUDA tensors, rows of each image already
    concatenated in detector order.  Returns a dict of device tensors:
      boxes f64 [Ntot,4], scores f32 [Ntot], classes f32 [Ntot], keep i32 [Ntot], counts i32 [B];
    image b's fused rows are [offsets[b], offsets[b]+counts[b]).
    """
    _check_mode(score_fusion, class_prior, "fuse_batch", pool_weights, with_posterior, presence, box_fusion, box_correlation)
    logp = score_fusion == LOGP
    pool = pool_weights is not None
    pres = presence is not None
    cavg = box_fusion == CAVG
    if cavg and (row_source is None or row_source.dim() != 1 or row_source.shape[0] != boxes.shape[0]):
        raise ValueError(f"fuse_batch: box_fusion '{CAVG}' needs row_source [Ntot] for the {boxes.shape[0]} rows, got "
                         f"{None if row_source is None else tuple(row_source.shape)}")
    if pres and (row_source is None or row_source.dim() != 1 or row_source.shape[0] != boxes.shape[0]):
        raise ValueError(f"fuse_batch: presence needs row_source [Ntot] for the {boxes.shape[0]} rows, got "
                         f"{None if row_source is None else tuple(row_source.shape)}")
    if pool and (row_source is None or row_source.dim() != 1 or row_source.shape[0] != boxes.shape[0]):
        raise ValueError(f"fuse_batch: pool_weights need row_source [Ntot] for the {boxes.shape[0]} rows, got "
                         f"{None if row_source is None else tuple(row_source.shape)}")
    if logp:
        if log_probs is None or log_probs.dim() != 2 or log_probs.shape[1] < 2 or log_probs.shape[0] != boxes.shape[0]:
            raise ValueError(f"fuse_batch: score_fusion '{LOGP}' needs log_probs [Ntot, K+1] for the {boxes.shape[0]} rows, got "
                             f"{None if log_probs is None else tuple(log_probs.shape)}")
        probs = log_probs
    _lib.require_cuda(boxes, scores, probs, variances, classes, offsets, row_source if pool or pres or cavg else None)
    if score_fusion == "max" and box_fusion == "argmax":
        raise ValueError("('max','argmax') is the class-aware NMS route: use fusion()/nms_fuse_batch")
    B = offsets.numel() - (0 if row_counts is not None else 1)
    ntot = boxes.shape[0]
    K = probs.shape[1] if probs is not None and probs.dim() == 2 else 1
    K -= 1 if logp else 0
    log_prior = log_class_prior(class_prior, K + 1, boxes.device) if logp else None
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
    dev = boxes.device
    if pool:
        weights = pool_weight_tensor(pool_weights, len(pool_weights), dev)
    if pool or pres or cavg:
        row_source = row_source.contiguous().to(torch.int32)
    if cavg:
        from .calibration import box_correlation_tensor
        corr = box_correlation_tensor(box_correlation, None, dev)
        if pool and int(weights.numel()) != corr.shape[0]:
            raise ValueError(f"fuse_batch: {int(weights.numel())} pool weights beside a box correlation over {corr.shape[0]} detectors")
        if not (pool or pres or with_posterior):      # no entry point that writes "cluster" is selected: the pooled one at w = 1
            pool, weights = True, torch.ones((corr.shape[0],), dtype=torch.float64, device=dev)
    if pres:
        from .calibration import presence_detectors, presence_table
        table = presence_table(presence, None, K + 1, dev)
        nd = presence_detectors(table)
        if pool and int(weights.numel()) != nd:
            raise ValueError(f"fuse_batch: {int(weights.numel())} pool weights beside a presence table over {nd} detectors")
        if cavg and corr.shape[0] != nd:
            raise ValueError(f"fuse_batch: a box correlation over {corr.shape[0]} detectors beside a presence table over {nd}")
    out = {
        "boxes": torch.empty((ntot, 4), dtype=torch.float64, device=dev),
        "scores": torch.empty((ntot,), dtype=torch.float32, device=dev),
        "classes": torch.empty((ntot,), dtype=torch.float32, device=dev),
        "keep": torch.empty((ntot,), dtype=torch.int32, device=dev),
        "counts": torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)[:B],
    }
    name = ("pe_proben_fuse_batch_presence" if pres else "pe_proben_fuse_batch_posterior" if with_posterior else "pe_proben_fuse_batch_pooled" if pool
            else "pe_proben_fuse_batch_logp" if logp else "pe_proben_fuse_batch")
    head = (_lib.ptr(boxes), _lib.ptr(scores), _lib.ptr(probs), _lib.ptr(variances), _lib.ptr(classes),
            *([_lib.ptr(row_source) if pool or pres else None] if pool or with_posterior or pres else []), _lib.ptr(offsets), _lib.ptr(row_counts), _lib.ptr(passthrough), B, K, max_rows)
    geometry = (BOX_MODES["v-avg" if cavg else box_fusion], float(iou_thresh), float(frame[0]), float(frame[1]))
    mode = geometry + (_lib.ptr(log_prior),) if logp else (SCORE_MODES[score_fusion],) + geometry
    tail = ()
    if pres:
        mode += (_lib.ptr(weights) if pool else None, _lib.ptr(table), nd)
        out["cluster"] = torch.full((ntot,), -2, dtype=torch.int32, device=dev)
        tail = (_lib.ptr(out["cluster"]),)
    elif pool:
        mode += (_lib.ptr(weights), int(weights.numel()))
        out["cluster"] = torch.full((ntot,), -2, dtype=torch.int32, device=dev)     # -2: never written (padding, counts == -1)
        tail = (_lib.ptr(out["cluster"]),)
    elif with_posterior:
        mode += (None, 0)          # row_source and pool_weights NULL together: the unpooled rule
        if cavg:
            out["cluster"] = torch.full((ntot,), -2, dtype=torch.int32, device=dev)
        tail = (_lib.ptr(out.get("cluster")),)
    if with_posterior:
        out["log_posterior"] = torch.full((ntot, K + 1), float("nan"), dtype=torch.float64, device=dev)
        out["vars"] = torch.full((ntot,), float("nan"), dtype=torch.float64, device=dev)
        out["members"] = torch.zeros((ntot,), dtype=torch.int32, device=dev)
        tail += (_lib.ptr(out["log_posterior"]), _lib.ptr(out["vars"]), _lib.ptr(out["members"]))
    elif pres:
        tail += (None, None, None)         # the three posterior outputs NULL together: a score-only run
    if pres:
        out["pattern"] = torch.full((ntot,), -1, dtype=torch.int32, device=dev)     # -1: never written (padding, counts == -1)
        tail += (_lib.ptr(out["pattern"]),)
    st = getattr(_lib.lib(), name)(*head, *mode, _lib.ptr(out["boxes"]), _lib.ptr(out["scores"]), _lib.ptr(out["classes"]),
                                   _lib.ptr(out["keep"]), _lib.ptr(out["counts"]), *tail, _lib.stream())
    _lib.check(st, name)
    if cavg:
        st = _lib.lib().pe_box_gls_batch(_lib.ptr(boxes), _lib.ptr(variances), _lib.ptr(row_source), _lib.ptr(out["cluster"]),
                                         _lib.ptr(offsets), _lib.ptr(row_counts), _lib.ptr(out["counts"]), B, max_rows, _lib.ptr(corr),
                                         int(corr.shape[0]), _lib.ptr(out["boxes"]), _lib.ptr(out.get("vars")), _lib.stream())
        _lib.check(st, "pe_box_gls_batch")
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
           box_correlation=None):
    """Drop-in for the reference's ``fusion`` (demo_probEn.py:189-196).

    Returns (out_boxes, out_scores, out_class): boxes as a list of float64 ndarrays [4]
    (or a float32 Tensor [n,4] on the ('max','argmax') route), scores / classes as float32
    CPU tensors - the reference's return types.
    temperatures (one T per info): the rows' prob / score are rebuilt from their class_logits as softmax(logits / T)
    (calibration.calibrate_rows); an info without logits is refused.
    method[0] "probEn-log": the rows' log-posteriors come from their class_logits too (temperatures None = 1 for every info) and
    are fused by pe_proben_fuse_batch_logp, with class_prior (K + 1 probabilities, background last) when given.
    variance_scales (one s per info): the rows' vars are multiplied by s in float64 (one multiply, as pe_proben_pack_calibrated does
    on the device route); the box rules "v-avg" and "c-avg" read them.
    pool_weights (one w per info, method[0] "probEn-log" only): the pooled rule of pe_proben_fuse_batch_pooled; a row's detector is
    its info's position.
    method[1] "c-avg" (method[0] "probEn-log" only) with box_correlation (one entry per pair of infos): fuse_batch's correlated box rule."""
    infos = [info_1, info_2] + ([info_3] if info_3 else [])
    _check_mode(method[0], class_prior, "fusion", pool_weights, box_fusion=method[1], box_correlation=box_correlation)
    if box_correlation is not None:
        from .calibration import check_box_correlation
        box_correlation = check_box_correlation(box_correlation, len(infos), "fusion: box_correlation")
    if pool_weights is not None:
        from .calibration import check_pool_weights
        pool_weights = check_pool_weights(pool_weights, len(infos), "fusion")
    if variance_scales is not None:
        from .calibration import check_variance_scales
        variance_scales = check_variance_scales(variance_scales, len(infos), "fusion")
        infos = [dict(d, vars=(np.asarray(d["vars"], dtype=np.float64) * s).tolist()) for d, s in zip(infos, variance_scales)]
    logp = method[0] == LOGP
    if logp and temperatures is None:
        temperatures = [1.0] * len(infos)
    if temperatures is not None:
        from . import calibration
        if len(temperatures) != len(infos):
            raise ValueError(f"fusion: {len(temperatures)} temperatures for {len(infos)} detectors")
        cal = []
        for k, (d, T) in enumerate(zip(infos, temperatures)):
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
    if logp and (pool_weights is not None or box_correlation is not None):
        b, s, p, v, c, offs, lp, src = pack_infos([infos], with_log_probs=True, with_sources=True)
        out = fuse_batch(b, s, p, v, c, offs, method[0], method[1], log_probs=lp, class_prior=class_prior, pool_weights=pool_weights,
                         row_source=src, box_correlation=box_correlation)
    elif logp:
        b, s, p, v, c, offs, lp = pack_infos([infos], with_log_probs=True)
        out = fuse_batch(b, s, p, v, c, offs, method[0], method[1], log_probs=lp, class_prior=class_prior)
    else:
        b, s, p, v, c, offs = pack_infos([infos])
        out = fuse_batch(b, s, p, v, c, offs, method[0], method[1])
    m = int(out["counts"][0].item())
    if m < 0:
        raise RuntimeError("fusion: too many rows for one image")
    boxes = out["boxes"][:m].cpu().numpy()
    return [boxes[i] for i in range(m)], out["scores"][:m].cpu(), out["classes"][:m].cpu()


def pack_rows(dets, max_class=2, temperatures=None, log_posteriors=False, variance_scales=None, pool_weights=None):
    """The detectors' padded outputs -> ProbEn input rows on the device (pe_proben_pack_detections; with temperatures
    pe_proben_pack_logits: probabilities and scores from class_logits as softmax(logits / T_d) in float64).
    Returns (boxes f64 [B*S,4], scores f64, probs f64 [B*S,K], vars f64, classes i32, offsets i32 [B], counts i32 [B],
    single-source flags i32 [B]), S = len(dets) * D.  log_posteriors (needs temperatures): pe_proben_pack_log_posteriors, the
    same eight plus the rows' log-posteriors f64 [B*S,K+1] as a ninth.
    variance_scales (one s per detector): pe_proben_pack_calibrated, whichever of the three routes the other arguments select, with
    vars = (double)var * s_d; None calls the three entry points above as before.
    pool_weights (one w per detector; only their presence and count matter here): pe_proben_pack_pooled, the same route with each
    written row's detector index i32 [B*S] appended as the LAST element of the result."""
    import ctypes
    nd = len(dets)
    if pool_weights is not None and not (isinstance(pool_weights, torch.Tensor) and pool_weights.is_cuda):
        from .calibration import check_pool_weights
        check_pool_weights(pool_weights, nd, "pack_rows")
    elif pool_weights is not None and pool_weights.numel() != nd:
        raise ValueError(f"pack_rows: {pool_weights.numel()} pool weights for {nd} detectors")
    if variance_scales is not None:
        from .calibration import check_variance_scales
        variance_scales = check_variance_scales(variance_scales, nd, "pack_rows")
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
    if temperatures is not None:       # (worded for fuse_detections, the caller these messages have always named)
        if len(temperatures) != nd:
            raise ValueError(f"fuse_detections: {len(temperatures)} temperatures for {nd} detectors")
        for d in dets:
            if d["class_logits"].shape != (B, D, K + 1) or d["class_logits"].dtype != torch.float32:
                raise ValueError(f"fuse_detections: class_logits {tuple(d['class_logits'].shape)} is not float32 [{B}, {D}, {K + 1}]")
    logits = temperatures is not None
    olp = torch.empty((B * S, K + 1), dtype=torch.float64, device=dev) if log_posteriors else None
    temps = (ctypes.c_double * nd)(*[float(t) for t in temperatures]) if logits else None
    scores, probs, lg = (None, None, arr("class_logits")) if logits else (arr("scores"), arr("prob_score"), None)
    dims = (nd, B, D, K, max_class, S)
    head, tail = [_lib.ptr(t) for t in (ob, os_, op)], [_lib.ptr(t) for t in (ov, oc, ooff, ocnt, osingle)]
    osrc = torch.empty((B * S,), dtype=torch.int32, device=dev) if pool_weights is not None else None
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


def fuse_detections(dets, score_fusion="probEn", box_fusion="v-avg", max_class=2, iou_thresh=0.5, temperatures=None,
                    class_prior=None, variance_scales=None, pool_weights=None, with_posterior=False, presence=None,
                    box_correlation=None):
    """Device-to-device stage fusion: `dets` = the result dicts of 2 or 3 detectors run on the SAME batch
    (rcnn.GeneralizedRCNN.forward_batch).  Packs their detections into ProbEn rows (classes <= max_class,
    like the JSON writer demo_FLIR_save_predictions.py:148-155), applies the reference's per-image case
    split (0 detectors -> nothing, 1 -> passthrough, >= 2 -> fusion; demo_probEn.py:237-267) and fuses.
    temperatures (one T per detector): the rows' probabilities and scores come from the detectors' class_logits as
    softmax(logits / T) in float64 (pe_proben_pack_logits) instead of the float32 prob_score / scores.
    score_fusion "probEn-log": pe_proben_pack_log_posteriors + pe_proben_fuse_batch_logp (temperatures None = 1 per detector;
    class_prior: K + 1 probabilities, background last, or the device tensor of log_class_prior).
    variance_scales (one s per detector): the rows' variances are (double)var * s_d (pe_proben_pack_calibrated); they weight the
    member boxes of box_fusion "v-avg" and "c-avg" and nothing else, so every other box rule and the NMS route give the bits they gave.
    pool_weights (one w per detector or pool_weight_tensor's device tensor, "probEn-log" only): pe_proben_pack_pooled +
    pe_proben_fuse_batch_pooled; the result then also holds "cluster" and "row_source".
    with_posterior ("probEn-log" only): the fusion is pe_proben_fuse_batch_posterior and the result also holds fuse_batch's
    "log_posterior", "vars" and "members".
    presence ("probEn-log" only; a table [2^D][K+1], D = len(dets), or calibration.presence_table's device tensor): the rows' detector
    indices come from pe_proben_pack_pooled and the fusion is pe_proben_fuse_batch_presence - images on which one detector fired are
    rescored row by row, not copied; the result then also holds "pattern", "cluster" and "row_source".
    box_fusion "c-avg" ("probEn-log" only) with box_correlation (a matrix [D][D], D = len(dets), or calibration.box_correlation_tensor's
    device tensor): the rows' detector indices come from pe_proben_pack_pooled and fuse_batch's second launch, pe_box_gls_batch,
    overwrites the boxes (and "vars") of the clusters of two or more rows; the result then also holds "cluster" and "row_source".
    No host synchronisation.  Returns a dict: boxes f64 [B*S,4], scores f32, classes f32, counts i32 [B],
    offsets i32 [B], stride S = len(dets) * D."""
    # the box heads' candidate-cap bookkeeping travels with the result (no kernel here): check_candidate_overflow() looks
    # at it at the consumer's first host synchronisation
    _check_mode(score_fusion, class_prior, "fuse_detections", pool_weights, with_posterior, presence, box_fusion, box_correlation)
    if box_correlation is not None:
        from .calibration import box_correlation_tensor
        box_correlation = box_correlation_tensor(box_correlation, len(dets), dets[0]["scores"].device)
    if presence is not None:
        from .calibration import presence_table
        presence = presence_table(presence, len(dets), dets[0]["prob_score"].shape[2] + 1, dets[0]["scores"].device)
    overflow_src = [(d["cand_total"], d["cand_max"]) for d in dets if "cand_total" in d]
    B, D = dets[0]["scores"].shape
    S = len(dets) * D
    dev = dets[0]["scores"].device
    logp = score_fusion == LOGP
    if logp and temperatures is None:
        temperatures = [1.0] * len(dets)
    ob, os_, op, ov, oc, ooff, ocnt, osingle, *olp = pack_rows(dets, max_class, temperatures, log_posteriors=logp,
                                                               variance_scales=variance_scales,
                                                               pool_weights=pool_weights if (presence is None and box_correlation is None)
                                                               or pool_weights is not None
                                                               else [1.0] * len(dets))      # only their presence matters to pack_rows
    osrc = olp.pop() if pool_weights is not None or presence is not None or box_correlation is not None else None
    if score_fusion == "max" and box_fusion == "argmax":
        from .layers import nms_batched_raw
        b32 = ob.float().view(B, S, 4)
        keep, kcnt = nms_batched_raw(b32, os_.float().view(B, S), oc.view(B, S), ocnt, None, iou_thresh, 0, S)
        # images where only ONE detector fired are passed through untouched by the reference (demo_probEn.py:239-254)
        single = osingle.bool()
        keep = torch.where(single[:, None], torch.arange(S, dtype=torch.int32, device=dev).expand(B, S), keep)
        kcnt = torch.where(single, ocnt, kcnt)
        # same contract as the ProbEn route: image b's fused rows are [offsets[b], offsets[b] + counts[b]) of the flat
        # arrays (score-descending), so late_fusion.fused_rows_device / comm.all_gather_fused_rows need no special case
        g = (torch.arange(B, device=dev).view(B, 1) * S + keep.clamp(0, S - 1).long()).view(-1)
        return {"boxes": ob[g], "scores": os_.float()[g], "classes": oc.float()[g], "counts": kcnt, "keep": keep,
                "offsets": ooff, "stride": S, "in_counts": ocnt, "nms_route": True, "cand_overflow_src": overflow_src}
    out = fuse_batch(ob, os_, op, ov, oc, ooff, score_fusion, box_fusion, max_rows=S, iou_thresh=iou_thresh,
                     row_counts=ocnt, passthrough=osingle, log_probs=olp[0] if logp else None, class_prior=class_prior,
                     pool_weights=pool_weights, row_source=osrc, with_posterior=with_posterior, presence=presence,
                     box_correlation=box_correlation)
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
