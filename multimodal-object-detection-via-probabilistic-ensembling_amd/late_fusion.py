"""The per-image late-fusion driver (demo/FLIR/demo_probEn.py:198-298 `apply_late_fusion_and_evaluate`) and
the prediction-JSON interchange (demo/FLIR/demo_FLIR_save_predictions.py:83-176), batched for the GPU.

J1 schema (kept readable / writable for drop-in): one dict of parallel per-image lists
  image, boxes [n][4], scores [n], classes [n], image_id, class_logits [n][K+1], probs [n][K], vars [n][1]
with detections of classes > 2 dropped."""
import json
import time

import numpy as np
import torch

from . import fusion as F
from . import options as O
from .structures import Boxes, Instances

J1_KEYS = ["image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars"]


def predictions_to_j1(file_names, image_ids, instances_list, max_class=2):
    """list of Instances (CPU or GPU) -> the reference's prediction dict (demo_FLIR_save_predictions.py:133-176)."""
    out = {k: [] for k in J1_KEYS}
    for name, iid, inst in zip(file_names, image_ids, instances_list):
        inst = inst.to("cpu")
        boxes = inst.pred_boxes.tensor.tolist()
        scores = inst.scores.tolist()
        classes = inst.pred_classes.tolist()
        logits = inst.class_logits.tolist() if inst.has("class_logits") else [[] for _ in boxes]
        probs = inst.prob_score.tolist() if inst.has("prob_score") else [[] for _ in boxes]
        var = inst.vars.tolist() if inst.has("vars") else [[1.0] for _ in boxes]
        keep = [j for j in range(len(boxes)) if classes[j] <= max_class]
        out["image"].append(name)
        out["boxes"].append([boxes[j] for j in keep])
        out["scores"].append([scores[j] for j in keep])
        out["classes"].append([classes[j] for j in keep])
        out["image_id"].append(iid)
        out["class_logits"].append([logits[j] for j in keep])
        out["probs"].append([probs[j] for j in keep])
        out["vars"].append([var[j] for j in keep])
    return out


def write_j1(path, pred):
    with open(path, "w") as f:
        json.dump(pred, f, indent=2)


def read_j1(path):
    with open(path) as f:
        d = json.load(f)
    for k in J1_KEYS:
        assert k in d, f"{path}: missing key '{k}' of the prediction schema"
    return d


def shard_j1(det, index_range):
    """The slice of a prediction dict one rank works on (contiguous InferenceSampler block: rank order == image order)."""
    lo, hi = (index_range.start, index_range.stop) if len(index_range) else (0, 0)
    return {k: v[lo:hi] for k, v in det.items()}


def _info(det, i):
    d = {"img_name": det["image"][i], "bbox": det["boxes"][i], "score": det["scores"][i], "class": det["classes"][i],
         "class_logits": det["class_logits"][i], "prob": det["probs"][i], "vars": det["vars"][i]}
    if "log_probs" in det:        # calibration.calibrate_j1(log_probs=True): score_fusion "probEn-log"
        d["log_prob"] = det["log_probs"][i]
    return d


def _calibrated(dets, opts, names, device):
    """The prediction dicts as the fusion reads them: vars times the variance scales (calibration.scale_j1_vars: float64, the single
    multiply of the device route's pe_proben_pack_calibrated), probs / scores - and, "probEn-log", log_probs - rebuilt from the
    class_logits at the temperatures (calibration.calibrate_j1).  `names` (the files) word the refusal of a file without logits: every
    file is checked before the first launch."""
    from . import calibration
    if opts.variance_scales is not None:
        dets = [calibration.scale_j1_vars(d, s) for d, s in zip(dets, opts.variance_scales)]
    if opts.temperatures is not None:
        names = names or [f"prediction file {k + 1}" for k in range(len(dets))]
        for d, n in zip(dets, names):
            calibration.require_logits(d, n)
        dets = [calibration.calibrate_j1(d, t, n, device, log_probs=opts.logp) for d, t, n in zip(dets, opts.temperatures, names)]
    return dets


def late_fusion(dets, method, device="cuda", temperatures=None, names=None, class_prior=None, variance_scales=None,
                pool_weights=None, with_posterior=False, presence=None, box_correlation=None, options=None, iou_thresh=None,
                stats=None):
    """dets: 2 or 3 J1 dicts over the same images (order = detector order).  Returns per-image
    (boxes float64 [m,4] | None, scores f32, classes f32); None = skipped image (no detector fired).
    Case split of demo_probEn.py:237-267: 0 detectors -> skip, 1 -> passthrough, >= 2 -> fusion of the
    non-empty lists in order.  All images needing fusion go through ONE batched launch.
    The option keywords, or `options` (options.FusionOptions, which documents them; not both), one value per file; a row's detector is
    its file's position in dets, what pe_proben_pack_pooled writes on the device route.  Temperatures and variance scales are applied
    to the files before the case split (_calibrated), so passed-through rows carry the calibrated score like the device route's.
    with_posterior: every per-image result is a 6-tuple, the three above plus (log_posterior f64 [m, K+1], vars f64 [m], members i32
    [m]); a passed-through image takes its log-posterior from the calibrated file ("log_probs") and its vars from the scaled file, what
    the device route's passthrough copies.
    presence: images on which one detector fired are no longer answered on the host: they go into the batched launch with their
    passthrough flag set and come back rescored row by row (never clustered), which is what the device route does with the pack
    kernel's single-source flag - the two routes stay byte-identical.
    method ("wbf", "wbf") (weighted boxes fusion, pe_wbf_fuse_batch): there is no case split at all, an image on which one detector
    fired goes into the batched launch like any other and comes back fused (a lone box at score * min(1, U) / U).  iou_thresh: None is
    fuse_batch's default (0.5; 0.55 for "wbf").  stats: a dict that receives "skipped", the rows "wbf" skipped over all images."""
    opts = O.FusionOptions.of(options, "late_fusion", len(dets), method[0], method[1], temperatures=temperatures, class_prior=class_prior,
                              variance_scales=variance_scales, pool_weights=pool_weights, with_posterior=with_posterior,
                              presence=presence, box_correlation=box_correlation)
    dets = _calibrated(dets, opts, names, device)
    with_posterior, presence, logp = opts.with_posterior, opts.presence, opts.logp
    n_img = len(dets[1]["image"]) if len(dets) > 1 else len(dets[0]["image"])      # the reference loops over det_2's images (:205)
    results = [None] * n_img
    batch, where, single = [], [], []
    for i in range(n_img):
        infos = [_info(d, i) for d in dets]
        live = [x for x in infos if len(x["bbox"]) > 0]
        if len(live) == 0:
            continue
        if len(live) == 1 and presence is None and not opts.wbf:
            x = live[0]
            results[i] = (np.array(x["bbox"], dtype=np.float64), torch.tensor(x["score"], dtype=torch.float32),
                          torch.tensor(x["class"], dtype=torch.float32))
            if with_posterior:
                m = len(x["bbox"])
                results[i] += (np.asarray(x["log_prob"], dtype=np.float64).reshape(m, -1),
                               np.asarray(x["vars"], dtype=np.float64).reshape(m), np.ones(m, dtype=np.int32))
            continue
        batch.append(infos if opts.needs_row_source else live)      # pack_infos skips the empty ones; the positions stay
        where.append(i)
        single.append(int(len(live) == 1))          # presence only: the image's passthrough flag
    if batch:
        if method[0] == "max" and method[1] == "argmax":
            for i, live in zip(where, batch):
                b, s, c = F.fusion(method, *live)
                results[i] = (b.double().numpy(), s, c)
        else:
            b, s, p, v, c, offs, *rest = F.pack_infos(batch, device, with_log_probs=logp, with_sources=opts.needs_row_source)
            out = F.fuse_batch(b, s, p, v, c, offs, log_probs=rest[0] if logp else None,
                               row_source=rest[-1] if opts.needs_row_source else None, options=opts, iou_thresh=iou_thresh,
                               passthrough=torch.tensor(single, dtype=torch.int32, device=b.device) if presence is not None else None)
            cnt = out["counts"].cpu().numpy()
            ob, os_, oc = out["boxes"].cpu().numpy(), out["scores"].cpu(), out["classes"].cpu()
            oh = offs.cpu().numpy()
            post = [out[k].cpu().numpy() for k in ("log_posterior", "vars", "members")] if with_posterior else []
            for j, i in enumerate(where):
                sl = slice(oh[j], oh[j] + cnt[j])
                results[i] = (ob[sl], os_[sl], oc[sl]) + tuple(x[sl] for x in post)
            if stats is not None and opts.wbf:
                stats["skipped"] = stats.get("skipped", 0) + int(out["skipped"].sum().item())
    return results


def _fused_j1_rows(out, boxes, scores, classes, log_posterior, variances):
    """One image's fused rows appended to the J1 lists of `out`; returns the background rows left out."""
    if len(scores) == 0:
        for key in ("boxes", "scores", "classes", "class_logits", "probs", "vars"):
            out[key].append([])
        return 0
    lq = np.asarray(log_posterior, dtype=np.float64).reshape(len(scores), -1)
    k = lq.shape[1] - 1
    cls = np.asarray(classes).astype(np.int64)
    keep = np.nonzero(cls != k)[0]
    out["boxes"].append(np.asarray(boxes, dtype=np.float64).reshape(-1, 4)[keep].tolist())
    out["scores"].append([float(x) for x in np.asarray(scores, dtype=np.float32)[keep]])
    out["classes"].append(cls[keep].tolist())
    out["class_logits"].append(lq[keep].tolist())
    out["probs"].append(np.exp(lq[keep, :k]).tolist())
    out["vars"].append([[float(v)] for v in np.asarray(variances, dtype=np.float64)[keep]])
    return len(cls) - len(keep)


def fused_to_j1(dets, fused):
    """The fused detections of late_fusion(dets, ..., with_posterior=True) as a prediction dict (J1 schema) over the same images - a
    detector's file in its own right, so a fusion can be cascaded, refitted or reported on.  class_logits = the fused log-posterior
    (softmax(class_logits / 1) is the fused posterior: a valid "probEn-log" input at T = 1), probs = exp of its first K columns,
    scores / classes = the float32 score and the class the fusion wrote, vars = [[the fused box's variance]]; image / image_id are
    dets[1]'s, as the driver pairs them.  A skipped image (no detector fired) gets empty lists.  Rows whose fused class is the
    background column K are not detections and are not written.  Returns (the dict, the number of background rows dropped)."""
    ref = dets[1] if len(dets) > 1 else dets[0]
    out = {k: [] for k in J1_KEYS}
    dropped = 0
    for i, r in enumerate(fused):
        out["image"].append(ref["image"][i])
        out["image_id"].append(ref["image_id"][i])
        if r is None:
            for k in ("boxes", "scores", "classes", "class_logits", "probs", "vars"):
                out[k].append([])
            continue
        if len(r) != 6:
            raise ValueError("fused_to_j1: the fused rows carry no posterior (late_fusion(..., with_posterior=True) writes it)")
        dropped += _fused_j1_rows(out, r[0], r[1].numpy() if isinstance(r[1], torch.Tensor) else r[1],
                                  r[2].numpy() if isinstance(r[2], torch.Tensor) else r[2], r[3], r[4])
    return out, dropped


def _plain_j1_rows(out, boxes, scores, classes):
    """One image's fused rows appended to the J1 lists of `out` as predictions_to_j1 writes a detector without logit, probability and
    variance heads: class_logits [], probs [], vars [1.0]."""
    m = len(scores)
    out["boxes"].append(np.asarray(boxes, dtype=np.float64).reshape(-1, 4).tolist())
    out["scores"].append([float(x) for x in np.asarray(scores, dtype=np.float32)])
    out["classes"].append(np.asarray(classes).astype(np.int64).tolist())
    out["class_logits"].append([[] for _ in range(m)])
    out["probs"].append([[] for _ in range(m)])
    out["vars"].append([[1.0] for _ in range(m)])


def wbf_to_j1(dets, fused):
    """The fused detections of late_fusion(dets, ("wbf", "wbf")) as a prediction dict (J1 schema) over the same images: boxes, scores and
    classes as fused, and what predictions_to_j1 writes for a detector without those heads - class_logits [], probs [], vars [1.0] -,
    since weighted boxes fusion forms no posterior and no variance.  Enough for bootstrap_ap and the evaluators; not an input of
    "probEn".  image / image_id are dets[1]'s, as the driver pairs them; an image no detector fired on gets empty lists."""
    ref = dets[1] if len(dets) > 1 else dets[0]
    out = {k: [] for k in J1_KEYS}
    for i, r in enumerate(fused):
        out["image"].append(ref["image"][i])
        out["image_id"].append(ref["image_id"][i])
        if r is None:
            r = (np.zeros((0, 4)), np.zeros((0,), dtype=np.float32), np.zeros((0,), dtype=np.float32))
        _plain_j1_rows(out, r[0], r[1].numpy() if isinstance(r[1], torch.Tensor) else r[1],
                       r[2].numpy() if isinstance(r[2], torch.Tensor) else r[2])
    return out


def wbf_device_to_j1(fused, file_names, image_ids):
    """wbf_to_j1 for the device route: `fused` = the result of fusion.fuse_detections(..., "wbf", "wbf") on one batch.  Synchronises (the
    rows leave for the host).  Returns (the dict, the rows the fusion skipped on this batch)."""
    if "skipped" not in fused:
        raise ValueError("wbf_device_to_j1: the fused rows are not those of score_fusion 'wbf'")
    S = fused["stride"]
    cnt = fused["counts"].cpu().numpy()
    host = {k: fused[k].cpu().numpy() for k in ("boxes", "scores", "classes")}
    out = {k: [] for k in J1_KEYS}
    for b, (name, iid) in enumerate(zip(file_names, image_ids)):
        out["image"].append(name)
        out["image_id"].append(iid)
        if cnt[b] < 0:
            raise RuntimeError(f"wbf_device_to_j1: image {name} has more rows than the fusion's bound")
        sl = slice(b * S, b * S + int(cnt[b]))
        _plain_j1_rows(out, *(host[k][sl] for k in ("boxes", "scores", "classes")))
    return out, int(fused["skipped"].sum().item())


def fused_device_to_j1(fused, file_names, image_ids):
    """fused_to_j1 for the device route: `fused` = the result of fusion.fuse_detections(..., with_posterior=True) on one batch,
    file_names / image_ids the batch's.  The same dict the file route builds from the same detections; synchronises (the rows leave
    for the host).  Returns (the dict, the number of background rows dropped)."""
    if "log_posterior" not in fused:
        raise ValueError("fused_device_to_j1: the fused rows carry no posterior (fuse_detections(..., with_posterior=True) writes it)")
    S = fused["stride"]
    cnt = fused["counts"].cpu().numpy()
    host = {k: fused[k].cpu().numpy() for k in ("boxes", "scores", "classes", "log_posterior", "vars")}
    out = {k: [] for k in J1_KEYS}
    dropped = 0
    for b, (name, iid) in enumerate(zip(file_names, image_ids)):
        out["image"].append(name)
        out["image_id"].append(iid)
        if cnt[b] < 0:
            raise RuntimeError(f"fused_device_to_j1: image {name} has more rows than the fusion's bound")
        sl = slice(b * S, b * S + int(cnt[b]))
        dropped += _fused_j1_rows(out, *(host[k][sl] for k in ("boxes", "scores", "classes", "log_posterior", "vars")))
    return out, dropped


def fused_clusters(dets, box_fusion="v-avg", device="cuda", temperatures=None, names=None, class_prior=None, variance_scales=None,
                   options=None):
    """The clusters "probEn-log" forms over dets (late_fusion's arguments), for the pooling-weight fit and its report: the images
    where two or more detectors fired go through ONE pe_proben_fuse_batch_pooled launch at w = 1 - which is probEn-log bit for bit -
    with out_cluster, and the clusters come back in CSR form, built with torch on the device.  Clustering and the fused boxes do not
    depend on the weights, so the clusters are those of every w.  Returns None when no image has two live detectors, else a dict
    of device tensors: log_probs f64 [N, K+1] and row_source i32 [N] (the packed rows), member_rows i32 [M] / cluster_offsets i32
    [C+1] (cluster c = fused row c, image-major; its rows in packed order), boxes f64 [C, 4] (the fused boxes), box_offsets i32
    [B'+1] (the clusters of fused image j), and "images": the B' positions of the fused images in dets; "row_boxes" f64 [N, 4] and
    "row_vars" f64 [N] (the packed rows' boxes and scaled variances: what calibration.fit_box_correlation takes its residuals from)."""
    D = len(dets)
    opts = O.FusionOptions.of(options, "fused_clusters", D, F.LOGP, box_fusion, temperatures=temperatures, class_prior=class_prior,
                              variance_scales=variance_scales)
    opts = opts.replace(pool_weights=[1.0] * D, with_posterior=False, presence=None)       # w = 1, for "cluster"
    dets = _calibrated(dets, opts, names, device)
    batch, where = [], []
    for i in range(len(dets[0]["image"])):
        infos = [_info(d, i) for d in dets]
        if sum(len(x["bbox"]) > 0 for x in infos) >= 2:
            batch.append(infos)
            where.append(i)
    if not batch:
        return None
    b, s, p, v, c, offs, lp, src = F.pack_infos(batch, device, with_log_probs=True, with_sources=True)
    out = F.fuse_batch(b, s, p, v, c, offs, log_probs=lp, row_source=src, options=opts)
    dev = b.device
    cnt, in_off = out["counts"].long(), offs.long()
    assert int(cnt.min()) >= 0, "fused_clusters: an image over the row bound"       # max_rows is the longest image: cannot happen
    C = int(cnt.sum())
    base = torch.cumsum(cnt, 0) - cnt                                               # the first cluster of every image
    img = torch.repeat_interleave(torch.arange(len(batch), device=dev), in_off[1:] - in_off[:-1])
    cl = out["cluster"].long()
    rows = torch.nonzero(cl >= 0).flatten()                                         # -1: the row left the pool without a cluster
    gid = base[img[rows]] + cl[rows]
    order = torch.sort(gid, stable=True).indices
    zero = torch.zeros((1,), dtype=torch.long, device=dev)
    first = torch.repeat_interleave(in_off[:-1] - base, cnt) + torch.arange(C, device=dev)      # cluster c's fused row
    return {"log_probs": lp, "row_source": src, "member_rows": rows[order].to(torch.int32),
            "cluster_offsets": torch.cat([zero, torch.cumsum(torch.bincount(gid, minlength=C), 0)]).to(torch.int32),
            "boxes": out["boxes"][first], "box_offsets": torch.cat([zero, torch.cumsum(cnt, 0)]).to(torch.int32), "images": where,
            "row_boxes": b, "row_vars": v}


def presence_rows(dets, box_fusion="v-avg", device="cuda", temperatures=None, names=None, class_prior=None, variance_scales=None,
                  pool_weights=None, presence=None, options=None):
    """Every fused row "probEn-log" forms over dets (late_fusion's arguments) under a presence table, for the table's fit and its
    report: all images on which a detector fired go through ONE pe_proben_fuse_batch_presence launch - images with one live detector
    with their passthrough flag set, as in late_fusion - with the posterior outputs and out_pattern.  presence None = the zero table:
    the fused log-posterior is then the `base` of calibration.fit_presence.  Clustering and boxes do not depend on the table.
    Returns None when no detector fired anywhere, else a dict of device tensors over the C fused rows, image-major: log_posterior f64
    [C, K+1], pattern i32 [C], boxes f64 [C, 4], box_offsets i32 [B'+1] (the rows of fused image j), and "images": the B' positions of
    the fused images in dets."""
    opts = O.FusionOptions.of(options, "presence_rows", len(dets), F.LOGP, box_fusion, temperatures=temperatures, class_prior=class_prior,
                              variance_scales=variance_scales, pool_weights=pool_weights, presence=presence)
    dets = _calibrated(dets, opts, names, device)
    batch, where, single = [], [], []
    for i in range(len(dets[0]["image"])):
        infos = [_info(d, i) for d in dets]
        live = sum(len(x["bbox"]) > 0 for x in infos)
        if live >= 1:
            batch.append(infos)
            where.append(i)
            single.append(int(live == 1))
    if not batch:
        return None
    b, s, p, v, c, offs, lp, src = F.pack_infos(batch, device, with_log_probs=True, with_sources=True)
    table = np.zeros((2 ** len(dets), lp.shape[1])) if opts.presence is None else opts.presence
    out = F.fuse_batch(b, s, p, v, c, offs, log_probs=lp, row_source=src, options=opts.replace(with_posterior=True, presence=table),
                       passthrough=torch.tensor(single, dtype=torch.int32, device=b.device))
    dev = b.device
    cnt, in_off = out["counts"].long(), offs.long()
    assert int(cnt.min()) >= 0, "presence_rows: an image over the row bound"       # max_rows is the longest image: cannot happen
    C = int(cnt.sum())
    base = torch.cumsum(cnt, 0) - cnt
    first = torch.repeat_interleave(in_off[:-1] - base, cnt) + torch.arange(C, device=dev)      # fused row c's place in the outputs
    zero = torch.zeros((1,), dtype=torch.long, device=dev)
    return {"log_posterior": out["log_posterior"][first], "pattern": out["pattern"][first], "boxes": out["boxes"][first],
            "box_offsets": torch.cat([zero, torch.cumsum(cnt, 0)]).to(torch.int32), "images": where}


def apply_late_fusion_and_evaluate(cfg, evaluator, det_1, det_2, method, det_3="", image_hw=None, device="cuda",
                                   img_folder="../../../Datasets/FLIR/val/thermal_8_bit/", temperatures=None, names=None,
                                   class_prior=None, variance_scales=None, pool_weights=None, fused_out=None, presence=None,
                                   box_correlation=None, options=None, iou_thresh=None, stats=None):
    """Same call as the reference (demo_probEn.py:198).  `image_hw`: {image_id: (H, W)} from the dataset
    json (the reference re-reads every thermal JPEG just for its shape); default 512 x 640 (FLIR).
    `img_folder`: the prefix the reference hard-codes into the `file_name` it hands to the evaluator (:200,271).
    `fused_out`: a list; when given ("probEn-log" only) the fusion keeps its posterior and the per-image 6-tuples of late_fusion are
    appended to it, for fused_to_j1 - the evaluator receives what it receives without it.
    The option keywords, or `options` (options.FusionOptions; not both), are late_fusion's; with `options`, fused_out needs one
    built with_posterior - or, for ("wbf", "wbf"), nothing: the per-image 3-tuples are appended, for wbf_to_j1.  iou_thresh and stats
    are late_fusion's.
    What the evaluator receives per image is pinned by tests/golden/p5_cases.json (the reference's function run with a recording
    evaluator): tests/test_pipeline_gpu.py::test_late_fusion_driver_reproduces_the_references_records."""
    dets = [det_1, det_2] + ([det_3] if det_3 else [])
    opts = O.FusionOptions.of(options, "late_fusion", len(dets), method[0], method[1], temperatures=temperatures, class_prior=class_prior,
                              variance_scales=variance_scales, pool_weights=pool_weights,
                              with_posterior=fused_out is not None and options is None and F.WBF not in method, presence=presence,
                              box_correlation=box_correlation)
    if fused_out is not None and not (opts.with_posterior or opts.wbf):
        raise ValueError("apply_late_fusion_and_evaluate: fused_out needs options built with_posterior")
    evaluator.reset()
    print("Method: ", method)
    start = time.time()
    fused = late_fusion(dets, method, device, names=names, options=opts, iou_thresh=iou_thresh, stats=stats)
    if fused_out is not None:
        fused_out.extend(fused)
    for i, r in enumerate(fused):
        if r is None:
            continue
        iid = det_2["image_id"][i]
        H, W = (image_hw or {}).get(iid, (512, 640))
        boxes, scores, classes = r[:3]
        inst = Instances((H, W))
        inst.pred_boxes = Boxes(torch.as_tensor(np.asarray(boxes), dtype=torch.float32).reshape(-1, 4))
        inst.scores = scores
        inst.pred_classes = classes
        name = img_folder + det_1["image"][i].split(".")[0] + ".jpeg"
        evaluator.process([{"file_name": name, "height": H, "width": W, "image_id": iid}], [{"instances": inst}])
    print("Average time:", (time.time() - start) / max(len(det_2["image"]), 1))
    return evaluator.evaluate()


def fused_rows_device(fused, image_ids, valid_classes=(0, 1, 2, 5, 7, 16)):
    """Evaluation rows of one batch ON THE DEVICE: [n,7] float64 = (image_id, x, y, w, h, score, category_id) with the
    evaluator's class whitelist / remap (FLIR_evaluation.py:313-382) applied - the tensor form that crosses ranks in
    comm.all_gather_rows (one RCCL all-gather instead of the reference's pickled lists over gloo).
    `fused`: result of fusion.fuse_detections (or any dict with boxes [B*S,4], scores, classes, counts, offsets, stride)."""
    B = fused["counts"].numel()
    S = fused["stride"]
    dev = fused["scores"].device
    F.check_candidate_overflow(fused)   # evaluation rows leave for the host / other ranks from here: the one sync point
    slot = torch.arange(S, device=dev).unsqueeze(0)                                  # [1,S]
    live = slot < fused["counts"].unsqueeze(1)                                       # [B,S]
    cls = fused["classes"].view(B, S).to(torch.int64)
    ok = torch.zeros_like(live)
    for c in valid_classes:
        ok |= cls == c
    live &= ok
    cat = torch.where((cls == 5) | (cls == 7), torch.full_like(cls, 2), cls)
    b = fused["boxes"].view(B, S, 4).double()
    ids = torch.as_tensor(image_ids, dtype=torch.float64, device=dev).view(B, 1).expand(B, S)
    rows = torch.stack([ids, b[..., 0], b[..., 1], b[..., 2] - b[..., 0], b[..., 3] - b[..., 1],
                        fused["scores"].view(B, S).double(), cat.double()], dim=2)
    return rows[live]                                                               # image-major, score order kept
