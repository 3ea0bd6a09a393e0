"""Paired bootstrap of the KAIST log-average miss rate over images.

Matching in evalKAIST/evaluation_script.py is per image, so it is done once by KAISTPedEval.evaluate on the host; a replicate that holds
image i m_i times only re-runs accumulate, as a weighted scan over the exported list on the GPU (pe_lamr_bootstrap,
csrc/lamr_bootstrap.hip).  The kernel returns integers; the host turns them into the figures with the evaluator's own expressions, so a
replicate equals KAISTPedEval on the dataset with m_i adjacent copies of image i bit for bit (section 28 has the argument and its one
condition: detections that tie in score inside one image must agree in tp / fp / ignored).

    export_lamr_matches(annotation, results, id_setup, fix_row_index)   the list, on the host, with the evaluator
    mixed_score_ties(matches)                                           how often that condition is not met
    lamr_cells(n_images, day_frames)                                    all / day / night as image-index ranges over ONE list
    lamr_bootstrap(matches, mult, cells, device)                        tp_at / totals / valid per replicate and cell
    lamr_statistics(run, matches)                                       MR, the nine miss rates and recall_all per replicate and cell
    resample_multiplicities_stratified(bounds, replicates, seed)        day and night resampled each to its own size
    bootstrap_lamr(annotation, results_a, results_b=None, ...)          point estimates, percentile intervals, standard errors, paired differences
"""
import copy

import numpy as np
import torch

from . import _lib
from .bootstrap import _interval, _narrow, check_same_images, paired, resample_multiplicities
from .evalKAIST.evaluation_script import DAY_FRAMES, KAIST, KAISTPedEval

SUBSETS = ("all", "day", "night")


def _as_gt(annotation):
    """A KAIST annotation: the file's path, its dict, or the loaded object."""
    if isinstance(annotation, KAIST):
        return annotation
    if isinstance(annotation, dict):
        gt = KAIST()
        gt.dataset = annotation
        gt._index()
        return gt
    return KAIST(annotation)


def _as_dt(gt, results):
    """Whatever KAIST.loadRes reads (txt rows, a COCO-result json, a list of result dicts), or the loaded object."""
    return results if isinstance(results, KAIST) else gt.loadRes(results)


def export_lamr_matches(annotation, results, id_setup=0, fix_row_index=False):
    """KAISTPedEval.evaluate(id_setup) over ALL image ids (sorted), flattened in image order and stably sorted by descending score -
    accumulate's own order.  Host arrays: list_img i32 [L] (position in the sorted image ids), list_flags u8 [L] (bit 0 matched, bit 1
    ignored), list_score f64 [L], npig i32 [I] (0 for an image whose evaluateImg is None), img_ids; "evaluator" is the KAISTPedEval."""
    gt = _as_gt(annotation)
    ev = KAISTPedEval(gt, _as_dt(gt, results), "bbox")
    ev.params.catIds = [1]
    ev.params.fixRowIndex = bool(fix_row_index)
    ev.evaluate(id_setup)
    p = ev.params
    t = int(np.argmin(np.abs(p.iouThrs - 0.5)))                    # the threshold summarize() reads
    I = len(p.imgIds)
    per = [(i, e) for i, e in enumerate(ev.evalImgs) if e is not None]
    npig = np.zeros(I, dtype=np.int32)
    for i, e in per:
        npig[i] = np.count_nonzero(~e["gtIgnore"])
    scores = np.concatenate([e["dtScores"] for _, e in per] + [np.zeros(0)])
    img = np.concatenate([np.full(len(e["dtScores"]), i, dtype=np.int32) for i, e in per] + [np.zeros(0, dtype=np.int32)])
    matched = np.concatenate([e["dtMatches"][t] for _, e in per] + [np.zeros(0, dtype=bool)])
    ignored = np.concatenate([e["dtIgnore"][t] for _, e in per] + [np.zeros(0, dtype=bool)])
    order = np.argsort(-scores, kind="mergesort")
    flags = (matched.astype(np.uint8) | (ignored.astype(np.uint8) << 1))[order]
    return {"list_img": np.ascontiguousarray(img[order], dtype=np.int32), "list_flags": np.ascontiguousarray(flags, dtype=np.uint8),
            "list_score": scores[order], "npig": npig, "img_ids": list(p.imgIds), "id_setup": id_setup, "evaluator": ev}


def mixed_score_ties(matches):
    """The number of neighbours in the list that belong to one image, tie in score (NaN ties with NaN) and differ in what they count
    as (tp / fp / ignored).  Section 28's one condition: where this is 0, every replicate is the evaluator on the duplicated dataset
    bit for bit; a pair counted here is weighed entry by entry where a duplicated image would repeat the pair as a whole."""
    li, s, f = matches["list_img"], matches["list_score"], matches["list_flags"]
    kind = np.where(f & 2, 2, f & 1)
    tie = (li[1:] == li[:-1]) & ((s[1:] == s[:-1]) | (np.isnan(s[1:]) & np.isnan(s[:-1])))
    return int(np.count_nonzero(tie & (kind[1:] != kind[:-1])))


def lamr_cells(n_images, day_frames=DAY_FRAMES):
    """int32 [3, 2] = (lo, hi) of all / day / night (SUBSETS order): day is the first day_frames of the sorted image ids, night the rest."""
    if n_images < 0 or day_frames < 0:
        raise ValueError(f"lamr_cells: n_images {n_images} and day_frames {day_frames} must be >= 0")
    d = min(int(day_frames), int(n_images))
    return np.array([[0, n_images], [0, d], [d, n_images]], dtype=np.int32)


def resample_multiplicities_stratified(bounds, replicates, seed):
    """resample_multiplicities with strata: bounds lists the (lo, hi) image-index ranges that partition [0, n_images) in order (day,
    night); every row but row 0 (all ones) draws hi - lo images with replacement inside each stratum, so each stratum keeps its size.
    int64 [replicates, n_images]; same arguments, same bytes."""
    bounds = [(int(lo), int(hi)) for lo, hi in bounds]
    if not bounds or bounds[0][0] != 0 or any(lo > hi for lo, hi in bounds) or any(a[1] != b[0] for a, b in zip(bounds, bounds[1:])):
        raise ValueError(f"resample_multiplicities_stratified: {bounds} is not a partition of [0, n_images) into ranges in order")
    n_images = bounds[-1][1]
    if n_images < 1 or replicates < 1:
        raise ValueError(f"resample_multiplicities_stratified: n_images {n_images} and replicates {replicates} must be >= 1")
    mult = np.ones((replicates, n_images), dtype=np.int64)
    if replicates > 1:
        rng = np.random.default_rng(seed)
        for lo, hi in bounds:
            if hi > lo:
                mult[1:, lo:hi] = rng.multinomial(hi - lo, np.full(hi - lo, 1.0 / (hi - lo)), size=replicates - 1)
    return mult


def lamr_bootstrap(matches, mult, cells, device="cuda"):
    """One launch of pe_lamr_bootstrap over mult [B, I] and cells [C, 2].  Returns host arrays: tp_at i64 [B, C, R] (the weighted true
    positives at the last operating point below each FPPI reference), totals i64 [B, C, 4] = N, NP, TP_tot, FP_tot, valid i32 [B, C];
    "cells" is what was evaluated."""
    thr = np.ascontiguousarray(matches["evaluator"].params.fppiThrs, dtype=np.float64)
    I, R, L = len(matches["npig"]), len(thr), len(matches["list_img"])
    m8 = _narrow(mult, I)
    cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
    B, C = m8.shape[0], cells.shape[0]
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    d_img, d_flags, d_npig = up(matches["list_img"]), up(matches["list_flags"]), up(matches["npig"])
    d_mult, d_cells, d_thr = up(m8), up(cells), up(thr)
    _lib.require_cuda(d_mult)
    tp_at = torch.empty((B, C, R), dtype=torch.int64, device=dev)
    totals = torch.empty((B, C, 4), dtype=torch.int64, device=dev)
    valid = torch.empty((B, C), dtype=torch.int32, device=dev)
    ptr = lambda t: _lib.ptr(t) if t.numel() else None      # noqa: E731
    with torch.cuda.device(dev):
        st = _lib.lib().pe_lamr_bootstrap(ptr(d_img), ptr(d_flags), L, ptr(d_npig), ptr(d_mult), B, I, ptr(d_thr), R, ptr(d_cells), C,
                                          ptr(tp_at), ptr(totals), ptr(valid), _lib.stream())
    _lib.check(st, "pe_lamr_bootstrap")
    out = {"tp_at": tp_at.cpu().numpy(), "totals": totals.cpu().numpy(), "valid": valid.cpu().numpy(), "cells": cells}
    if (out["valid"] < 0).any():
        raise ValueError(f"pe_lamr_bootstrap: a cell is not an image-index range inside [0, {I}]")
    return out


def figures(tp_at, NP, TP_tot, FP_tot):
    """One (replicate, cell): (MR, the miss rates at the references, recall_all) from the integers, by the evaluator's own expressions
    (accumulate: `recall = tp / npig`, `yy = 1 - recall`; summarize: `exp(mean(log(1 - recall)))` over a contiguous 1-D array; evaluate:
    `1 - yy[0][-1]`, nan when there is no operating point).  NP = 0: the evaluator leaves the cell at -1."""
    if NP == 0:
        return -1.0, np.full(len(tp_at), -1.0), -1.0
    recall = np.ascontiguousarray(tp_at).astype(np.float64) / int(NP)
    mrs = 1 - recall
    with np.errstate(divide="ignore"):
        mr = float(np.exp(np.mean(np.log(mrs))))
    rec_all = float(1 - (1 - np.float64(TP_tot) / int(NP))) if TP_tot + FP_tot > 0 else float("nan")
    return mr, mrs, rec_all


def lamr_statistics(run, matches=None):
    """{"MR" [B, C], "miss_rates" [B, C, R], "recall_all" [B, C]} from lamr_bootstrap's output, row by row (NumPy's pairwise sum over 9
    contiguous values and a reduction along an axis add in different orders: the mean is not vectorised over the replicates).  -1
    where the cell is undefined (NP = 0); recall_all is nan where there is ground truth and no counted detection, as evaluate() has it."""
    tp_at, totals = run["tp_at"], run["totals"]
    B, C, R = tp_at.shape
    mr, mrs, rec = np.empty((B, C)), np.empty((B, C, R)), np.empty((B, C))
    for b in range(B):
        for c in range(C):
            _, NP, TP, FP = (int(x) for x in totals[b, c])
            mr[b, c], mrs[b, c], rec[b, c] = figures(tp_at[b, c], NP if run["valid"][b, c] > 0 else 0, TP, FP)
    return {"MR": mr, "miss_rates": mrs, "recall_all": rec}


def subset_evaluators(matches, cells):
    """The evaluator's own figures per cell: KAISTPedEval over the cell's image ids, accumulated (its per-image records are the ones
    evaluate() makes for those ids: matching is per image)."""
    ev, out = matches["evaluator"], []
    for lo, hi in np.asarray(cells).reshape(-1, 2).tolist():
        sub = copy.copy(ev)
        sub.params = copy.deepcopy(ev.params)
        sub.params.imgIds = list(ev.params.imgIds[lo:hi])
        sub.evalImgs = ev.evalImgs[lo:hi]
        sub.accumulate()
        out.append(sub)
    return out


def point_estimates(sub, id_setup):
    """(MR, the nine miss rates, recall_all) as evaluate() and demo_LAMR_KAIST read them off an accumulated evaluator."""
    yy = sub.eval["yy"]
    return (float(sub.summarize(id_setup)), 1 - sub.eval["TP"][0, :, 0, 0], float(1 - yy[0][-1]) if yy and len(yy[0]) else float("nan"))


def _undefined(x):
    return ~np.isfinite(x) | (x <= -1)


def bootstrap_lamr(annotation, results_a, results_b=None, replicates=2000, seed=0, confidence=0.95, setups=(0,), fix_row_index=False,
                   day_frames=DAY_FRAMES, stratified=False, device="cuda"):
    """Percentile-bootstrap intervals of MR, the miss rates at the nine FPPI references and recall, per (setup, subset) for results_a
    (and results_b, under the SAME resamples, with the paired difference b - a, its interval and the two-sided bootstrap p-value, as
    bootstrap_ap reports it).  The point estimates are KAISTPedEval's own; the replicates are rows 1.. of the resamples (row 0, the
    dataset itself, is evaluated with them and is not part of the distribution).  stratified: day and night are resampled each to its
    own size."""
    if not 0.0 < confidence < 1.0:
        raise ValueError(f"confidence {confidence} is not in (0, 1)")
    if replicates < 2:
        raise ValueError(f"replicates {replicates}: the resamples are rows 1.. (row 0 is the dataset itself), so at least 2")
    gt = _as_gt(annotation)
    I = len(set(gt.getImgIds()))
    cells = lamr_cells(I, day_frames)
    mult = resample_multiplicities_stratified(cells[1:], replicates, seed) if stratified else resample_multiplicities(I, replicates, seed)
    files = [("a", results_a)] + ([("b", results_b)] if results_b is not None else [])
    out = {"replicates": replicates, "seed": seed, "confidence": confidence, "setups": [int(s) for s in setups], "subsets": list(SUBSETS),
           "images": I, "day_frames": int(cells[1, 1]), "stratified": bool(stratified), "fix_row_index": bool(fix_row_index),
           "resampling": "numpy.random.default_rng(seed).multinomial" + (" per stratum (day, night)" if stratified else "") +
                         "; row 0 = every image once"}
    reps = {}
    for name, res in files:
        dt = _as_dt(gt, res)
        out[name] = {"setups": {}, "mixed_score_ties": {}}
        for s in out["setups"]:
            m = export_lamr_matches(gt, dt, s, fix_row_index)
            if name == "b":
                check_same_images(reps["a", s][0]["img_ids"], m["img_ids"], "results_a", "results_b")
            stats = lamr_statistics(lamr_bootstrap(m, mult, cells, device), m)
            points = [point_estimates(sub, s) for sub in subset_evaluators(m, cells)]
            reps[name, s] = (m, stats, points)
            fppi = [float(x) for x in m["evaluator"].params.fppiThrs]
            out["fppi"] = fppi
            out[name]["mixed_score_ties"][str(s)] = mixed_score_ties(m)
            out[name]["setups"][str(s)] = {
                sub: {"MR": dict(point=pt[0], **_interval(stats["MR"][1:, c], pt[0], confidence)),
                      "miss_rate_at_fppi": [dict(point=float(pt[1][r]), **_interval(stats["miss_rates"][1:, c, r], pt[1][r], confidence))
                                            for r in range(len(fppi))],
                      "recall": dict(point=pt[2], **_interval(stats["recall_all"][1:, c], pt[2], confidence))}
                for c, (sub, pt) in enumerate(zip(SUBSETS, points))}
    if results_b is not None:
        out["paired"] = {"setups": {}}
        for s in out["setups"]:
            (_, sa, pa), (_, sb, pb) = reps["a", s], reps["b", s]
            diff = lambda xa, xb, a, b: paired(xa[1:], xb[1:], a, b, _undefined, confidence)      # noqa: E731
            out["paired"]["setups"][str(s)] = {
                sub: {"MR": diff(sa["MR"][:, c], sb["MR"][:, c], pa[c][0], pb[c][0]),
                      "miss_rate_at_fppi": [diff(sa["miss_rates"][:, c, r], sb["miss_rates"][:, c, r], pa[c][1][r], pb[c][1][r])
                                            for r in range(len(out["fppi"]))],
                      "recall": diff(sa["recall_all"][:, c], sb["recall_all"][:, c], pa[c][2], pb[c][2])}
                for c, sub in enumerate(SUBSETS)}
    return out
