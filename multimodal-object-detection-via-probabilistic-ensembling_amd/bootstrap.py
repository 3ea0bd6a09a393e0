"""Paired bootstrap of the COCO statistics over images.

Matching is per image, so it is done once by the host evaluator (pe_cocoeval_bbox_matches); a replicate that holds image i m_i times
only re-runs accumulate, as a weighted scan over the exported list on the GPU (pe_ap_bootstrap, csrc/ap_bootstrap.hip).  A replicate
equals COCOevalBBox on the dataset with m_i adjacent copies of image i bit for bit (section 27 has the argument and its one
condition: detections of one class that tie in score inside one image must agree in their tp / fp flags).

    resample_multiplicities(n_images, replicates, seed)   the resamples, row 0 = the dataset itself
    export_matches(gt_json, results)                       the lists, on the host
    mixed_score_ties(matches)                              how often that condition is not met (reported, 0 on the tests' case)
    ap_bootstrap(matches, mult, device)                    psum / recall / valid (and the full precision table on request) per replicate
    statistics(run, matches)                               the 12 summarize() statistics and AP per class, per replicate
    bootstrap_ap(gt_json, results_a, results_b=None, ...)  point estimates, percentile intervals, standard errors, paired differences
    paired(xa, xb, pa, pb, undefined, confidence)          the paired-difference record (lamr_bootstrap.py, section 28, reports with it too)
"""
import numpy as np
import torch

from . import _lib
from .evaluation import COCOevalBBox

STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
MULT_MAX = 255          # pe_ap_bootstrap takes the multiplicities as uint8
MAX_T, MAX_R, MAX_IMAGES = 16, 128, 32768
# the (area range, maxDets index) cells summarize() reads, per category: the position in this tuple is the cell's index inside its category
SUMMARY_CELLS = ((0, 2), (1, 2), (2, 2), (3, 2), (0, 0), (0, 1))
# statistic -> (its cell above, "p" precision / "r" recall, the IoU threshold it is taken at or None for all)
_STAT_CELLS = ((0, "p", None), (0, "p", .5), (0, "p", .75), (1, "p", None), (2, "p", None), (3, "p", None),
               (4, "r", None), (5, "r", None), (0, "r", None), (1, "r", None), (2, "r", None), (3, "r", None))


def resample_multiplicities(n_images, replicates, seed):
    """int64 [replicates, n_images]: row 0 is all ones (the dataset itself: the point estimate), every other row one multinomial
    draw of n_images images with replacement from np.random.default_rng(seed).  Same arguments, same bytes."""
    if n_images < 1 or replicates < 1:
        raise ValueError(f"resample_multiplicities: n_images {n_images} and replicates {replicates} must be >= 1")
    mult = np.ones((replicates, n_images), dtype=np.int64)
    if replicates > 1:
        rng = np.random.default_rng(seed)
        mult[1:] = rng.multinomial(n_images, np.full(n_images, 1.0 / n_images), size=replicates - 1)
    return mult


def export_matches(gt_json, results, num_threads=0):
    """The per-category sorted detection lists with their match flags and the per-image ground-truth counts (include/proben_hip.h,
    pe_cocoeval_bbox_matches), as host arrays, with the evaluator whose parameters they were made under."""
    ev = COCOevalBBox(gt_json, results, num_threads=num_threads)
    args = ev._native_arrays()
    n_dt, I, K, A = args[11], len(ev.img_ids), len(ev.cat_ids), len(ev.area_rng)
    out = {"list_off": np.zeros(K + 1, dtype=np.int64), "list_img": np.zeros(n_dt, dtype=np.int32),
           "list_rank": np.zeros(n_dt, dtype=np.uint8), "list_flags": np.zeros((A, n_dt), dtype=np.uint32),
           "npig": np.zeros((K, A, I), dtype=np.int32)}
    # an empty array travels as NULL; the entry point wants its offsets and counts even then
    if K == 0 or I == 0:
        raise ValueError("export_matches: the ground truth has no images or no categories")
    ev._native_call("pe_cocoeval_bbox_matches", args + [out[k] for k in ("list_off", "list_img", "list_rank", "list_flags", "npig")])
    out["evaluator"] = ev
    return out


def mixed_score_ties(matches):
    """The number of neighbours in the lists that belong to one image, tie in score (NaN ties with NaN) and differ, at some threshold
    and area range, in what they count as (tp / fp / nothing).  Section 27's one condition: where this is 0, every replicate is the
    evaluator on the duplicated dataset bit for bit; a pair counted here is weighed entry by entry where a duplicated image would
    repeat the pair as a whole."""
    ev = matches["evaluator"]
    args = ev._native_arrays()
    dt_img, dt_cat, dt_score, T = args[7], args[8], args[10], len(ev.iou_thrs)
    cap, n = ev.max_dets[-1], 0
    mask = np.uint32((1 << T) - 1)
    for k in range(len(ev.cat_ids)):
        rows = np.flatnonzero(dt_cat == k)
        rows = rows[np.lexsort((-dt_score[rows], dt_img[rows]))]          # stable: per image by descending score, NaN last, file order kept
        img = dt_img[rows]
        rank = np.arange(len(rows)) - np.searchsorted(img, img, side="left")
        score = np.full((len(ev.img_ids), cap), np.nan)
        keep = rank < cap
        score[img[keep], rank[keep]] = dt_score[rows][keep]
        sl = slice(int(matches["list_off"][k]), int(matches["list_off"][k + 1]))
        li, s = matches["list_img"][sl], score[matches["list_img"][sl], matches["list_rank"][sl]]
        f = matches["list_flags"][:, sl]
        tp, fp = f & ~(f >> 16) & mask, ~f & ~(f >> 16) & mask
        tie = (li[1:] == li[:-1]) & ((s[1:] == s[:-1]) | (np.isnan(s[1:]) & np.isnan(s[:-1])))
        n += int(np.count_nonzero(tie & ((tp[:, 1:] != tp[:, :-1]) | (fp[:, 1:] != fp[:, :-1])).any(0)))
    return n


def summary_cells(matches):
    """int32 [K * 6, 3] = (category, area range, maxDet): what summarize() reads, category-major in SUMMARY_CELLS order."""
    ev = matches["evaluator"]
    return np.array([[k, a, ev.max_dets[m]] for k in range(len(ev.cat_ids)) for a, m in SUMMARY_CELLS], dtype=np.int32).reshape(-1, 3)


def _narrow(mult, n_images):
    """The multiplicities as the kernel stores them; the range is checked here, before anything touches the GPU."""
    mult = np.asarray(mult)
    if mult.ndim != 2 or mult.shape[1] != n_images:
        raise ValueError(f"multiplicities of shape {mult.shape}: expected [replicates, {n_images}]")
    if not np.issubdtype(mult.dtype, np.integer):
        raise ValueError(f"multiplicities must be integers, got {mult.dtype}")
    if mult.size and (mult.min() < 0 or mult.max() > MULT_MAX):
        raise ValueError(f"multiplicities must lie in [0, {MULT_MAX}] (they are stored as uint8): got [{mult.min()}, {mult.max()}]")
    return np.ascontiguousarray(mult, dtype=np.uint8)


def launch_ap_bootstrap(lists, mult, sizes, rec_thrs, cells, device="cuda", full_table=False):
    """One launch of pe_ap_bootstrap over host lists ("list_off", "list_img", "list_rank", "list_flags" [A, n], "npig" [K, A, I]) with
    sizes = (I, K, A, T): ap_bootstrap's launch, which tide.price shares with its own planes on the area-range axis."""
    I, K, A, T = sizes
    R = len(rec_thrs)
    m8 = _narrow(mult, I)
    cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
    B, C = m8.shape[0], cells.shape[0]
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)      # noqa: E731
    d = {k: up(lists[k]) for k in ("list_off", "list_img", "list_rank", "list_flags", "npig")}
    d_mult, d_cells, d_thr = up(m8), up(cells), up(np.ascontiguousarray(rec_thrs, dtype=np.float64))
    _lib.require_cuda(d_mult)
    psum = torch.empty((B, C, T), dtype=torch.float64, device=dev)
    recall = torch.empty((B, C, T), dtype=torch.float64, device=dev)
    valid = torch.empty((B, C), dtype=torch.int32, device=dev)
    prec = torch.empty((B, C, T, R), dtype=torch.float64, device=dev) if full_table else None
    ptr = lambda t: _lib.ptr(t) if t is not None and t.numel() else None      # noqa: E731
    with torch.cuda.device(dev):
        st = _lib.lib().pe_ap_bootstrap(ptr(d["list_off"]), ptr(d["list_img"]), ptr(d["list_rank"]), ptr(d["list_flags"]),
                                        int(lists["list_img"].shape[0]), ptr(d["npig"]), ptr(d_mult), B, I, K, A, T, ptr(d_thr), R,
                                        ptr(d_cells), C, ptr(psum), ptr(recall), ptr(valid), ptr(prec), _lib.stream())
    _lib.check(st, "pe_ap_bootstrap")
    out = {"psum": psum.cpu().numpy(), "recall": recall.cpu().numpy(), "valid": valid.cpu().numpy(), "cells": cells}
    if (out["valid"] < 0).any():
        raise ValueError("pe_ap_bootstrap: a cell names a category or an area range outside the lists")
    if full_table:
        out["precision"] = prec.cpu().numpy()
    return out


def ap_bootstrap(matches, mult, device="cuda", cells=None, full_table=False):
    """One launch of pe_ap_bootstrap over mult [B, I].  Returns host arrays: psum [B, C, T] (the sum of the R interpolated precisions),
    recall [B, C, T], valid [B, C] and, with full_table, precision [B, C, T, R]; "cells" [C, 3] is what was evaluated."""
    ev = matches["evaluator"]
    sizes = (len(ev.img_ids), len(ev.cat_ids), len(ev.area_rng), len(ev.iou_thrs))
    return launch_ap_bootstrap(matches, mult, sizes, ev.rec_thrs, summary_cells(matches) if cells is None else cells, device, full_table)


def statistics(run, matches):
    """(stats [B, 12], class_ap [B, K]) from ap_bootstrap's output over summary_cells: COCOevalBBox._summ's mean over the entries
    that are not -1 (a statistic with no such entry is -1; a category without ground truth has AP nan, as FLIREvaluator prints it)."""
    ev = matches["evaluator"]
    K, T, R = len(ev.cat_ids), len(ev.iou_thrs), len(ev.rec_thrs)
    B, S = run["psum"].shape[0], len(SUMMARY_CELLS)
    psum, recall, valid = run["psum"].reshape(B, K, S, T), run["recall"].reshape(B, K, S, T), run["valid"].reshape(B, K, S) > 0
    stats = np.full((B, len(_STAT_CELLS)), -1.0)
    for s, (c, kind, iou) in enumerate(_STAT_CELLS):
        ts = np.arange(T) if iou is None else np.where(np.isclose(ev.iou_thrs, iou))[0]
        v = valid[:, :, c]                                              # [B, K]
        x = (psum if kind == "p" else recall)[:, :, c][:, :, ts]        # [B, K, |ts|]
        n = v.sum(1) * len(ts) * (R if kind == "p" else 1)
        tot = np.where(v[:, :, None], x, 0.0).sum((1, 2))
        stats[:, s] = np.where(n > 0, tot / np.maximum(n, 1), -1.0)
    class_ap = np.where(valid[:, :, 0], psum[:, :, 0].sum(2) / (T * R), np.nan)
    return stats, class_ap


def _interval(x, point, confidence):
    """Percentile interval and standard error of the replicates x (the undefined ones, -1 or nan, left out)."""
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x) & (x > -1)] if point is not None else x[np.isfinite(x)]
    if x.size == 0:
        return {"lo": float("nan"), "hi": float("nan"), "se": float("nan"), "replicates": 0}
    a = (1.0 - confidence) / 2.0
    return {"lo": float(np.quantile(x, a)), "hi": float(np.quantile(x, 1.0 - a)), "se": float(np.std(x, ddof=1)) if x.size > 1 else float("nan"),
            "replicates": int(x.size)}


def paired(xa, xb, pa, pb, undefined, confidence):
    """The paired-difference record of two files' replicates under the same resamples: b - a with its percentile interval, standard
    error and the two-sided bootstrap p-value 2 min(P(d* <= 0), P(d* >= 0)), over the replicates both files have defined."""
    ok = ~(undefined(xa) | undefined(xb))
    d = (xb - xa)[ok]
    rec = dict(point=float(pb - pa), **_interval(d, None, confidence))
    rec["p"] = float(min(1.0, 2.0 * min(np.mean(d <= 0), np.mean(d >= 0)))) if d.size else float("nan")
    return rec


def check_results(gt_json, results, name):
    ids = {im["id"] for im in gt_json["images"]}
    bad = [r["image_id"] for r in results if r["image_id"] not in ids]
    if bad:
        raise ValueError(f"{name}: {len(bad)} detections on images the ground truth does not have (image id {bad[0]} is one)")


def check_same_images(ids_a, ids_b, name_a="A", name_b="B"):
    """The paired bootstrap resamples ONE image list: two prediction files must list the same images."""
    a, b = set(ids_a), set(ids_b)
    if a != b:
        only = sorted(a ^ b, key=str)
        raise ValueError(f"{name_a} and {name_b} do not list the same images ({len(a)} vs {len(b)}; image id {only[0]} is in one only): "
                         "a paired bootstrap needs both files over one image set")


def bootstrap_ap(gt_json, results_a, results_b=None, replicates=2000, seed=0, confidence=0.95, device="cuda"):
    """Percentile-bootstrap intervals of the 12 COCO statistics and of AP per class for results_a (and results_b, under the SAME
    resamples, with the paired difference b - a, its interval and the two-sided bootstrap p-value 2 min(P(d* <= 0), P(d* >= 0))).
    The point estimates are COCOevalBBox's own; the replicates are rows 1.. of resample_multiplicities (row 0, the dataset itself,
    is evaluated with them and is not part of the distribution)."""
    if not 0.0 < confidence < 1.0:
        raise ValueError(f"confidence {confidence} is not in (0, 1)")
    if replicates < 2:
        raise ValueError(f"replicates {replicates}: the resamples are rows 1.. (row 0 is the dataset itself), so at least 2")
    files = [("a", results_a)] + ([("b", results_b)] if results_b is not None else [])
    for name, res in files:
        check_results(gt_json, res, "results_" + name)
    mult = resample_multiplicities(len({im["id"] for im in gt_json["images"]}), replicates, seed)
    out = {"replicates": replicates, "seed": seed, "confidence": confidence, "statistics": list(STAT_NAMES),
           "resampling": "numpy.random.default_rng(seed).multinomial; row 0 = every image once"}
    reps = {}
    for name, res in files:
        m = export_matches(gt_json, res)
        ev = m["evaluator"]
        ev.evaluate()
        ev.accumulate()
        point = ev.summarize(printer=None)
        p = ev.eval["precision"][:, :, :, 0, -1]
        point_cls = [float(np.mean(p[:, :, k][p[:, :, k] > -1])) if (p[:, :, k] > -1).any() else float("nan") for k in range(p.shape[2])]
        stats, cls = statistics(ap_bootstrap(m, mult, device), m)
        reps[name] = (stats, cls, point, point_cls)
        out[name] = {"stats": {s: dict(point=float(point[i]), **_interval(stats[1:, i], point[i], confidence)) for i, s in enumerate(STAT_NAMES)},
                     "class_ap": {str(c): dict(point=point_cls[k], **_interval(cls[1:, k], point_cls[k], confidence))
                                  for k, c in enumerate(ev.cat_ids)},
                     "mixed_score_ties": mixed_score_ties(m)}
        out["categories"] = list(ev.cat_ids)
    if results_b is not None:
        (sa, ca, pa, pca), (sb, cb, pb, pcb) = reps["a"], reps["b"]
        out["paired"] = {"stats": {s: paired(sa[1:, i], sb[1:, i], pa[i], pb[i], lambda x: x <= -1, confidence) for i, s in enumerate(STAT_NAMES)},
                         "class_ap": {str(c): paired(ca[1:, k], cb[1:, k], pca[k], pcb[k], np.isnan, confidence)
                                      for k, c in enumerate(out["categories"])}}
    return out
