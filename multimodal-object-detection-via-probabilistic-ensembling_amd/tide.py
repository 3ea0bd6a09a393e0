"""TIDE error decomposition of AP50 with paired bootstrap intervals.

Every false positive and every missed ground truth gets one error type (Bolya, Foley, Hays, Hoffman, "TIDE: A General Toolbox for
Identifying Object Detection Errors", ECCV 2020, restated for this evaluator), and each type is priced by the AP50 gained if that type
alone were repaired.  The typing is per image and runs once, on the GPU (pe_tide_classify, csrc/tide.hip); a repaired variant is another
set of flags and ground-truth counts over the evaluator's own lists, so all nine variants go through pe_ap_bootstrap (section 27) as
nine planes of its area-range axis, under the same resamples bootstrap_ap uses.

    classify_arrays(...)                              one launch of pe_tide_classify over flat arrays
    layout(matches) / assemble(matches, lay, raw)     the kernel's inputs from the exported lists / classify()'s record from its outputs
    classify(gt_json, results, background_iou)        types, partners and claims per list entry, ground-truth bits, the counts
    variant_lists(cl)                                 the nine variants as list_flags [9][n] and npig [K][9][I] of one set of lists
    price(lists, mult)                                AP50 of every variant under every replicate, one launch
    tide(gt_json, results_a, results_b=None, ...)     the report: counts, dAP per repair with intervals, paired differences
"""
import numpy as np
import torch

from . import _lib
from .bootstrap import (_interval, check_results, export_matches, launch_ap_bootstrap, mixed_score_ties, paired,
                        resample_multiplicities)

TYPES = ("TP", "Cls", "Loc", "Both", "Dupe", "Bkg", "Ignored")          # pe_tide_classify's out_type codes (PE_TIDE_*)
TP, CLS, LOC, BOTH, DUPE, BKG, IGNORED = range(7)
VARIANTS = ("base", "Cls", "Loc", "Both", "Dupe", "Bkg", "Miss", "FP", "FN")      # the repair of variant v >= 1; 1 - 5 are the type codes
GT_MATCHED, GT_LOC, GT_CLS, GT_MISSED = 1, 2, 4, 8                       # out_gt's bits
MAX_DETS, MAX_GT, MAX_CLASSES = 8000, 1024, 80                           # per image / per launch (include/proben_hip.h)


def _check_thresholds(t_f, t_b):
    if not 0.0 <= t_b < t_f <= 1.0:
        raise ValueError(f"background_iou {t_b} and the match threshold {t_f} are not in 0 <= background_iou < threshold <= 1")


def classify_arrays(det_box, det_cat, det_off, gt_box, gt_cat, gt_crowd, gt_off, num_classes, t_f=0.5, t_b=0.1, device="cuda"):
    """One launch of pe_tide_classify.  Host arrays: det_box f64 [M, 4] xywh and det_cat [M] in the total order, det_off [B + 1];
    gt_box f64 [G, 4], gt_cat [G], gt_crowd [G] in annotation order, gt_off [B + 1].  Returns host int32 arrays "match", "type",
    "partner", "claim" [M] (ground-truth indices local to the image) and "gt" [G] (bits)."""
    _check_thresholds(t_f, t_b)
    det_off, gt_off = np.ascontiguousarray(det_off, dtype=np.int32), np.ascontiguousarray(gt_off, dtype=np.int32)
    if det_off.ndim != 1 or det_off.shape != gt_off.shape or det_off.size < 1:
        raise ValueError(f"det_off {det_off.shape} and gt_off {gt_off.shape} must both be [images + 1]")
    B, M, G = det_off.size - 1, int(np.asarray(det_cat).shape[0]), int(np.asarray(gt_cat).shape[0])
    dev = torch.device(device)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    d_box, d_cat = up(np.asarray(det_box, dtype=np.float64).reshape(M, 4), np.float64), up(det_cat, np.int32)
    g_box, g_cat, g_crowd = up(np.asarray(gt_box, dtype=np.float64).reshape(G, 4), np.float64), up(gt_cat, np.int32), up(gt_crowd, np.uint8)
    ws = torch.empty(2 * (B + 1), dtype=torch.int32, device=dev)
    _lib.require_cuda(ws)
    out = {k: torch.empty(M, dtype=torch.int32, device=dev) for k in ("match", "type", "partner", "claim")}
    out["gt"] = torch.empty(G, dtype=torch.int32, device=dev)
    ptr = lambda t: _lib.ptr(t) if t.numel() else None      # noqa: E731
    with torch.cuda.device(dev):
        st = _lib.lib().pe_tide_classify(ptr(d_box), ptr(d_cat), det_off.ctypes.data, ptr(g_box), ptr(g_cat), ptr(g_crowd), gt_off.ctypes.data,
                                         B, int(num_classes), M, G, float(t_f), float(t_b), ptr(ws), ptr(out["match"]), ptr(out["type"]),
                                         ptr(out["partner"]), ptr(out["claim"]), ptr(out["gt"]), _lib.stream())
    _lib.check(st, "pe_tide_classify")
    return {k: v.cpu().numpy() for k, v in out.items()}


def entry_rows(matches):
    """int64 [n]: the row of the evaluator's detection arrays (COCOevalBBox._native_arrays) behind every entry of the exported lists."""
    ev = matches["evaluator"]
    args = ev._native_arrays()
    dt_img, dt_cat, dt_score = args[7], args[8], args[10]
    cap, I = ev.max_dets[-1], len(ev.img_ids)
    row = np.zeros(matches["list_img"].shape[0], dtype=np.int64)
    for k in range(len(ev.cat_ids)):
        rows = np.flatnonzero(dt_cat == k)
        rows = rows[np.lexsort((-dt_score[rows], dt_img[rows]))]          # stable: per image by descending score, NaN last, file order kept
        img = dt_img[rows]
        rank = np.arange(len(rows)) - np.searchsorted(img, img, side="left")
        table = np.full((I, cap), -1, dtype=np.int64)
        keep = rank < cap
        table[img[keep], rank[keep]] = rows[keep]
        sl = slice(int(matches["list_off"][k]), int(matches["list_off"][k + 1]))
        row[sl] = table[matches["list_img"][sl], matches["list_rank"][sl]]
    assert (row >= 0).all()
    return row


def layout(matches):
    """The kernel's inputs from the exported lists: per image the entries in the total order (descending score, NaN last, ties by
    category index, then by the evaluator's rank) and the ground truths in annotation order.  ValueError where the rule's area range
    "all" would ignore a box (an area outside the evaluator's first range): the kernel knows crowd boxes only."""
    ev = matches["evaluator"]
    args = ev._native_arrays()
    gt_img, gt_cat, gt_box, gt_area, gt_crowd, dt_box, dt_score = args[0], args[1], args[2], args[3], args[4], args[9], args[10]
    I, K = len(ev.img_ids), len(ev.cat_ids)
    lo, hi = ev.area_rng[0]
    row = entry_rows(matches)
    cat = np.repeat(np.arange(K, dtype=np.int32), np.diff(matches["list_off"]))
    img, rank, score, box = matches["list_img"], matches["list_rank"].astype(np.int32), dt_score[row], dt_box[row].reshape(-1, 4)
    d_area = box[:, 2] * box[:, 3]
    if ((gt_crowd == 0) & ((gt_area < lo) | (gt_area > hi))).any() or ((d_area < lo) | (d_area > hi)).any():
        raise ValueError(f"tide: a ground-truth or detection area lies outside the evaluator's range [{lo}, {hi}]: unsupported")
    order = np.lexsort((rank, cat, -score, img))          # entry indices, image-major, in the total order
    g_order = np.argsort(gt_img, kind="stable")
    return {"order": order, "det_box": box[order], "det_cat": cat[order], "det_off": np.searchsorted(img[order], np.arange(I + 1)),
            "g_order": g_order, "gt_box": gt_box[g_order].reshape(-1, 4), "gt_cat": gt_cat[g_order], "gt_crowd": gt_crowd[g_order],
            "gt_off": np.searchsorted(gt_img[g_order], np.arange(I + 1)), "entry_cat": cat, "entry_score": score, "gt_img": gt_img,
            "gt_cat_rows": gt_cat, "gt_crowd_rows": gt_crowd}


def classify(gt_json, results, background_iou=0.1, device="cuda", matches=None):
    """The TIDE types of one result list.  Per entry of the exported lists (matches = bootstrap.export_matches(gt_json, results), made
    here when it is not given): "type" (TYPES), "match" and "partner" (rows of the evaluator's ground-truth arrays, -1 for none),
    "partner_cat" (category index or -1), "claim"; per ground-truth row "gt" (GT_* bits).  "counts": per type and class [7, K],
    "missed" [K], "unmatched" [K] (every unmatched non-crowd ground truth) and the K x K "confusion" of the Cls errors (predicted
    class by partner class)."""
    check_results(gt_json, results, "results")
    m = export_matches(gt_json, results) if matches is None else matches
    ev = m["evaluator"]
    t_f, K = float(ev.iou_thrs[0]), len(ev.cat_ids)
    _check_thresholds(t_f, background_iou)
    lay = layout(m)
    raw = classify_arrays(lay["det_box"], lay["det_cat"], lay["det_off"], lay["gt_box"], lay["gt_cat"], lay["gt_crowd"], lay["gt_off"], K,
                          t_f, background_iou, device)
    return assemble(m, lay, raw, background_iou)


def assemble(m, lay, raw, background_iou=0.1):
    """classify()'s record from the kernel's arrays `raw` (image-major, indices local to the image) over layout(m)."""
    ev = m["evaluator"]
    t_f, K = float(ev.iou_thrs[0]), len(ev.cat_ids)
    n, order = len(lay["order"]), lay["order"]
    base = np.repeat(lay["gt_off"][:-1], np.diff(lay["det_off"]))          # image-local -> position among the sorted ground truths
    G = len(lay["g_order"])

    def to_row(x):          # image-local index -> row of the evaluator's ground-truth arrays
        return np.where(x >= 0, lay["g_order"][np.clip(x + base, 0, G - 1)], -1) if G else np.full(len(x), -1, dtype=np.int64)
    out = {"matches": m, "layout": lay, "background_iou": float(background_iou), "threshold": t_f}
    for key, val in (("type", raw["type"]), ("claim", raw["claim"]), ("match", to_row(raw["match"])), ("partner", to_row(raw["partner"]))):
        full = np.zeros(n, dtype=np.int64)
        full[order] = val
        out[key] = full
    out["position"] = np.zeros(n, dtype=np.int64)
    out["position"][order] = np.arange(n)                                   # the entry's place in the image-major total order
    out["partner_cat"] = np.where(out["partner"] >= 0, lay["gt_cat_rows"][np.clip(out["partner"], 0, None)], -1) if G else np.full(n, -1, dtype=np.int64)
    gt = np.zeros(len(lay["g_order"]), dtype=np.int64)
    gt[lay["g_order"]] = raw["gt"]
    out["gt"] = gt
    counts = np.zeros((len(TYPES), K), dtype=np.int64)
    np.add.at(counts, (out["type"], lay["entry_cat"]), 1)
    conf = np.zeros((K, K), dtype=np.int64)
    cls = out["type"] == CLS
    np.add.at(conf, (lay["entry_cat"][cls], out["partner_cat"][cls]), 1)
    regular = lay["gt_crowd_rows"] == 0
    out["counts"] = {"types": counts, "confusion": conf,
                     "missed": np.bincount(lay["gt_cat_rows"][(gt & GT_MISSED) != 0], minlength=K),
                     "unmatched": np.bincount(lay["gt_cat_rows"][regular & ((gt & GT_MATCHED) == 0)], minlength=K)}
    return out


def variant_lists(cl):
    """The nine variants of classify()'s output as the planes of ONE set of lists: "list_off" [K + 1], "list_img", "list_rank" [n'],
    "list_flags" u32 [9][n'] (bit 0 matched, bit 16 ignored: T = 1) and "npig" i32 [K][9][I], the variant on pe_ap_bootstrap's area-range
    axis.  The lists are the evaluator's with every claimed Cls error entered a second time, in the list of its partner's category at
    its own score (behind the list's own entries of that score, then in image order) with rank 0: that copy counts in variant 1 only.
    "source" [n'] is the entry of the exported lists behind each row and "moved" [n'] marks the copies."""
    m, lay = cl["matches"], cl["layout"]
    ev = m["evaluator"]
    K, I = len(ev.cat_ids), len(ev.img_ids)
    typ, claim, score = cl["type"], cl["claim"] != 0, lay["entry_score"]
    matched, ignored = (typ == TP) | (typ == IGNORED), typ == IGNORED
    fp = (typ >= CLS) & (typ <= BKG)
    mt, ig = np.repeat(matched[None], len(VARIANTS), 0), np.repeat(ignored[None], len(VARIANTS), 0)
    ig[1] |= typ == CLS
    mt[2] |= (typ == LOC) & claim
    ig[2] |= (typ == LOC) & ~claim
    for v in (BOTH, DUPE, BKG):
        ig[v] |= typ == v
    ig[7] |= fp
    flags = mt.astype(np.uint32) | (ig.astype(np.uint32) << 16)
    moved_flags = np.full(len(VARIANTS), 1 << 16, dtype=np.uint32)
    moved_flags[1] = 1
    movers = np.flatnonzero((typ == CLS) & claim)
    movers = movers[np.argsort(cl["position"][movers], kind="stable")]      # image order, then the total order inside the image
    off, source, is_moved = [0], [], []
    for k in range(K):
        own = np.arange(int(m["list_off"][k]), int(m["list_off"][k + 1]))
        mv = movers[cl["partner_cat"][movers] == k]
        both = np.concatenate([own, mv])
        o = np.argsort(-score[both], kind="stable")                         # descending, NaN last, ties: own entries first, then the copies
        source.append(both[o])
        is_moved.append((np.arange(len(both)) >= len(own))[o])
        off.append(off[-1] + len(both))
    source, is_moved = np.concatenate(source).astype(np.int64), np.concatenate(is_moved).astype(bool)
    list_flags = np.where(is_moved[None], moved_flags[:, None], flags[:, source]).astype(np.uint32)
    npig = np.repeat(m["npig"][:, :1, :], len(VARIANTS), 1).astype(np.int32)
    gt_cat, gt_img, gt = lay["gt_cat_rows"], lay["gt_img"], cl["gt"]
    missed = (gt & GT_MISSED) != 0
    unmatched = (lay["gt_crowd_rows"] == 0) & ((gt & GT_MATCHED) == 0)
    np.subtract.at(npig[:, 6, :], (gt_cat[missed], gt_img[missed]), 1)
    np.subtract.at(npig[:, 8, :], (gt_cat[unmatched], gt_img[unmatched]), 1)
    return {"list_off": np.array(off, dtype=np.int64), "list_img": np.ascontiguousarray(m["list_img"][source], dtype=np.int32),
            "list_rank": np.where(is_moved, 0, m["list_rank"][source]).astype(np.uint8), "list_flags": np.ascontiguousarray(list_flags),
            "npig": np.ascontiguousarray(npig), "source": source, "moved": is_moved, "sizes": (I, K, len(VARIANTS), 1),
            "rec_thrs": np.ascontiguousarray(ev.rec_thrs, dtype=np.float64), "max_det": int(ev.max_dets[-1])}


def price(lists, mult, device="cuda", full_table=False):
    """AP50 of every variant under every replicate of mult [B, I], by one launch of pe_ap_bootstrap over K x 9 cells.  "ap" [B, 9]: the
    mean over the categories whose cell is valid in that variant of psum / R, the cells added in category order, -1 where no category
    is valid (COCOevalBBox._summ's convention); "psum" and "valid" [B, K, 9]; with full_table "precision" [B, K, 9, R]."""
    I, K, V, _ = lists["sizes"]
    R = len(lists["rec_thrs"])
    cells = np.array([[k, v, lists["max_det"]] for k in range(K) for v in range(V)], dtype=np.int32)
    run = launch_ap_bootstrap(lists, mult, lists["sizes"], lists["rec_thrs"], cells, device, full_table)
    B = run["psum"].shape[0]
    psum, valid = run["psum"].reshape(B, K, V), run["valid"].reshape(B, K, V) > 0
    tot, n = np.zeros((B, V)), np.zeros((B, V), dtype=np.int64)
    for k in range(K):
        tot = tot + np.where(valid[:, k], psum[:, k] / R, 0.0)
        n += valid[:, k]
    out = {"ap": np.where(n > 0, tot / np.maximum(n, 1), -1.0), "psum": psum, "valid": valid}
    if full_table:
        out["precision"] = run["precision"].reshape(B, K, V, R)
    return out


def _gains(ap):
    """dAP [B, 8] = AP50 of repair v minus the base's; nan where either is undefined (-1)."""
    return np.where((ap[:, 1:] > -1) & (ap[:, :1] > -1), ap[:, 1:] - ap[:, :1], np.nan)


def tide(gt_json, results_a, results_b=None, replicates=2000, seed=0, confidence=0.95, background_iou=0.1, device="cuda"):
    """The TIDE report of results_a (and results_b under the SAME resamples, with the paired difference b - a of every dAP, its interval
    and the two-sided bootstrap p-value).  Per file: "AP50", per repair of VARIANTS[1:] its "count" (errors of that type; for Miss the
    missed, for FN the unmatched ground truths; for FP all false positives) and "dAP" = AP50 with that type alone repaired minus AP50,
    each with point estimate (row 0 of resample_multiplicities: the dataset itself), percentile interval and standard error over rows
    1..; the counts per type and class, the confusion counts of the Cls errors and mixed_score_ties of the exported lists."""
    if not 0.0 < confidence < 1.0:
        raise ValueError(f"confidence {confidence} is not in (0, 1)")
    if replicates < 2:
        raise ValueError(f"replicates {replicates}: the resamples are rows 1.. (row 0 is the dataset itself), so at least 2")
    files = [("a", results_a)] + ([("b", results_b)] if results_b is not None else [])
    for name, res in files:
        check_results(gt_json, res, "results_" + name)
    mult = resample_multiplicities(len({im["id"] for im in gt_json["images"]}), replicates, seed)
    out = {"replicates": replicates, "seed": seed, "confidence": confidence, "background_iou": float(background_iou),
           "repairs": list(VARIANTS[1:]), "types": list(TYPES), "resampling": "numpy.random.default_rng(seed).multinomial; row 0 = every image once"}
    reps = {}
    for name, res in files:
        cl = classify(gt_json, res, background_iou, device)
        ev = cl["matches"]["evaluator"]
        run = price(variant_lists(cl), mult, device)
        ap, gain = run["ap"], _gains(run["ap"])
        c = cl["counts"]
        count = {**{VARIANTS[v]: int(c["types"][v].sum()) for v in range(1, 6)}, "Miss": int(c["missed"].sum()),
                 "FP": int(c["types"][CLS:BKG + 1].sum()), "FN": int(c["unmatched"].sum())}
        reps[name] = gain
        out["threshold"], out["categories"] = cl["threshold"], list(ev.cat_ids)
        out[name] = {"AP50": dict(point=float(ap[0, 0]), **_interval(ap[1:, 0], ap[0, 0], confidence)),
                     "repairs": {r: dict(count=count[r], point=float(gain[0, i]), **_interval(gain[1:, i], None, confidence))
                                 for i, r in enumerate(VARIANTS[1:])},
                     "counts": {"types": {TYPES[t]: c["types"][t].tolist() for t in range(len(TYPES))}, "missed": c["missed"].tolist(),
                                "unmatched": c["unmatched"].tolist(), "confusion": c["confusion"].tolist()},
                     "mixed_score_ties": mixed_score_ties(cl["matches"])}
    if results_b is not None:
        ga, gb = reps["a"], reps["b"]
        out["paired"] = {r: paired(ga[1:, i], gb[1:, i], ga[0, i], gb[0, i], np.isnan, confidence) for i, r in enumerate(VARIANTS[1:])}
    return out
