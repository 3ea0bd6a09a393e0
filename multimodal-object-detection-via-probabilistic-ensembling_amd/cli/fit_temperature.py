"""Fit one softmax temperature per detector from its validation predictions (calibration.py).

    python -m proben_amd.cli.fit_temperature --dataset_path DATA/FLIR/val \\
        --predictions out/val_thermal_only_predictions.json out/val_early_fusion_predictions.json \\
        [--holdout 0.5] --out calibration.json

Every detection of a prediction file is labelled from the ground truth (calibration.match_labels: the class of the box it overlaps
most at IoU >= 0.5, else background), and T minimises the negative log-likelihood of those labels under softmax(class_logits / T)
(calibration.fit_temperature).  --holdout f: the first fraction f of the images, in dataset order, is fitted; the rest is left for
evaluation.  The fitted image ids go into the file, and demo_probEn warns when it evaluates on them.  The detector's name is the
<name> of val_<name>_predictions.json.  Prints, per detector, T and the NLL before (T = 1) and after.
--with-prior also writes "class_prior": the frequencies of the labels 0..K (background last) over the fitted rows of all the files
together, with one added to every count so that a class no fitted row carries keeps a prior > 0 ("class_prior_counts" holds the raw
counts).  `demo_probEn --score_fusion probEn-log --calibration FILE` uses it.  Without the flag the file is what it always was.
--with-variance also fits one box-variance scale per detector on the same fitted images: every detection is matched to the ground
truth on the device (calibration.match_rows_device, --iou), the matched rows' residuals are the box deltas from the detection to its
ground-truth box (--bbox_reg_weights, the units of the variance head), and s = sum_i q_i / (4 n) minimises their Gaussian NLL under
variance s * var_i (calibration.fit_variance_scale).  The file gains "variance_scales" {name: s}, "variance_nll", "variance_rows",
"variance_excluded" and "variance_coverage"; `demo_probEn --calibration FILE` then fuses with the scaled variances.  Only matched
detections are rows of the fit, so "variance_rows" + "variance_excluded" is the number of matched detections: the excluded count (and the
printed one) is over matched rows - a degenerate box, a variance that is not finite and > 0 - and never includes unmatched detections.  Matching at
IoU >= --iou cuts off the residuals' tails: s is biased low for a detector whose misses are large.  The fit
takes the vars the file carries: fit and fuse under the same PROBEN.FIX_VARS setting.
--with-pool-weights (2 or 3 prediction files) also fits one pooling weight per detector for score_fusion "probEn-log" (DESIGN.md
section 15).  After everything above is fitted, the fitted images are fused once with probEn-log at those temperatures (and prior and
variance scales, when asked for) at w = 1, with --box_fusion (default v-avg), and every cluster of two or more rows is labelled by
matching its fused box to the ground truth on the device (--iou; unmatched = background, a class without a column folds to
background, as above).  The clusters go to the device in CSR form and calibration.fit_pool_weights minimises the NLL of the pooled
posterior against those labels.  The file gains "pool_weights" {name: w}, "pool_nll" {"before", "after"} (per cluster, at w = 1 and
at the fit), "pool_clusters" (used), "pool_excluded" (clusters of one row, which the product does not fuse), "pool_at_bound"
{name: "lo" / "hi" / null} and "pool_fit" (the box fusion, IoU, rounds and whether the gradient criterion was met);
`demo_probEn --score_fusion probEn-log --calibration FILE` then fuses with the weights.
--with-presence (2 or 3 prediction files) also fits the presence table of score_fusion "probEn-log" (DESIGN.md section 18): one row
of log-evidence per presence pattern - which detectors put a row into a cluster.  It runs last, so its base includes the
temperatures, prior, variance scales and pool weights of the same run: the fitted images are fused once through
pe_proben_fuse_batch_presence at a zero table with the posterior outputs (late_fusion.presence_rows), every fused box - clusters of
one row and the rows of images on which one detector fired included - is labelled by matching it to the ground truth on the device
(--iou; unmatched = background), and calibration.fit_presence fits each pattern's row to its clusters.  The file gains "presence"
{"detectors", "columns", "table", "hi", "patterns": per pattern the clusters used / excluded, the NLL per cluster at 0 and at the fit,
rounds, converged, at_bound, "box_fusion", "iou"}; `demo_probEn --score_fusion probEn-log --calibration FILE` then fuses with the table.
--with-box-correlation (2 or 3 prediction files) also fits the correlation of the detectors' box errors for --box_fusion c-avg
(DESIGN.md section 19).  It runs after the variance fit of the same run: the fitted images are fused once with probEn-log at v-avg, at
the run's temperatures, prior and variance scales (late_fusion.fused_clusters); every cluster takes the ground-truth box its fused box
matches on the device (--iou; a cluster without one adds nothing); a member row's residual is the variance fit's, divided by the
square root of its (scaled) variance; calibration.fit_box_correlation forms the uncentred correlation per detector pair from
pe_box_pair_stats' sums - the entry of a detector with itself is that of two different rows of it in one cluster.  Prints the matrix,
the pair counts and the standard errors.  The file gains "box_correlation" {"detectors", "matrix", "raw", "shrink", "pairs", "rows",
"excluded", "stderr", "empty", "clamped", "iou", "box_fusion": "v-avg"};
`demo_probEn --score_fusion probEn-log --box_fusion c-avg --calibration FILE` then fuses with the matrix.
"""
import argparse
import json
import os
import re
import sys

import torch

from .. import calibration
from ..data import load_coco_json
from ..late_fusion import fused_clusters, presence_rows, read_j1
from ..options import FusionOptions


def detector_name(path):
    m = re.fullmatch(r"val_(.+)_predictions\.json", os.path.basename(path))
    return m.group(1) if m else os.path.splitext(os.path.basename(path))[0]


def parse(argv):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--predictions", nargs="+", required=True, help="val_<method>_predictions.json files, one per detector")
    p.add_argument("--dataset_path", required=True, help="FLIR val folder (FLIR_thermal_RGBT_pairs_val.json)")
    p.add_argument("--holdout", type=float, default=0.5, help="fraction of the images (the first ones, dataset order) that is fitted")
    p.add_argument("--out", default="calibration.json")
    p.add_argument("--iou", type=float, default=0.5, help="IoU from which a detection takes a ground-truth box's class")
    p.add_argument("--device", default="cuda")
    p.add_argument("--with-prior", action="store_true",
                   help="also write the label frequencies of the fitted rows (background last, add-one smoothed) as class_prior")
    p.add_argument("--with-variance", action="store_true",
                   help="also fit one box-variance scale per detector on the fitted images and write the variance_* keys")
    p.add_argument("--bbox_reg_weights", type=str, default="10,10,5,5",
                   help="--with-variance: the box head's BBOX_REG_WEIGHTS 'wx,wy,ww,wh' (the units of the predicted variance)")
    p.add_argument("--with-pool-weights", action="store_true",
                   help="also fit one pooling weight per detector for score_fusion probEn-log and write the pool_* keys")
    p.add_argument("--with-presence", action="store_true",
                   help="also fit the presence table of score_fusion probEn-log (one row per pattern of detectors) and write the presence key")
    p.add_argument("--with-box-correlation", action="store_true",
                   help="also fit the correlation of the detectors' box errors for box_fusion c-avg and write the box_correlation key")
    p.add_argument("--box_fusion", default="v-avg", help="--with-pool-weights / --with-presence: box fusion of the fused boxes that are labelled")
    args = p.parse_args(argv)
    if args.with_presence and not 2 <= len(args.predictions) <= 3:
        p.error(f"--with-presence: --predictions lists {len(args.predictions)} files: late fusion takes 2 or 3")
    if args.with_box_correlation and not 2 <= len(args.predictions) <= 3:
        p.error(f"--with-box-correlation: --predictions lists {len(args.predictions)} files: late fusion takes 2 or 3")
    if args.with_pool_weights and not 2 <= len(args.predictions) <= 3:
        p.error(f"--with-pool-weights: --predictions lists {len(args.predictions)} files: late fusion takes 2 or 3")
    if not 0.0 < args.holdout <= 1.0:
        p.error(f"--holdout {args.holdout} is not in (0, 1]")
    try:
        args.bbox_reg_weights = [float(x) for x in args.bbox_reg_weights.split(",")]
    except ValueError:
        p.error(f"--bbox_reg_weights {args.bbox_reg_weights!r} is not 'wx,wy,ww,wh'")
    if len(args.bbox_reg_weights) != 4 or not all(0 < w < float("inf") for w in args.bbox_reg_weights):
        p.error(f"--bbox_reg_weights {args.bbox_reg_weights} is not four numbers that are finite and > 0")
    return args


def variance_fit(pred, records, fitted_ids, iou, name, weights, device):
    """calibration.fit_variance_scale over the file's detections on the fitted images, matched on the device."""
    det, var, gt, cls, crowd, doff, goff = [], [], [], [], [], [0], [0]
    k = None
    for i, iid in enumerate(pred["image_id"]):
        if iid not in fitted_ids:
            continue
        anns = records[iid]["annotations"]
        if len(pred["vars"][i]) != len(pred["boxes"][i]):
            raise ValueError(f"{name}: {len(pred['vars'][i])} vars for the {len(pred['boxes'][i])} detections of image {i} "
                             f"({pred['image'][i]}): the variance fit needs the box head's vars")
        if k is None and pred["class_logits"][i] and len(pred["class_logits"][i][0]) >= 2:
            k = len(pred["class_logits"][i][0]) - 1
        det += pred["boxes"][i]
        var += [v[0] if isinstance(v, (list, tuple)) else v for v in pred["vars"][i]]
        gt += [[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in anns]      # COCO XYWH -> XYXY
        cls += [a["category_id"] for a in anns]
        crowd += [a["iscrowd"] for a in anns]
        doff.append(len(det))
        goff.append(len(gt))
    t = lambda x, dt, shape: torch.tensor(x, dtype=dt).reshape(shape).to(device)
    db, gb = t(det, torch.float64, (-1, 4)), t(gt, torch.float64, (-1, 4))
    _, match, _ = calibration.match_rows_device(db, t(doff, torch.int32, (-1,)), gb, t(goff, torch.int32, (-1,)), t(cls, torch.int32, (-1,)),
                                                t(crowd, torch.int32, (-1,)), iou, k if k is not None else 1)     # k sizes the labels only,
    # which this fit does not read (k is None when no fitted image has a detection: nothing is matched then either)
    hit = match >= 0               # the unmatched detections are no residuals: only the matched rows are rows of the fit
    return calibration.fit_variance_scale(db[hit], match[hit], gb, t(var, torch.float64, (-1,))[hit], weights)


def pool_clusters(dets, names, records, ids, iou, device, cal):
    """The labelled clusters of the pooling-weight fit (and of calibration_report's fused NLL): dets = the prediction dicts sliced to
    the images `ids`, in that order; cal = the FusionOptions ("probEn-log") whose temperatures, prior, variance scales and box fusion
    form them.  late_fusion.fused_clusters fuses them once at w = 1; every fused box is matched to the ground truth of its image on
    the device (pe_match_ground_truth at `iou`): an unmatched cluster is background, and so is a class the head has no column for.
    Returns (clusters, labels i32 [C] on the device), or None when no image has two live detectors."""
    from .calibration_report import ground_truth
    cl = fused_clusters(dets, device=device, names=names, options=cal)
    if cl is None:
        return None
    k = cl["log_probs"].shape[1] - 1
    gt = ground_truth(records, [ids[i] for i in cl["images"]], device)
    labels, _, _ = calibration.match_rows_device(cl["boxes"], cl["box_offsets"], gt[0], gt[1], gt[2], gt[3], iou, k)
    return cl, torch.where((labels < 0) | (labels > k), torch.full_like(labels, k), labels)


def pool_fit(preds, names, records, fitted, iou, device, cal):
    """calibration.fit_pool_weights over the clusters of the fitted images."""
    from .calibration_report import positions, take_j1
    dets = [take_j1(p, positions(p, fitted, n)) for p, n in zip(preds, names)]
    got = pool_clusters(dets, names, records, fitted, iou, device, cal)
    if got is None:
        raise ValueError(f"no image among the {len(fitted)} fitted ones on which two detectors fired: no cluster to fit pooling weights on")
    cl, labels = got
    lp = cl["log_probs"]
    return calibration.fit_pool_weights(lp, cl["row_source"], cl["member_rows"], cl["cluster_offsets"], labels, len(preds),
                                        cal.on(lp.device, lp.shape[1]).log_prior)


def presence_labelled(dets, names, records, ids, iou, device, cal):
    """The labelled fused rows of the presence fit (and of calibration_report's per-pattern NLL): dets = the prediction dicts sliced to
    the images `ids`, in that order; cal = the FusionOptions ("probEn-log") they are fused with.  late_fusion.presence_rows fuses them
    once (a zero table unless cal has one); every fused box is matched to the ground truth of its image on the device: an unmatched row
    is background, and so is a class the head has no column for.  Returns (rows, labels i32 [C] on the device), or None when no
    detector fired."""
    from .calibration_report import ground_truth
    rows = presence_rows(dets, device=device, names=names, options=cal)
    if rows is None:
        return None
    k = rows["log_posterior"].shape[1] - 1
    gt = ground_truth(records, [ids[i] for i in rows["images"]], device)
    labels, _, _ = calibration.match_rows_device(rows["boxes"], rows["box_offsets"], gt[0], gt[1], gt[2], gt[3], iou, k)
    return rows, torch.where((labels < 0) | (labels > k), torch.full_like(labels, k), labels)


def presence_fit(preds, names, records, fitted, iou, device, cal):
    """calibration.fit_presence over the fused rows of the fitted images."""
    from .calibration_report import positions, take_j1
    dets = [take_j1(p, positions(p, fitted, n)) for p, n in zip(preds, names)]
    got = presence_labelled(dets, names, records, fitted, iou, device, cal)
    if got is None:
        raise ValueError(f"no detection on the {len(fitted)} fitted images: no fused row to fit a presence table on")
    rows, labels = got
    return calibration.fit_presence(rows["log_posterior"], rows["pattern"], labels, len(preds))


def box_correlation_fit(preds, names, records, fitted, iou, device, cal, weights):
    """calibration.fit_box_correlation over the clusters probEn-log / v-avg forms on the fitted images, each with the ground-truth box
    its fused box matches (pe_match_ground_truth's match output at `iou`)."""
    from .calibration_report import ground_truth, positions, take_j1
    dets = [take_j1(p, positions(p, fitted, n)) for p, n in zip(preds, names)]
    cl = fused_clusters(dets, device=device, names=names, options=cal)
    if cl is None:
        raise ValueError(f"no image among the {len(fitted)} fitted ones on which two detectors fired: no cluster to fit a box correlation on")
    gt = ground_truth(records, [fitted[i] for i in cl["images"]], device)
    _, match, _ = calibration.match_rows_device(cl["boxes"], cl["box_offsets"], gt[0], gt[1], gt[2], gt[3], iou, cl["log_probs"].shape[1] - 1)
    return calibration.fit_box_correlation(cl["row_boxes"], cl["row_vars"], cl["row_source"], cl["member_rows"], cl["cluster_offsets"],
                                           match, gt[0], len(preds), weights)


def pattern_name(P, names):
    return "+".join(n for d, n in enumerate(names) if P >> d & 1)


def labelled_rows(pred, records, fitted_ids, iou, name):
    """(logits [M, K+1] list, labels [M] list) of the file's detections on the fitted images."""
    calibration.require_logits(pred, name)
    logits, labels = [], []
    for i, iid in enumerate(pred["image_id"]):
        if iid not in fitted_ids or not pred["boxes"][i]:
            continue
        anns = records[iid]["annotations"]
        # COCO XYWH -> XYXY
        gt = [[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]] for a in anns]
        k = len(pred["class_logits"][i][0]) - 1
        lab = calibration.match_labels(pred["boxes"][i], pred["classes"][i], gt, [a["category_id"] for a in anns], iou,
                                       gt_crowd=[a["iscrowd"] for a in anns], num_classes=k)
        # a ground-truth class the detector has no column for (FLIR's dog, category 17 -> index 3 of a 3-class head) is background to it
        lab[(lab < 0) | (lab > k)] = k
        logits += pred["class_logits"][i]
        labels += lab.tolist()
    return logits, labels


def main(cmd=None):
    args = parse(list(cmd) if cmd is not None else sys.argv[1:])
    records = load_coco_json(os.path.join(args.dataset_path, "FLIR_thermal_RGBT_pairs_val.json"),
                             os.path.join(args.dataset_path, "thermal_8_bit"))
    order = [r["image_id"] for r in records]
    n_fit = max(1, int(len(order) * args.holdout))
    fitted = order[:n_fit]
    by_id = {r["image_id"]: r for r in records}
    temps, nll, rows, bound = {}, {}, {}, {}
    vfit, preds = {}, []
    counts = None
    for path in args.predictions:
        name = detector_name(path)
        if name in temps:
            raise ValueError(f"{path}: a second prediction file for detector {name}")
        pred = read_j1(path)
        preds.append(pred)
        logits, labels = labelled_rows(pred, by_id, set(fitted), args.iou, path)
        if not logits:
            raise ValueError(f"{path}: no detections on the {n_fit} fitted images: nothing to fit")
        if args.with_prior:
            k1 = len(logits[0])
            if counts is not None and len(counts) != k1:
                raise ValueError(f"{path}: {k1} class columns, the files before it have {len(counts)}: one prior cannot serve both")
            counts = [a + b for a, b in zip(counts or [0] * k1, [labels.count(j) for j in range(k1)])]
        fit = calibration.fit_temperature(torch.tensor(logits, dtype=torch.float32, device=args.device),
                                          torch.tensor(labels, dtype=torch.int32, device=args.device))
        temps[name], rows[name], bound[name] = fit["T"], fit["rows"], fit["at_bound"]
        nll[name] = {"before": fit["nll_at_1"], "after": fit["nll"]}
        note = f"  (minimum on the {fit['at_bound']} end of the search range: not a fitted value)" if fit["at_bound"] else ""
        print(f"{name}: T = {fit['T']:.6f}  NLL {fit['nll_at_1']:.6f} -> {fit['nll']:.6f} over {fit['rows']} rows{note}")
        if args.with_variance:
            try:
                v = vfit[name] = variance_fit(pred, by_id, set(fitted), args.iou, path, args.bbox_reg_weights, args.device)
            except ValueError as e:
                raise ValueError(f"{path}: {e}") from None
            print(f"{name}: variance scale = {v['scale']:.6f}  NLL {v['nll_before']:.6f} -> {v['nll_after']:.6f} over {v['rows']} matched rows "
                  f"({v['excluded']} excluded), within 1 / 2 sigma {v['coverage_before'][0]:.4f} / {v['coverage_before'][1]:.4f} -> "
                  f"{v['coverage_after'][0]:.4f} / {v['coverage_after'][1]:.4f} (a Gaussian: 0.6827 / 0.9545)")
    pool = {}
    names = list(temps)
    if args.with_pool_weights or args.with_presence or args.with_box_correlation:
        # the calibration fitted so far, as the later fits fuse with it (the box-correlation fit at v-avg, the others at --box_fusion)
        cal = FusionOptions("probEn-log", "v-avg", [temps[n] for n in names], [c + 1 for c in counts] if args.with_prior else None,
                            [vfit[n]["scale"] for n in names] if args.with_variance else None, num_detectors=len(names), who="fit_temperature")
    if args.with_pool_weights:
        fit = pool_fit(preds, args.predictions, by_id, fitted, args.iou, args.device, cal.replace(box_fusion=args.box_fusion))
        n = fit["clusters"]
        pool = {"pool_weights": dict(zip(names, fit["weights"])), "pool_nll": {"before": fit["nll_at_1"] / n, "after": fit["nll"] / n},
                "pool_clusters": n, "pool_excluded": fit["excluded"], "pool_at_bound": dict(zip(names, fit["at_bound"])),
                "pool_fit": {"box_fusion": args.box_fusion, "iou": args.iou, "rounds": fit["rounds"], "converged": fit["converged"]}}
        held = [f"{m} on the {a} end" for m, a in zip(names, fit["at_bound"]) if a]
        note = f"  (minimum on the search range's bound: {', '.join(held)}: not a fitted value)" if held else ""
        print("pool weights:", ", ".join(f"{m} = {w:.6f}" for m, w in zip(names, fit["weights"])),
              f" NLL per cluster {fit['nll_at_1'] / n:.6f} -> {fit['nll'] / n:.6f} over {n} clusters of >= 2 rows ({fit['excluded']} excluded)"
              f"{'' if fit['converged'] else '  (the gradient criterion was not met)'}{note}")
    if args.with_presence:
        fit = presence_fit(preds, args.predictions, by_id, fitted, args.iou, args.device,
                           cal.replace(box_fusion=args.box_fusion, pool_weights=[pool["pool_weights"][n] for n in names] if pool else None))
        per = {}
        for P, r in fit["patterns"].items():
            n = max(r["clusters"], 1)
            per[pattern_name(P, names)] = {"pattern": P, "clusters": r["clusters"], "excluded": r["excluded"],
                                           "nll": {"before": r["nll_at_0"] / n, "after": r["nll"] / n}, "rounds": r["rounds"],
                                           "converged": r["converged"], "at_bound": r["at_bound"]}
            held = [f"column {j} on the {a} end" for j, a in enumerate(r["at_bound"]) if a]
            note = f"  (on the search range's bound +-{fit['hi']:g}: {', '.join(held)}: not a fitted value)" if held else ""
            print(f"presence {pattern_name(P, names)}: ({', '.join(f'{v:+.6f}' for v in fit['table'][P])})  NLL per cluster "
                  f"{r['nll_at_0'] / n:.6f} -> {r['nll'] / n:.6f} over {r['clusters']} clusters ({r['excluded']} excluded)"
                  f"{'' if r['converged'] else '  (the gradient criterion was not met)'}{note}")
        pool = dict(pool, presence={"detectors": names, "columns": len(fit["table"][0]), "table": fit["table"], "hi": fit["hi"],
                                    "patterns": per, "unassigned": fit["unassigned"], "box_fusion": args.box_fusion, "iou": args.iou})
    if args.with_box_correlation:
        fit = box_correlation_fit(preds, args.predictions, by_id, fitted, args.iou, args.device, cal, args.bbox_reg_weights)
        shrunk = "" if fit["shrink"] == 1.0 else f"; off-diagonal entries times {fit['shrink']:.6f} to make it positive semidefinite"
        print(f"box correlation ({sum(fit['rows'])} member rows, {fit['excluded']} excluded{shrunk}):")
        for a in range(len(names)):
            for b in range(a, len(names)):
                se = fit["stderr"][a][b]
                note = "  (no pair: set to 0)" if [a, b] in fit["empty"] else "  (not in [0, 1): set to 0)" if a == b and a in fit["clamped"] else ""
                print(f"  {names[a]}:{names[b]} = {fit['matrix'][a][b]:+.6f}  raw {fit['raw'][a][b]:+.6f}  over {fit['pairs'][a][b]} pairs, "
                      f"standard error {'-' if se is None else format(se, '.6f')}{note}")
        pool = dict(pool, box_correlation=dict(fit, detectors=names, iou=args.iou, box_fusion="v-avg"))
    if args.with_prior:
        calibration.save(args.out, temps, nll, rows, class_prior=[c + 1 for c in counts], holdout=args.holdout, fitted_image_ids=fitted,
                         at_bound=bound, class_prior_counts=counts, **pool)
        print("class prior (background last):", ", ".join(f"{c + 1}/{sum(counts) + len(counts)}" for c in counts))
    else:
        calibration.save(args.out, temps, nll, rows, holdout=args.holdout, fitted_image_ids=fitted, at_bound=bound, **pool)
    if args.with_variance:
        calibration.save_variance(args.out, {n: v["scale"] for n, v in vfit.items()},
                                  {n: {"before": v["nll_before"], "after": v["nll_after"]} for n, v in vfit.items()},
                                  {n: v["rows"] for n, v in vfit.items()}, {n: v["excluded"] for n, v in vfit.items()},
                                  {n: {"before": v["coverage_before"], "after": v["coverage_after"]} for n, v in vfit.items()})
    print("calibration file:", args.out)
    return args.out


if __name__ == "__main__":
    main()
