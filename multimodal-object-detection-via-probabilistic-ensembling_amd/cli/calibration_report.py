"""Held-out calibration report: does what cli/fit_temperature fitted help on the images it did not see?

    python -m proben_amd.cli.calibration_report --dataset_path DATA/FLIR/val \\
        --predictions out/val_thermal_only_predictions.json out/val_early_fusion_predictions.json \\
        --calibration calibration.json [--bins 15] [--iou 0.5] [--on heldout|fitted|all] \\
        [--score_fusion probEn --box_fusion v-avg] [--fused-posterior] [--out report.json]

--on heldout (the default) takes the dataset's images that are not among the calibration file's "fitted_image_ids"; `fitted` takes
those, `all` every image.  A file fitted with --holdout 1.0 leaves nothing held out: that is refused, choose --on fitted or --on all.

Per detector (the <name> of val_<name>_predictions.json), once at T = 1 ("before") and once at the file's T ("after"): the detections
of the chosen images are labelled on the device in one launch (calibration.match_rows_device; a ground-truth class the head has no
column for is background, as in the fit), then the NLL per row (calibration.temperature_nll) and ECE, MCE and the Brier score of the
detection's own score p[class] - the score ProbEn consumes - from calibration.reliability; "top_label" holds the same for the top label
over all K + 1 columns.  When the file has "variance_scales": the Gaussian NLL per matched row and the 1-sigma / 2-sigma coverage of
the box residuals (calibration.variance_stats) at s = 1 and at the file's s, beside a Gaussian's 0.6827 / 0.9545.
For the fused detections: late_fusion over the chosen images without any calibration ("before") and with the file's temperatures,
variance scales and - for --score_fusion probEn-log - class prior ("after"); the fused boxes are matched the same way, a fused row is
correct when its label is its fused class, and its confidence is its fused score (calibration.reliability_scores).
When the file has "pool_weights" (fit_temperature --with-pool-weights): the "after" fusion of --score_fusion probEn-log uses them,
and the report prints the NLL per cluster of the fused posterior against the label of the fused box, at w = 1 and at the file's
weights, over the clusters of two or more rows that probEn-log forms on the chosen images at the file's temperatures, prior and
variance scales (fit_temperature.pool_clusters: the fit's own labelling; calibration.pool_nll, both in one launch).
When the file has "presence" (fit_temperature --with-presence): the "after" fusion of --score_fusion probEn-log uses the table, and
the report prints the NLL per fused row of the fused posterior against the label of the fused box, without the table (the candidate
b = 0) and with it, per presence pattern and overall, over every fused row probEn-log forms on the chosen images at the file's
temperatures, prior, variance scales and pool weights - clusters of one row and passthrough rows included
(fit_temperature.presence_labelled: the fit's own labelling; calibration.bias_nll, both candidates in one launch per pattern).
--fused-posterior (with --score_fusion probEn-log) judges the fused detections as full predictions (late_fusion with_posterior,
pe_proben_fuse_batch_posterior), before and after: under "posterior" the NLL per fused row of the fused posterior against the label of
the fused box (calibration.temperature_nll at T = 1 on the fused log-posterior) and ECE / MCE / Brier of its top label over all K + 1
columns; under "variance" the Gaussian NLL per matched fused row and the 1-sigma / 2-sigma coverage of the fused boxes' residuals under
the fused variance (calibration.variance_stats), as printed per detector.  The posterior figures go through the statistics the detectors'
logits go through, which take float32: they are those of the float32 cast of the float64 fused log-posterior (6e-8 relative on a
log-probability), renormalised - a report's precision, not the fusion's.  Only new keys: everything else is what it is without the flag.
When the file also has "box_correlation" (fit_temperature --with-box-correlation), --fused-posterior prints the same Gaussian NLL and
coverage of the fused box variance under --box_fusion v-avg and under c-avg at the file's matrix, side by side, both at the file's
calibration: c-avg moves boxes and variances only, so the two fusions have the same rows.
Rows that cannot be binned (a NaN score, a label outside the columns) are counted as "excluded" and printed, never dropped silently.

What the detection-level figures are not.  A detection is "correct" when the ground-truth box it overlaps most, at IoU >= --iou, has
its class: two detections on one box are both correct.  That is the temperature fit's labelling, not COCO's one-to-one matching, so
the figures describe the scores as the fit sees them, not AP.  And with no trained weights or FLIR frames offline, whatever this
prints on synthetic detectors says nothing about real FLIR data.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from .. import calibration
from ..data import load_coco_json
from ..late_fusion import late_fusion, read_j1
from ..options import FusionOptions
from .fit_temperature import detector_name, pattern_name, pool_clusters, presence_labelled

ON = ("heldout", "fitted", "all")
GAUSSIAN_COVERAGE = (0.682689492137086, 0.954499736103642)


def parse(argv):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--predictions", nargs="+", required=True, help="val_<method>_predictions.json files, one per detector")
    p.add_argument("--dataset_path", required=True, help="FLIR val folder (FLIR_thermal_RGBT_pairs_val.json)")
    p.add_argument("--calibration", required=True, help="the file cli/fit_temperature wrote")
    p.add_argument("--bins", type=int, default=15, help="confidence bins of equal width on [0, 1]")
    p.add_argument("--iou", type=float, default=0.5, help="IoU from which a detection takes a ground-truth box's class")
    p.add_argument("--on", choices=ON, default="heldout", help="which images: those the file was not fitted on, those it was, or all")
    p.add_argument("--score_fusion", default="probEn", help="score fusion of the fused detections (avg / max / probEn / probEn-log)")
    p.add_argument("--box_fusion", default="v-avg", help="box fusion of the fused detections (v-avg / s-avg / avg / argmax)")
    p.add_argument("--fused-posterior", action="store_true",
                   help="--score_fusion probEn-log: also report the fused posterior (NLL per row, top-label ECE / MCE / Brier) and the "
                        "fused box variance (Gaussian NLL, 1-sigma / 2-sigma coverage)")
    p.add_argument("--out", default=None, help="write the report as JSON")
    p.add_argument("--device", default="cuda")
    args = p.parse_args(argv)
    if not 1 <= args.bins <= calibration.RELIABILITY_MAX_BINS:
        p.error(f"--bins {args.bins} is not in [1, {calibration.RELIABILITY_MAX_BINS}]")
    if not 0.0 <= args.iou <= 1.0:
        p.error(f"--iou {args.iou} is not in [0, 1]")
    if not 2 <= len(args.predictions) <= 3:
        p.error(f"--predictions lists {len(args.predictions)} files: late fusion takes 2 or 3")
    if args.box_fusion == "c-avg":
        p.error("--box_fusion c-avg: the \"before\" fusion has no matrix to run it with; --fused-posterior with a calibration file that "
                "carries \"box_correlation\" prints v-avg and c-avg side by side")
    if args.fused_posterior and args.score_fusion != "probEn-log":
        p.error(f"--fused-posterior belongs to --score_fusion probEn-log (got {args.score_fusion}): the other score fusions form no posterior")
    return args


def select_images(order, fitted_ids, on, source="the calibration file"):
    """The dataset's image ids (dataset order) that --on names.  An empty choice is refused."""
    if on not in ON:
        raise ValueError(f"--on {on!r} is not one of {', '.join(ON)}")
    fitted = set(fitted_ids)
    ids = [i for i in order if on == "all" or (i in fitted) == (on == "fitted")]
    if not ids:
        what = ("lists every image of the dataset among its fitted_image_ids (fit_temperature --holdout 1.0): nothing is held out"
                if on == "heldout" else "lists none of the dataset's images among its fitted_image_ids" if on == "fitted"
                else "is beside an empty dataset")
        raise ValueError(f"{source} {what}.  Choose the images with --on {' / --on '.join(o for o in ON if o != on)}")
    return ids


def take_j1(det, index):
    """shard_j1 for a list of positions: the prediction dict of those images."""
    return {k: [v[i] for i in index] for k, v in det.items()}


def positions(pred, ids, name):
    where = {iid: i for i, iid in enumerate(pred["image_id"])}
    missing = [i for i in ids if i not in where]
    if missing:
        raise ValueError(f"{name}: no entry for {len(missing)} of the {len(ids)} chosen images (image id {missing[0]} is one)")
    return [where[i] for i in ids]


def ground_truth(records, ids, device):
    """(boxes f64 [G,4] XYXY, offsets i32 [B+1], classes i32 [G], crowd i32 [G]) of the chosen images on the device."""
    gt, cls, crowd, off = [], [], [], [0]
    for iid in ids:
        for a in records[iid]["annotations"]:
            x, y, w, h = a["bbox"]                        # COCO XYWH -> XYXY
            gt.append([x, y, x + w, y + h])
            cls.append(a["category_id"])
            crowd.append(a["iscrowd"])
        off.append(len(gt))
    t = lambda x, dt, shape: torch.tensor(x, dtype=dt).reshape(shape).to(device)
    return t(gt, torch.float64, (-1, 4)), t(off, torch.int32, (-1,)), t(cls, torch.int32, (-1,)), t(crowd, torch.int32, (-1,))


def match_device(boxes, offsets, gt, iou, k, device):
    """Labels in [0, k] (a class outside the head's columns folds to k, as fit_temperature.labelled_rows does) and the match index."""
    db = torch.tensor(boxes, dtype=torch.float64).reshape(-1, 4).to(device)
    doff = torch.tensor(offsets, dtype=torch.int32).to(device)
    labels, match, _ = calibration.match_rows_device(db, doff, gt[0], gt[1], gt[2], gt[3], iou, k)
    labels = torch.where((labels < 0) | (labels > k), torch.full_like(labels, k), labels)
    return db, labels, match


def _figures(rel):
    return {k: rel[k] for k in ("rows", "excluded", "ece", "mce", "brier", "bins")}


def detector_report(pred, name, gt, T, bins, iou, device):
    """{"before", "after"} of one (already sliced) prediction dict, plus the tensors the variance block reuses."""
    calibration.require_logits(pred, name)
    flat = lambda key: [r for rows in pred[key] for r in rows]
    logits, classes = flat("class_logits"), flat("classes")
    if not logits:
        raise ValueError(f"{name}: no detections on the chosen images: nothing to report")
    k = len(logits[0]) - 1
    offsets = np.cumsum([0] + [len(b) for b in pred["boxes"]]).tolist()
    db, labels, match = match_device(flat("boxes"), offsets, gt, iou, k, device)
    lg = torch.tensor(logits, dtype=torch.float32, device=device).reshape(len(logits), k + 1)
    cls = torch.tensor(classes, dtype=torch.int32, device=device)
    out = {}
    for tag, t in (("before", 1.0), ("after", T)):
        nll, _ = calibration.temperature_nll(lg, labels, [t])
        rec = {"T": t, "nll": float(nll[0]) / len(logits)}
        rec.update(_figures(calibration.reliability(lg, labels, t, cls, bins)))
        rec["top_label"] = _figures(calibration.reliability(lg, labels, t, None, bins))
        out[tag] = rec
    return out, (db, match)


def variance_report(pred, rows, gt_boxes, s, device):
    """Gaussian NLL per matched row and the coverage of the box residuals at s = 1 and at the file's s."""
    db, match = rows
    var = torch.tensor([v[0] if isinstance(v, (list, tuple)) else v for r in pred["vars"] for v in r], dtype=torch.float64, device=device)
    if var.numel() != db.shape[0]:
        raise ValueError(f"{var.numel()} vars for {db.shape[0]} detections: the variance report needs the box head's vars")
    hit = match >= 0
    out = {}
    for tag, scale in (("before", 1.0), ("after", s)):
        st = calibration.variance_stats(db[hit], match[hit], gt_boxes, var[hit], scale)
        n = st["n"]
        out[tag] = {"scale": scale, "rows": n, "excluded": st["excluded"],
                    "nll": calibration.variance_nll(st, scale) / n if n else float("nan"),
                    "coverage": [st["cover1"] / (4 * n), st["cover2"] / (4 * n)] if n else [float("nan")] * 2}
    return out


def fused_report(dets, names, gt, k, bins, iou, device, options):
    """Reliability of the fused score of late_fusion(dets, options=options) on the chosen images.  options.with_posterior: plus "posterior"
    (NLL per row and top-label reliability of the fused posterior, of its float32 cast: the statistics take float32 logits) and "variance" (the fused boxes' residuals under the fused variance)."""
    posterior = options.with_posterior
    boxes, conf, cls, offsets, lq, var = [], [], [], [0], [], []
    for r in late_fusion(dets, [options.score_fusion, options.box_fusion], device, names=names, options=options):
        if r is not None:
            boxes += np.asarray(r[0], dtype=np.float64).reshape(-1, 4).tolist()
            conf += r[1].double().tolist()
            cls += r[2].tolist()
            if posterior:
                lq.append(r[3])
                var.append(r[4])
        offsets.append(len(boxes))
    db, labels, match = match_device(boxes, offsets, gt, iou, k, device)
    correct = labels == torch.tensor(cls, dtype=torch.float64, device=device).to(torch.int32)
    out = _figures(calibration.reliability_scores(torch.tensor(conf, dtype=torch.float64, device=device), correct, bins))
    if posterior:
        n = len(boxes)
        out["posterior"] = {"rows": n, "nll": float("nan"), "top_label": None}
        out["variance"] = {"rows": 0, "excluded": 0, "nll": float("nan"), "coverage": [float("nan")] * 2}
        if n:
            lg = torch.from_numpy(np.concatenate(lq).reshape(n, k + 1)).to(device)       # the fused log-posterior is its own logits at T = 1
            nll, _ = calibration.temperature_nll(lg, labels, [1.0])
            out["posterior"] = {"rows": n, "nll": float(nll[0]) / n, "top_label": _figures(calibration.reliability(lg, labels, 1.0, None, bins))}
            hit = match >= 0
            st = calibration.variance_stats(db[hit], match[hit], gt[0], torch.from_numpy(np.concatenate(var)).to(device)[hit], 1.0)
            m = st["n"]
            out["variance"] = {"rows": m, "excluded": st["excluded"], "nll": calibration.variance_nll(st, 1.0) / m if m else float("nan"),
                               "coverage": [st["cover1"] / (4 * m), st["cover2"] / (4 * m)] if m else [float("nan")] * 2}
    return out


def pool_report(dets, names, records, ids, iou, device, cal):
    """NLL per cluster of probEn-log's fused posterior on the chosen images, at w = 1 ("before") and at cal's pool weights ("after");
    cal = the file's calibration as a FusionOptions ("probEn-log")."""
    out = {"clusters": 0, "excluded": 0, "nll": {"before": float("nan"), "after": float("nan")}}
    got = pool_clusters(dets, names, records, ids, iou, device, cal)
    if got is None:
        return out
    cl, labels = got
    lp, weights = cl["log_probs"], cal.pool_weights
    prior = cal.on(lp.device, lp.shape[1]).log_prior
    nll, _, bad, _ = calibration.pool_nll(lp, cl["row_source"], cl["member_rows"], cl["cluster_offsets"], labels,
                                          [[1.0] * len(weights), weights], prior)
    used = int(labels.numel()) - bad
    out["clusters"], out["excluded"] = used, bad
    if used:
        out["nll"] = {"before": float(nll[0]) / used, "after": float(nll[1]) / used}
    return out


def presence_report(dets, names, files, records, ids, iou, device, cal):
    """NLL per fused row of probEn-log's fused posterior on the chosen images, without cal's presence table ("before": b = 0) and with it
    ("after"), per pattern and overall; both from pe_bias_nll over the rows fused at a zero table.  cal = the file's calibration as a
    FusionOptions ("probEn-log")."""
    nan = float("nan")
    table = cal.presence
    out = {"rows": 0, "excluded": 0, "nll": {"before": nan, "after": nan}, "patterns": {}}
    got = presence_labelled(dets, files, records, ids, iou, device, cal.replace(presence=None))
    if got is None:
        return out
    rows, labels = got
    tot = [0.0, 0.0]
    for P in range(1, len(table)):
        idx = torch.nonzero(rows["pattern"] == P).flatten()
        nll, _, bad, _ = calibration.bias_nll(rows["log_posterior"][idx], labels[idx], [np.zeros(len(table[P])), table[P]])
        used = int(idx.numel()) - bad
        out["patterns"][pattern_name(P, names)] = {"pattern": P, "rows": used, "excluded": bad,
                                                   "nll": {"before": float(nll[0]) / used if used else nan, "after": float(nll[1]) / used if used else nan}}
        out["rows"] += used
        out["excluded"] += bad
        tot = [tot[0] + float(nll[0]), tot[1] + float(nll[1])]
    if out["rows"]:
        out["nll"] = {"before": tot[0] / out["rows"], "after": tot[1] / out["rows"]}
    return out


def table(report):
    head = ("", "", "rows", "excl", "NLL/row", "ECE", "MCE", "Brier", "1 sigma", "2 sigma")
    rows = [head]
    f = lambda x: "-" if x is None else f"{x:.6f}"
    for name, d in report["detectors"].items():
        for tag in ("before", "after"):
            r = d[tag]
            rows.append((name, f"{tag} (T = {r['T']:.4g})", str(r["rows"]), str(r["excluded"]), f(r["nll"]), f(r["ece"]), f(r["mce"]), f(r["brier"]), "", ""))
            t = r["top_label"]
            rows.append((name, "  top label", str(t["rows"]), str(t["excluded"]), "", f(t["ece"]), f(t["mce"]), f(t["brier"]), "", ""))
    for name, d in report["variance"].items():
        for tag in ("before", "after"):
            r = d[tag]
            rows.append((name, f"variance {tag} (s = {r['scale']:.4g})", str(r["rows"]), str(r["excluded"]), f(r["nll"]), "", "", "",
                         f(r["coverage"][0]), f(r["coverage"][1])))
    if report["variance"]:
        rows.append(("", "a Gaussian", "", "", "", "", "", "", f(GAUSSIAN_COVERAGE[0]), f(GAUSSIAN_COVERAGE[1])))
    for tag in ("before", "after"):
        r = report["fused"][tag]
        rows.append(("fused", f"{tag} ({'/'.join(report['method'])})", str(r["rows"]), str(r["excluded"]), "", f(r["ece"]), f(r["mce"]), f(r["brier"]), "", ""))
        if "posterior" in r and r["posterior"]["rows"]:       # no fused row: nothing to print (the keys hold NaN / None)
            q, t, v = r["posterior"], r["posterior"]["top_label"], r["variance"]
            rows.append(("fused", "  posterior, top label", str(q["rows"]), str(t["excluded"]), f(q["nll"]), f(t["ece"]), f(t["mce"]), f(t["brier"]), "", ""))
            rows.append(("fused", "  fused box variance", str(v["rows"]), str(v["excluded"]), f(v["nll"]), "", "", "",
                         f(v["coverage"][0]), f(v["coverage"][1])))
    width = [max(len(r[c]) for r in rows) for c in range(len(head))]
    return "\n".join("  ".join(x.ljust(w) if c < 2 else x.rjust(w) for c, (x, w) in enumerate(zip(r, width))).rstrip() for r in rows)


def main(cmd=None):
    args = parse(list(cmd) if cmd is not None else sys.argv[1:])
    rec = calibration.load(args.calibration)
    records = load_coco_json(os.path.join(args.dataset_path, "FLIR_thermal_RGBT_pairs_val.json"),
                             os.path.join(args.dataset_path, "thermal_8_bit"))
    ids = select_images([r["image_id"] for r in records], rec.get("fitted_image_ids", []), args.on, args.calibration)
    by_id = {r["image_id"]: r for r in records}
    names = [detector_name(p) for p in args.predictions]
    if len(set(names)) != len(names):
        raise ValueError(f"two prediction files for one detector ({', '.join(names)})")
    # the file as demo_probEn would fuse with it: `after` at the report's own fusion, `cal` at probEn-log (everything the file carries)
    after = FusionOptions.from_args(args, names, who="calibration_report", say=None).replace(with_posterior=args.fused_posterior)
    cal = FusionOptions.from_args(argparse.Namespace(score_fusion="probEn-log", box_fusion=args.box_fusion, calibration=args.calibration),
                                  names, who="calibration_report", say=None)
    temps, svals, pvals, ptable = cal.temperatures, cal.variance_scales, cal.pool_weights, cal.presence
    gt = ground_truth(by_id, ids, args.device)
    report = {"images": ids, "on": args.on, "bins": args.bins, "iou": args.iou, "method": [args.score_fusion, args.box_fusion],
              "detectors": {}, "variance": {}}
    dets, k1 = [], set()
    for d, (path, name) in enumerate(zip(args.predictions, names)):
        full = read_j1(path)
        pred = take_j1(full, positions(full, ids, path))
        report["detectors"][name], rows = detector_report(pred, path, gt, temps[d], args.bins, args.iou, args.device)
        if svals is not None:
            try:
                report["variance"][name] = variance_report(pred, rows, gt[0], svals[d], args.device)
            except ValueError as e:
                raise ValueError(f"{path}: {e}") from None
        k1.add(len(next(r for rows_ in pred["class_logits"] for r in rows_)))
        dets.append(pred)
    if len(k1) != 1:
        raise ValueError(f"the prediction files have {sorted(k1)} class columns: they cannot be fused")
    k = k1.pop() - 1
    logp = after.logp
    fuse = lambda options: fused_report(dets, args.predictions, gt, k, args.bins, args.iou, args.device, options)  # noqa: E731
    report["fused"] = {"before": fuse(FusionOptions(args.score_fusion, args.box_fusion, with_posterior=args.fused_posterior,
                                                    num_detectors=len(names), who="calibration_report")), "after": fuse(after)}
    ctable = None if "box_correlation" not in rec or not (logp and args.fused_posterior) else \
        calibration.resolve_box_correlation(rec["box_correlation"], names, args.calibration)
    if ctable is not None:
        report["box_correlation"] = {"v-avg": fuse(after.replace(box_fusion="v-avg"))["variance"],
                                     "c-avg": fuse(after.replace(box_fusion="c-avg", box_correlation=ctable))["variance"],
                                     "matrix": ctable.tolist(), "detectors": names}
    if pvals is not None:
        report["pool"] = pool_report(dets, args.predictions, by_id, ids, args.iou, args.device, cal)
        report["pool"]["weights"] = dict(zip(names, pvals))
        report["pool"]["applied"] = logp
    if ptable is not None:
        report["presence"] = presence_report(dets, names, args.predictions, by_id, ids, args.iou, args.device, cal)
        report["presence"]["table"] = ptable.tolist()
        report["presence"]["applied"] = logp
    print(f"{len(ids)} images ({args.on}) of {len(records)}, {args.bins} bins, IoU >= {args.iou}")
    print(table(report))
    if ctable is not None:
        print("fused box variance at the file's calibration, under v-avg and under c-avg at the file's box correlation "
              f"({', '.join(f'{names[a]}:{names[b]} = {ctable[a, b]:.6g}' for a in range(len(names)) for b in range(a, len(names)))}):")
        for rule in ("v-avg", "c-avg"):
            v = report["box_correlation"][rule]
            print(f"  {rule}: Gaussian NLL per matched fused row {v['nll']:.6f} over {v['rows']} rows ({v['excluded']} excluded), within 1 / 2 "
                  f"sigma {v['coverage'][0]:.6f} / {v['coverage'][1]:.6f} (a Gaussian: {GAUSSIAN_COVERAGE[0]:.4f} / {GAUSSIAN_COVERAGE[1]:.4f})")
    if pvals is not None:
        r = report["pool"]
        print(f"fused NLL per cluster (probEn-log/{args.box_fusion}, {r['clusters']} clusters of >= 2 rows, {r['excluded']} excluded): "
              f"{r['nll']['before']:.6f} at w = 1, {r['nll']['after']:.6f} at the file's pool weights "
              f"({', '.join(f'{n} = {w:.6g}' for n, w in zip(names, pvals))})")
        if not logp:
            print(f"the file's pool weights are not in the fused rows above: --score_fusion {args.score_fusion} has no pooled form "
                  "(they belong to probEn-log)")
    if ptable is not None:
        r = report["presence"]
        print(f"fused NLL per row (probEn-log/{args.box_fusion}, {r['rows']} fused rows, {r['excluded']} excluded): "
              f"{r['nll']['before']:.6f} without the presence table, {r['nll']['after']:.6f} with the file's")
        for pname, q in r["patterns"].items():
            print(f"  presence {pname}: {q['nll']['before']:.6f} -> {q['nll']['after']:.6f} over {q['rows']} rows ({q['excluded']} excluded)")
        if not logp:
            print(f"the file's presence table is not in the fused rows above: --score_fusion {args.score_fusion} has no log-evidence to add "
                  "it to (it belongs to probEn-log)")
    excluded = sum(d[t]["excluded"] + d[t]["top_label"]["excluded"] for d in report["detectors"].values() for t in ("before", "after")) \
        + sum(report["fused"][t]["excluded"] for t in ("before", "after"))
    if excluded:
        print("excluded rows (a NaN score, a label or class outside the columns) are not in the figures above: see the excl column")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
        print("report:", args.out)
    return report


if __name__ == "__main__":
    main()
