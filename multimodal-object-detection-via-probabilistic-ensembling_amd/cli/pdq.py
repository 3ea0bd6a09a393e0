"""Is a fused detection a better PROBABILISTIC prediction?  The Probability-based Detection Quality of a prediction file.

    python -m proben_amd.cli.pdq --dataset_path DATA/FLIR/val --predictions A.json [B.json] \\
        [--calibration calibration.json | --temperatures ... --variance_scales ...] \\
        [--score_thresh 0.5[,0.3,...]] [--support 0.0027] [--replicates 2000] [--seed 0] [--confidence 0.95] [--out report.json]

AP is blind to a monotone change of the scores and never reads a variance; PDQ (Hall et al., WACV 2020; DESIGN.md section 30 states the
rule as computed here, restated from the paper) scores each detection's label distribution and per-pixel box probability against the
ground truth it is optimally assigned to: PDQ = sum of the pair qualities / (TP + FP + FN).  Printed per file and score threshold: PDQ with
its percentile-bootstrap interval over resampled images and standard error, the mean pair, spatial, label, foreground and background
quality of the true positives, and the three counts.  With two files over the same images both are evaluated under the SAME resamples and
the paired difference B - A is printed with its interval and the two-sided bootstrap p-value.  The pair qualities take one launch per
file (pe_pdq_pair_quality); the intervals come from the per-image records, with no further launch.

A file is a prediction file of the detectors' schema.  With class_logits a row's label distribution is softmax(logits / T) and its box
variance s * vars, T and s those of the file's detector (the <name> of val_<name>_predictions.json) in --calibration, or the entry of
--temperatures / --variance_scales (by position or name=value); a file the calibration does not name - a fused file - takes T = 1 and
s = 1.  A file without logits and probabilities (a conventional method's, `wbf --write_fused`) is scored as what it is: the score on the
row's class, the rest spread evenly, a hard box.  Only rows with score >= --score_thresh take part (the calibrated score where there are
logits).  Limits: box ground truth only, one scalar variance per box, corners treated as independent, and a detection on a crowd box is a
false positive.
"""
import argparse
import json
import os
import sys

from .. import bootstrap, calibration, pdq
from ..data import load_coco_json
from ..late_fusion import read_j1
from .fit_temperature import detector_name


def parse(argv):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--predictions", nargs="+", required=True, help="one prediction file, or two for the paired difference B - A")
    p.add_argument("--dataset_path", required=True, help="FLIR val folder (FLIR_thermal_RGBT_pairs_val.json)")
    p.add_argument("--calibration", default=None, help="the file cli/fit_temperature wrote: T and s per detector name")
    p.add_argument("--temperatures", default=None, help="T per file: 'a[,b]' by position or 'name=a,...'")
    p.add_argument("--variance_scales", default=None, help="s per file, like --temperatures")
    p.add_argument("--score_thresh", default="0.5", help="score threshold, or a comma list of them")
    p.add_argument("--support", type=float, default=0.0027, help="tau: a detection claims the pixels where its probability is above it")
    p.add_argument("--num_classes", type=int, default=None, help="K, for files without logits and probabilities (default 3)")
    p.add_argument("--replicates", type=int, default=2000, help="resamples of the image list")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--confidence", type=float, default=0.95, help="coverage of the percentile interval")
    p.add_argument("--out", default=None, help="write the report as JSON")
    p.add_argument("--device", default="cuda")
    args = p.parse_args(argv)
    if not 1 <= len(args.predictions) <= 2:
        p.error(f"--predictions lists {len(args.predictions)} files: one, or two for the paired difference")
    if args.replicates < 2:
        p.error(f"--replicates {args.replicates} is below 2")
    if not 0.0 < args.confidence < 1.0:
        p.error(f"--confidence {args.confidence} is not in (0, 1)")
    if not 0.0 <= args.support < 1.0:
        p.error(f"--support {args.support} is not in [0, 1)")
    try:
        args.thresholds = sorted({float(x) for x in args.score_thresh.split(",") if x.strip()})
    except ValueError:
        p.error(f"--score_thresh {args.score_thresh!r} is not a number or a comma list of numbers")
    if not args.thresholds or any(not 0.0 <= t <= 1.0 for t in args.thresholds):
        p.error(f"--score_thresh {args.score_thresh!r}: thresholds lie in [0, 1]")
    if args.calibration is not None and (args.temperatures is not None or args.variance_scales is not None):
        p.error("--calibration and --temperatures / --variance_scales: one or the other")
    return args


def resolve(args, names):
    """(T, s) per file: the flags' entries, else the calibration file's entry for the file's detector name, else 1 (a fused file)."""
    T, s = [1.0] * len(names), [1.0] * len(names)
    if args.temperatures is not None:
        T = calibration.parse_temperatures(args.temperatures, names)
    if args.variance_scales is not None:
        s = calibration.parse_variance_scales(args.variance_scales, names)
    if args.calibration is not None:
        temps = calibration.load(args.calibration)["detectors"]
        scales = calibration.load_variance(args.calibration) or {}
        T = [float(temps.get(n, 1.0)) for n in names]
        s = [float(scales.get(n, 1.0)) for n in names]
    return T, s


def table(report, names):
    f = lambda x: f"{x:9.6f}"      # noqa: E731
    conf = f"{100 * report['confidence']:g} %"
    lines = []
    for key, title in zip("ab", names):
        if key not in report:
            continue
        r = report[key]
        lines.append(f"{title} (T = {r['temperature']:.6g}, s = {r['variance_scale']:.6g}): PDQ, {conf} interval, standard error; mean pair / "
                     "spatial / label / foreground / background quality of the true positives; TP FP FN")
        for row in r["thresholds"]:
            lines.append(f"  score >= {row['score_thresh']:<6g}{f(row['pdq']['point'])}  [{f(row['pdq']['lo'])}, {f(row['pdq']['hi'])}]  se "
                         f"{f(row['pdq']['se'])}  {f(row['pair_quality'])} {f(row['spatial'])} {f(row['label'])} {f(row['foreground'])} "
                         f"{f(row['background'])}  {row['tp']:d} {row['fp']:d} {row['fn']:d}")
    if "paired" in report:
        lines.append(f"{names[1]} - {names[0]}: PDQ difference, {conf} interval, standard error, two-sided p")
        for row in report["paired"]:
            d = row["pdq"]
            lines.append(f"  score >= {row['score_thresh']:<6g}{f(d['point'])}  [{f(d['lo'])}, {f(d['hi'])}]  se {f(d['se'])}  p {d['p']:.4f}")
    return "\n".join(lines)


def main(cmd=None):
    args = parse(list(cmd) if cmd is not None else sys.argv[1:])
    records = load_coco_json(os.path.join(args.dataset_path, "FLIR_thermal_RGBT_pairs_val.json"),
                             os.path.join(args.dataset_path, "thermal_8_bit"))
    names = [detector_name(p) for p in args.predictions]
    preds = [read_j1(p) for p in args.predictions]
    if len(preds) == 2:
        bootstrap.check_same_images(preds[0]["image_id"], preds[1]["image_id"], args.predictions[0], args.predictions[1])
    T, s = resolve(args, names)
    report = {"predictions": list(args.predictions), "images": len(records), "score_thresh": args.thresholds, "support": args.support,
              "replicates": args.replicates, "seed": args.seed, "confidence": args.confidence,
              "resampling": "numpy.random.default_rng(seed).multinomial; row 0 = every image once"}
    runs = []
    for key, path, pred, t, v in zip("ab", args.predictions, preds, T, s):
        try:
            run = pdq.pdq_from_predictions(records, pred, t, v, args.thresholds, args.support, args.device, args.num_classes)
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None
        runs.append(run)
        rows = []
        for ti, th in enumerate(run["score_thresh"]):
            summ = run["summary"][ti]
            boot = pdq.bootstrap_pdq(run["per_image"][ti], None, args.replicates, args.seed, args.confidence)["a"]
            rows.append({"score_thresh": th, "pdq": boot, **{k: summ[k] for k in ("pair_quality", "spatial", "label", "foreground", "background")},
                         "tp": int(summ["tp"]), "fp": int(summ["fp"]), "fn": int(summ["fn"]), "detections": run["detections"][ti]})
        report[key] = {"temperature": t, "variance_scale": v, "num_classes": run["num_classes"], "flags": run["flags"],
                       "live_ground_truths": run["live_ground_truths"], "thresholds": rows}
    if len(runs) == 2:
        report["paired"] = [{"score_thresh": th, "pdq": pdq.bootstrap_pdq(runs[0]["per_image"][ti], runs[1]["per_image"][ti], args.replicates,
                                                                         args.seed, args.confidence)["paired"]}
                            for ti, th in enumerate(args.thresholds)]
    print(f"{len(records)} images, {args.replicates - 1} resamples (seed {args.seed}), support {args.support:g}")
    print(table(report, [os.path.basename(p) for p in args.predictions]))
    for key, path in zip("ab", args.predictions):
        if key in report and (report[key]["flags"]["excluded_detections"] or report[key]["flags"]["ignored_ground_truths"]):
            fl = report[key]["flags"]
            print(f"{path}: {fl['excluded_detections']} detections excluded (a non-finite coordinate, no width or height, a bad variance: false "
                  f"positives), {fl['ignored_ground_truths']} ground truths ignored (crowd, no pixel, a class outside the columns)")
        if key in report and report[key]["flags"]["unscored_rows"]:
            print(f"{path}: {report[key]['flags']['unscored_rows']} rows have a NaN score: they pass no threshold and are not counted")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
        print("report:", args.out)
    return report


if __name__ == "__main__":
    main()
