"""Is a difference of two AP figures real?  Percentile-bootstrap intervals of the COCO statistics over the validation images.

    python -m proben_amd.cli.bootstrap_ap --dataset_path DATA/FLIR/val --predictions A.json [B.json] \\
        [--replicates 2000] [--seed 0] [--confidence 0.95] [--out report.json]

The images are resampled with replacement --replicates times (numpy.random.default_rng(--seed), multinomial) and the 12 statistics of
COCOeval.summarize plus AP per class are recomputed for every resample: matching once on the host, accumulate per replicate on the GPU
(proben_amd.bootstrap).  Printed per statistic: the evaluator's own figure, the percentile interval at
--confidence and the bootstrap standard error.  With two files both are evaluated under the SAME resamples, and the paired difference
B - A is printed with its interval and the two-sided bootstrap p-value 2 min(P(d* <= 0), P(d* >= 0)).
A file is a prediction file of the detectors' schema: what cli/save_predictions writes, or the fused detections of
demo_probEn --write_fused.  Its rows go through FLIREvaluator's class whitelist and XYXY -> XYWH conversion.  Two files must list the
same images.  The interval describes the sampling of images, given the detector: it says nothing about retraining.
"""
import argparse
import json
import os
import sys

from .. import bootstrap
from ..evaluation import prediction_file_results
from ..late_fusion import read_j1


def parse(argv):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--predictions", nargs="+", required=True, help="one prediction file, or two for the paired difference B - A")
    p.add_argument("--dataset_path", required=True, help="FLIR val folder (FLIR_thermal_RGBT_pairs_val.json)")
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
    return args


def load(gt_json, paths):
    """The COCO result rows of one or two prediction files over gt_json; ValueError when they do not list the same images or list
    images the dataset does not have."""
    preds = [read_j1(p) for p in paths]
    known = {im["id"] for im in gt_json["images"]}
    for path, pred in zip(paths, preds):
        extra = [i for i in pred["image_id"] if i not in known]
        if extra:
            raise ValueError(f"{path}: {len(extra)} images the dataset does not have (image id {extra[0]} is one)")
    if len(preds) == 2:
        bootstrap.check_same_images(preds[0]["image_id"], preds[1]["image_id"], paths[0], paths[1])
    return [prediction_file_results(pred, gt_json) for pred in preds]


def table(report, names):
    pct = lambda x: f"{100 * x:8.3f}"      # noqa: E731
    lines = []
    for key, title in (("a", names[0]),) + ((("b", names[1]),) if "b" in report else ()):
        lines.append(f"{title}: figure, {100 * report['confidence']:g} % interval, standard error (x 100)")
        rows = list(report[key]["stats"].items()) + [("AP-" + c, r) for c, r in report[key]["class_ap"].items()]
        for name, r in rows:
            lines.append(f"  {name:<8}{pct(r['point'])}  [{pct(r['lo'])}, {pct(r['hi'])}]  se {pct(r['se'])}")
    if "paired" in report:
        lines.append(f"{names[1]} - {names[0]}: difference, {100 * report['confidence']:g} % interval, standard error (x 100), two-sided p")
        rows = list(report["paired"]["stats"].items()) + [("AP-" + c, r) for c, r in report["paired"]["class_ap"].items()]
        for name, r in rows:
            lines.append(f"  {name:<8}{pct(r['point'])}  [{pct(r['lo'])}, {pct(r['hi'])}]  se {pct(r['se'])}  p {r['p']:.4f}")
    return "\n".join(lines)


def main(cmd=None):
    args = parse(list(cmd) if cmd is not None else sys.argv[1:])
    with open(os.path.join(args.dataset_path, "FLIR_thermal_RGBT_pairs_val.json")) as f:
        gt_json = json.load(f)
    results = load(gt_json, args.predictions)
    report = bootstrap.bootstrap_ap(gt_json, results[0], results[1] if len(results) > 1 else None, replicates=args.replicates,
                                    seed=args.seed, confidence=args.confidence, device=args.device)
    names = {c["id"]: c.get("name", str(c["id"])) for c in gt_json.get("categories", [])}
    report["category_names"] = {str(c): names.get(c, str(c)) for c in report["categories"]}
    report["predictions"] = list(args.predictions)
    print(f"{len(gt_json['images'])} images, {args.replicates - 1} resamples (seed {args.seed})")
    print(table(report, [os.path.basename(p) for p in args.predictions]))
    for key, path in zip("ab", args.predictions):
        if report[key]["mixed_score_ties"]:
            print(f"{path}: {report[key]['mixed_score_ties']} pairs of detections tie in score inside one image and differ in what they "
                  "count as: a resample weighs them one by one where a duplicated image would repeat the pair (DESIGN.md section 27)")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
        print("report:", args.out)
    return report


if __name__ == "__main__":
    main()
