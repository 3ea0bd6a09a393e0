"""Where does a difference of two AP50 figures come from?  TIDE error decomposition with paired bootstrap intervals.

    python -m proben_amd.cli.tide --dataset_path DATA/FLIR/val --predictions A.json [B.json] \\
        [--background_iou 0.1] [--replicates 2000] [--seed 0] [--confidence 0.95] [--out report.json]

Every false positive gets one type - Cls (right place, wrong class), Loc (right class, IoU in [--background_iou, 0.5)), Both, Dupe (its
object is already taken), Bkg - and every ground truth no error points at is Miss; each type is priced by dAP, the AP50 gained if that
type alone were repaired (FP: every false positive removed; FN: every unmatched ground truth removed).  The typing runs once on the GPU
and all nine variants are accumulated per resample of the images on the GPU (proben_amd.tide), under the resamples
of bootstrap_ap: numpy.random.default_rng(--seed), multinomial.  Printed per file: AP50, and per repair its count and dAP with the
percentile interval at --confidence and the bootstrap standard error.  With two files both are evaluated under the SAME resamples and
the paired difference B - A of every dAP is printed with its interval and the two-sided bootstrap p-value.
A file is a prediction file of the detectors' schema: what cli/save_predictions writes, the fused detections of demo_probEn
--write_fused, or a wbf file.  Two files must list the same images.  The rule is restated from Bolya et al. (ECCV 2020); the order in
which the types are tested (Loc, Cls, Dupe, Bkg, Both) is this project's definition.
"""
import argparse
import json
import os
import sys

from .. import tide
from .bootstrap_ap import load


def parse(argv):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--predictions", nargs="+", required=True, help="one prediction file, or two for the paired difference B - A")
    p.add_argument("--dataset_path", required=True, help="FLIR val folder (FLIR_thermal_RGBT_pairs_val.json)")
    p.add_argument("--background_iou", type=float, default=0.1, help="t_b: below it a box overlaps nothing")
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
    if not 0.0 <= args.background_iou < 0.5:
        p.error(f"--background_iou {args.background_iou} is not in [0, 0.5)")
    return args


def table(report, names):
    pct = lambda x: f"{100 * x:8.3f}"      # noqa: E731
    lines = []
    for key, title in (("a", names[0]),) + ((("b", names[1]),) if "b" in report else ()):
        r = report[key]["AP50"]
        lines.append(f"{title}: figure, {100 * report['confidence']:g} % interval, standard error (x 100)")
        lines.append(f"  {'AP50':<6}{'':>8}{pct(r['point'])}  [{pct(r['lo'])}, {pct(r['hi'])}]  se {pct(r['se'])}")
        for name, r in report[key]["repairs"].items():
            lines.append(f"  {'d' + name:<6}{r['count']:>8d}{pct(r['point'])}  [{pct(r['lo'])}, {pct(r['hi'])}]  se {pct(r['se'])}")
    if "paired" in report:
        lines.append(f"{names[1]} - {names[0]}: difference of dAP, {100 * report['confidence']:g} % interval, standard error (x 100), two-sided p")
        for name, r in report["paired"].items():
            lines.append(f"  {'d' + name:<6}{'':>8}{pct(r['point'])}  [{pct(r['lo'])}, {pct(r['hi'])}]  se {pct(r['se'])}  p {r['p']:.4f}")
    return "\n".join(lines)


def main(cmd=None):
    args = parse(list(cmd) if cmd is not None else sys.argv[1:])
    with open(os.path.join(args.dataset_path, "FLIR_thermal_RGBT_pairs_val.json")) as f:
        gt_json = json.load(f)
    results = load(gt_json, args.predictions)
    report = tide.tide(gt_json, results[0], results[1] if len(results) > 1 else None, replicates=args.replicates, seed=args.seed,
                       confidence=args.confidence, background_iou=args.background_iou, device=args.device)
    names = {c["id"]: c.get("name", str(c["id"])) for c in gt_json.get("categories", [])}
    report["category_names"] = {str(c): names.get(c, str(c)) for c in report["categories"]}
    report["predictions"] = list(args.predictions)
    print(f"{len(gt_json['images'])} images, {args.replicates - 1} resamples (seed {args.seed}), background IoU {args.background_iou:g}")
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
