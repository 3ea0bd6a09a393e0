"""Is a difference of two KAIST miss rates real?  Percentile-bootstrap intervals of the log-average miss rate over the test images.

    python -m proben_amd.cli.bootstrap_lamr --annotation_json GT.json --results A.txt [B.txt] [--replicates 2000] [--seed 0] \\
        [--confidence 0.95] [--setups 0[,1,2,3]] [--fix-row-index] [--day_frames 1455] [--stratified] [--out report.json]

The images are resampled with replacement --replicates times (numpy.random.default_rng(--seed), multinomial; --stratified: day and night
each to its own size) and MR, the miss rates at the nine FPPI references and the recall are recomputed for every resample, per setup
(0 = Reasonable) and subset (all / day / night): matching once on the host, accumulate per replicate on the GPU
(proben_amd.lamr_bootstrap).  Printed per setup and subset: the evaluator's own MR, the percentile interval at
--confidence, the bootstrap standard error and the recall.  With two files both are evaluated under the SAME resamples, and the paired
difference B - A is printed with its interval and the two-sided bootstrap p-value 2 min(P(d* <= 0), P(d* >= 0)).
A file is what KAIST.loadRes reads: the demo's text rows `<1-based frame index>,x,y,w,h,score` or a COCO-result json.  The interval
describes the sampling of images, given the detector: it says nothing about retraining.
"""
import argparse
import json
import os
import sys

from .. import lamr_bootstrap
from ..evalKAIST.evaluation_script import DAY_FRAMES, KAISTParams


def parse(argv):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--annotation_json", required=True, help="KAIST_annotation.json (COCO-style), as demo_LAMR_KAIST takes it")
    p.add_argument("--results", nargs="+", required=True, help="one result file, or two for the paired difference B - A")
    p.add_argument("--replicates", type=int, default=2000, help="resamples of the image list")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--confidence", type=float, default=0.95, help="coverage of the percentile interval")
    p.add_argument("--setups", default="0", help="comma-separated evaluation setups: 0 Reasonable, 1 Reasonable_small, 2 Reasonable_occ=heavy, 3 All")
    p.add_argument("--fix-row-index", action="store_true", help="evaluator: every kept detection's own overlaps (evalKAIST/evaluation_script.py)")
    p.add_argument("--day_frames", type=int, default=DAY_FRAMES, help="the first this many image ids are the day subset")
    p.add_argument("--stratified", action="store_true", help="resample day and night each to its own size")
    p.add_argument("--out", default=None, help="write the report as JSON")
    p.add_argument("--device", default="cuda")
    args = p.parse_args(argv)
    if not 1 <= len(args.results) <= 2:
        p.error(f"--results lists {len(args.results)} files: one, or two for the paired difference")
    if args.replicates < 2:
        p.error(f"--replicates {args.replicates} is below 2")
    if not 0.0 < args.confidence < 1.0:
        p.error(f"--confidence {args.confidence} is not in (0, 1)")
    if args.day_frames < 0:
        p.error(f"--day_frames {args.day_frames} is negative")
    try:
        args.setups = tuple(int(s) for s in args.setups.split(","))
    except ValueError:
        p.error(f"--setups {args.setups}: comma-separated integers")
    n = len(KAISTParams().SetupLbl)
    if not args.setups or any(not 0 <= s < n for s in args.setups):
        p.error(f"--setups {args.setups}: each in [0, {n})")
    return args


def table(report, names):
    pct = lambda x: f"{100 * x:8.3f}"      # noqa: E731
    labels = KAISTParams().SetupLbl
    lines = []
    for key, title in (("a", names[0]),) + ((("b", names[1]),) if "b" in report else ()):
        lines.append(f"{title}: MR, {100 * report['confidence']:g} % interval, standard error, recall (x 100)")
        for s, subsets in report[key]["setups"].items():
            for sub, r in subsets.items():
                m = r["MR"]
                lines.append(f"  {labels[int(s)]:<22}{sub:<6}{pct(m['point'])}  [{pct(m['lo'])}, {pct(m['hi'])}]  se {pct(m['se'])}  "
                             f"recall {pct(r['recall']['point'])}  ({m['replicates']} resamples)")
    if "paired" in report:
        lines.append(f"{names[1]} - {names[0]}: MR difference, {100 * report['confidence']:g} % interval, standard error (x 100), two-sided p")
        for s, subsets in report["paired"]["setups"].items():
            for sub, r in subsets.items():
                m = r["MR"]
                lines.append(f"  {labels[int(s)]:<22}{sub:<6}{pct(m['point'])}  [{pct(m['lo'])}, {pct(m['hi'])}]  se {pct(m['se'])}  p {m['p']:.4f}")
    return "\n".join(lines)


def main(cmd=None):
    args = parse(list(cmd) if cmd is not None else sys.argv[1:])
    with open(args.annotation_json) as f:
        annotation = json.load(f)
    report = lamr_bootstrap.bootstrap_lamr(annotation, args.results[0], args.results[1] if len(args.results) > 1 else None,
                                           replicates=args.replicates, seed=args.seed, confidence=args.confidence, setups=args.setups,
                                           fix_row_index=args.fix_row_index, day_frames=args.day_frames, stratified=args.stratified,
                                           device=args.device)
    report["results"] = list(args.results)
    print(f"{report['images']} images ({report['day_frames']} day), {args.replicates - 1} resamples (seed {args.seed}"
          f"{', stratified' if args.stratified else ''})")
    print(table(report, [os.path.basename(p) for p in args.results]))
    for key, path in zip("ab", args.results):
        for s, n in report[key]["mixed_score_ties"].items():
            if n:
                print(f"{path} (setup {s}): {n} pairs of detections tie in score inside one image and differ in what they count as: a "
                      "resample weighs them one by one where a duplicated image would repeat the pair (DESIGN.md section 28)")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
        print("report:", args.out)
    return report


if __name__ == "__main__":
    main()
