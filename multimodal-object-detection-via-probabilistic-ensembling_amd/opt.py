"""The ProbEn CLI flag set (detectron2/utils/opt.py:3-19; the reference uses configargparse, plain argparse
here) plus the MI355X additions --device / --batch / --world-size and demo_probEn's --one-pass mode."""
import argparse


def config_parser(cmd=None):
    p = argparse.ArgumentParser()
    p.add_argument("--outfolder", type=str, default="out", help="name of output folder")
    p.add_argument("--dataset_name", type=str, default="FLIR", help="name of dataset")
    p.add_argument("--dataset_path", type=str, default=None, help="path to dataset")
    p.add_argument("--prediction_path", type=str, default=None, help="path to model predictions")
    p.add_argument("--fusion_method", type=str, default="middle_fusion",
                   choices=["rgb_only", "thermal_only", "early_fusion", "middle_fusion"], help="Which fusion method to use?")
    p.add_argument("--model_path", type=str, default=None, help="path to trained model")
    p.add_argument("--score_fusion", type=str, default="probEn", choices=["avg", "max", "probEn", "probEn-log", "wbf"],
                   help="Which fusion method to use?  probEn-log (not in the reference): ProbEn on log_softmax(class_logits / T) with the "
                        "background column kept - needs prediction files with class_logits.  wbf (not in the reference; with "
                        "--box_fusion wbf): weighted boxes fusion, Solovyev et al. 2021")
    p.add_argument("--box_fusion", type=str, default="v-avg", choices=["avg", "s-avg", "v-avg", "argmax", "c-avg", "wbf"],
                   help="Which fusion method to use?  c-avg (not in the reference; --score_fusion probEn-log with --box_correlation or a "
                        "--calibration file that carries one): the generalised-least-squares mean under correlated box errors.  wbf "
                        "(with --score_fusion wbf): weighted boxes fusion - not the reference's weighted_box_fusion, which is s-avg")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--world-size", type=int, default=1,
                   help="ranks (one per GPU) the dataset is sharded over; > 1 re-launches the driver under torch.distributed.run (launch.py)")
    p.add_argument("--detectors", type=str, default="thermal_only,early_fusion,middle_fusion",
                   help="comma separated prediction files to fuse, in order (val_<name>_predictions.json)")
    # one-pass mode of demo_probEn (stream.py -> FramePairPipeline -> ProbEn -> FLIREvaluator, no prediction files in between)
    p.add_argument("--one-pass", action="store_true",
                   help="demo_probEn: run the --detectors on the frame pairs themselves (decoded by --workers processes) and fuse on the GPU")
    p.add_argument("--model_paths", type=str, default=None,
                   help="--one-pass: comma separated weights, one per --detectors entry (.pth or synthetic://<seed>)")
    p.add_argument("--workers", type=int, default=4, help="--one-pass: JPEG decode processes (0 = in-process, at most 15)")
    p.add_argument("--write-predictions", action="store_true",
                   help="--one-pass: also write every detector's val_<method>_predictions.json to --prediction_path (or --outfolder)")
    # temperature calibration of the detectors' posteriors ahead of ProbEn (calibration.py)
    cal = p.add_mutually_exclusive_group()
    cal.add_argument("--temperatures", type=str, default=None,
                     help="demo_probEn: one softmax temperature per --detectors entry, 'a,b[,c]' by position or 'name=a,name=b' by name")
    cal.add_argument("--calibration", type=str, default=None,
                     help="demo_probEn: calibration file written by cli/fit_temperature (temperatures looked up by detector name)")
    p.add_argument("--variance_scales", type=str, default=None,
                   help="demo_probEn: one box-variance scale per --detectors entry, 'a,b[,c]' by position or 'name=a,name=b' by name "
                        "(variance' = s * variance, the weights of --box_fusion v-avg); default: the calibration file's variance_scales "
                        "if it has them (fit_temperature --with-variance), else none")
    p.add_argument("--class_prior", type=str, default=None,
                   help="demo_probEn --score_fusion probEn-log: class prior 'p_0,...,p_K' (K + 1 numbers > 0, background last; normalised); "
                        "default: the calibration file's class_prior if it has one, else uniform")
    p.add_argument("--pool_weights", type=str, default=None,
                   help="demo_probEn --score_fusion probEn-log: one pooling weight per --detectors entry, 'a,b[,c]' by position or "
                        "'name=a,name=b' by name (a_j = sum_t w_d(t) log p_t[j]: the logarithmic opinion pool); default: the calibration "
                        "file's pool_weights if it has them (fit_temperature --with-pool-weights), else the plain product")
    p.add_argument("--presence", type=str, default=None, metavar="TEXT",
                   help="demo_probEn --score_fusion probEn-log (either route): presence evidence, one row of K + 1 numbers per presence "
                        "pattern, 'thermal_only=a:b:c:d,thermal_only+early_fusion=a:b:c:d' (detector names joined by +, background "
                        "last; patterns not listed get zeros); default: the calibration file's presence table if it has one "
                        "(fit_temperature --with-presence), else none")
    p.add_argument("--box_correlation", type=str, default=None, metavar="TEXT",
                   help="demo_probEn --score_fusion probEn-log --box_fusion c-avg (either route): the correlation of the detectors' "
                        "normalised box errors, 'thermal_only:early_fusion=0.6,thermal_only:thermal_only=0.2' (one entry per detector "
                        "pair, the same name twice = two rows of one detector; pairs not listed get 0), or a bare number for the one "
                        "pair of two detectors; default: the calibration file's box_correlation (fit_temperature --with-box-correlation)")
    p.add_argument("--wbf_weights", type=str, default=None,
                   help="demo_probEn --score_fusion wbf --box_fusion wbf (either route): one detector weight per --detectors entry, "
                        "'a,b[,c]' by position or 'name=a,name=b' by name (a row counts with score * weight); default 1 each")
    p.add_argument("--wbf_iou", type=float, default=0.55,
                   help="demo_probEn --score_fusion wbf --box_fusion wbf: the IoU above which a row joins a cluster's fused box "
                        "(the method's published default)")
    p.add_argument("--wbf_skip", type=float, default=0.0,
                   help="demo_probEn --score_fusion wbf --box_fusion wbf: rows with score * weight below this are skipped")
    p.add_argument("--write_fused", type=str, default=None, metavar="FILE",
                   help="demo_probEn --score_fusion probEn-log (either route): write the fused detections as a prediction file (the "
                        "schema of val_<method>_predictions.json: class_logits = the fused log-posterior, vars = the fused box's "
                        "variance), a detector's file for a later fusion, fit_temperature or calibration_report.  With --score_fusion "
                        "wbf: boxes, scores and classes with class_logits [], probs [], vars [1.0] - a file for bootstrap_ap")
    p.add_argument("--var_voting", type=float, nargs="?", const=0.025, default=None, metavar="SIGMA_T",
                   help="save_predictions, demo_probEn --one-pass: variance voting inside every detector after its box-head NMS "
                        "(PROBEN.VAR_VOTING, DESIGN.md section 31): a kept box becomes the mean of its overlapping same-class candidates, "
                        "weighted by exp(-(1 - IoU)^2 / SIGMA_T) / variance; SIGMA_T defaults to 0.025")
    args = p.parse_args(cmd) if cmd is not None else p.parse_args()
    if args.var_voting is not None and not (0.0 < args.var_voting < float("inf")):
        p.error(f"--var_voting takes a finite SIGMA_T > 0 (got {args.var_voting})")
    wbf = args.score_fusion == "wbf"
    if wbf != (args.box_fusion == "wbf"):
        p.error(f"--score_fusion wbf and --box_fusion wbf go together (got {args.score_fusion}, {args.box_fusion}): weighted boxes "
                "fusion is one method")
    if args.wbf_weights is not None and not wbf:
        p.error(f"--wbf_weights belongs to --score_fusion wbf --box_fusion wbf (got {args.score_fusion}, {args.box_fusion})")
    if wbf and args.variance_scales is not None:
        p.error("--variance_scales belongs to the ProbEn box rules (got wbf): weighted boxes fusion reads no variance")
    if args.write_fused is not None and args.score_fusion not in ("probEn-log", "wbf"):
        p.error(f"--write_fused belongs to --score_fusion probEn-log or wbf (got {args.score_fusion}): the other score fusions form no "
                "posterior")
    if args.box_fusion == "c-avg" and args.score_fusion != "probEn-log":
        p.error(f"--box_fusion c-avg belongs to --score_fusion probEn-log (got {args.score_fusion})")
    if args.box_correlation is not None and args.box_fusion != "c-avg":
        p.error(f"--box_correlation belongs to --box_fusion c-avg (got {args.box_fusion})")
    if args.presence is not None and args.score_fusion != "probEn-log":
        p.error(f"--presence belongs to --score_fusion probEn-log (got {args.score_fusion})")
    if args.pool_weights is not None and args.score_fusion != "probEn-log":
        p.error(f"--pool_weights belongs to --score_fusion probEn-log (got {args.score_fusion})")
    if args.class_prior is not None:
        if args.score_fusion != "probEn-log":
            p.error(f"--class_prior belongs to --score_fusion probEn-log (got {args.score_fusion})")
        from .calibration import parse_class_prior
        try:
            parse_class_prior(args.class_prior)
        except ValueError as e:
            p.error(str(e))
    return args
