"""Counterpart of demo/FLIR/demo_probEn.py:300-342: read val_<method>_predictions.json files, ProbEn-fuse
them on the GPU, evaluate with FLIREvaluator.

    python -m proben_amd.cli.demo_probEn --dataset_path DATA/FLIR/val --prediction_path out/ \
        --score_fusion probEn --box_fusion v-avg [--detectors thermal_only,early_fusion,middle_fusion]

--one-pass runs the detectors too, in the same process: frame pairs stream from disk (stream.FlirPairLoader, --workers decode
processes) through FramePairPipeline and ProbEn to FLIREvaluator, with no prediction files in between (--write-predictions
still writes them, so the two-stage route can be replayed):

    python -m proben_amd.cli.demo_probEn --one-pass --dataset_path DATA/FLIR/val --detectors thermal_only,early_fusion \
        --model_paths thermal.pth,early.pth [--workers 4] [--batch 32] [--write-predictions --prediction_path out/]

Either route takes per-detector softmax temperatures (calibration.py): --temperatures 1.4,0.9 (by position) or
--temperatures thermal_only=1.4,early_fusion=0.9 (by name), or --calibration FILE written by cli/fit_temperature.  ProbEn then fuses
softmax(class_logits / T) instead of the detectors' own prob_score; the result names the temperatures used.

--score_fusion probEn-log (either route) fuses log_softmax(class_logits / T) over all K + 1 columns, background included, and
normalises in the log domain: ProbEn's rule, defined where probEn's `1 - sum(p)` background gives NaN.  T = 1 without
--temperatures / --calibration.  --class_prior 0.2,0.5,0.2,0.1 (K + 1 numbers, background last) divides the prior out
(p(y)^(m-1) for a cluster of m rows); without the flag a --calibration file written by `fit_temperature --with-prior` supplies it.

--variance_scales 0.5,2 (by position) or thermal_only=0.5,early_fusion=2 (by name) multiplies every detector's box variances by its
scale ahead of the fusion (either route): the 1 / variance weights of --box_fusion v-avg.  Without the flag a --calibration file
written by `fit_temperature --with-variance` supplies them, and the run says so; a file without them changes nothing.

--pool_weights 0.6,0.5 (by position) or thermal_only=0.6,early_fusion=0.5 (by name), with --score_fusion probEn-log on either route:
one exponent per detector inside the fusion (the logarithmic opinion pool, pe_proben_fuse_batch_pooled) for detectors that share
evidence.  Without the flag a --calibration file that carries "pool_weights" supplies them; 1,1 is the plain product bit for bit.

--presence 'thermal_only=-0.1:-0.9:0:0,early_fusion=-1.3:0:0.3:0,thermal_only+early_fusion=1.6:1.5:1.1:0', with --score_fusion
probEn-log on either route: presence evidence (pe_proben_fuse_batch_presence), one row of K + 1 log-evidence values (background last)
per presence pattern - the detectors that put a row into the cluster, names joined by + -, added to the fused columns; patterns not
listed get zeros.  Detections only one detector made, and images on which one detector fired, are rescored too.  Without the flag a
--calibration file that carries "presence" (fit_temperature --with-presence) supplies the table.  With --write_fused the fused
log-posterior includes the presence term.

--box_fusion c-avg, with --score_fusion probEn-log on either route: the generalised-least-squares mean of a cluster's boxes under
correlated box errors (pe_box_gls_batch after the fusion).  --box_correlation 0.6 (two detectors: their one pair) or
thermal_only:early_fusion=0.6,thermal_only:thermal_only=0.2 (one entry per detector pair; the same name twice is the correlation of
two rows of one detector; pairs not listed get 0); without the flag a --calibration file that carries "box_correlation"
(fit_temperature --with-box-correlation) supplies the matrix, and a run without either is refused.  With --write_fused the file's vars
are the variance the correlated mean really has.

--write_fused FILE, with --score_fusion probEn-log on either route: the fused detections leave as a prediction file of the schema the
detectors' files have (late_fusion.fused_to_j1): class_logits = the fused log-posterior over all K + 1 columns, probs / scores / classes,
vars = the variance of the fused box under its box rule.  Fused rows whose class is the background column are not detections and are
not written; the run prints how many.  The file is a detector's file: name it val_<name>_predictions.json and list <name> in
--detectors to fuse it with a further detector, or hand it to fit_temperature / calibration_report.

--score_fusion wbf --box_fusion wbf (either route): weighted boxes fusion (Solovyev, Wang, Gabruseva 2021; pe_wbf_fuse_batch), the
baseline ProbEn is compared against - every row is matched against the running fused box of each cluster of its class, and a cluster
fewer detectors than the weights' sum agree on is scored down.  --wbf_weights 1,0.7 (by position) or thermal_only=1,early_fusion=0.7 (by
name), --wbf_iou (default 0.55), --wbf_skip (default 0).  There is no case split: an image on which one detector fired is fused too.
--temperatures / --calibration still rebuild the scores; every other calibration option is refused.  --write_fused FILE writes the
fused rows with class_logits [], probs [], vars [1.0] (late_fusion.wbf_to_j1) and prints how many rows were skipped:
`bootstrap_ap val_thermal_only_predictions.json FILE` then compares the two.

--var_voting [SIGMA_T], with --one-pass (the route that runs detectors; it changes nothing without it): every detector votes its kept
boxes after its box-head NMS (PROBEN.VAR_VOTING / VAR_VOTING_SIGMA_T; SIGMA_T defaults to 0.025).  ProbEn then
fuses ordinary detections.  On the two-stage route give the flag to save_predictions.
"""
import json
import os
import sys

from .. import comm, get_cfg, launch
from ..data import DatasetCatalog, register_coco_instances
from ..evaluation import FLIREvaluator
from ..late_fusion import apply_late_fusion_and_evaluate, read_j1, shard_j1
from ..opt import config_parser
from ..options import FusionOptions


def main(cmd=None):
    argv = list(cmd) if cmd is not None else sys.argv[1:]
    args = config_parser(argv)
    # --world-size N: the image list is cut into N contiguous blocks, every rank fuses its block on its own GPU and the
    # evaluator gathers the fused rows to rank 0 (one tensor all-gather over RCCL)
    launch.maybe_self_launch(args.world_size, argv, module="proben_amd.cli.demo_probEn", device=args.device)
    rank, world, dev = launch.init_distributed(args.device, expect_world=args.world_size)
    names = [n for n in args.detectors.split(",") if n]
    assert 2 <= len(names) <= 3, "--detectors takes 2 or 3 names"
    opts = FusionOptions.from_args(args, names, say=print if comm.is_main_process() else None)
    if args.one_pass:
        return one_pass(args, names, world, dev, opts)
    files = [os.path.join(args.prediction_path, f"val_{n}_predictions.json") for n in names]
    if comm.is_main_process():
        for i, f in enumerate(files):
            print(f"detection file {i + 1}:", f)
        os.makedirs(args.outfolder, exist_ok=True)
    val_json = os.path.join(args.dataset_path, "FLIR_thermal_RGBT_pairs_val.json")
    cfg = _register(args)
    dets = [read_j1(f) for f in files]
    # the files are sharded with ONE index range: they must list the same images in the same order (the reference pairs by det_2's
    # position too, demo_probEn.py:205-233, and silently mis-pairs otherwise)
    for f, d in zip(files[:-1], dets[:-1]):
        if d["image_id"] != dets[-1]["image_id"]:
            raise ValueError(f"{f} and {files[-1]} do not list the same images in the same order ({len(d['image_id'])} vs "
                             f"{len(dets[-1]['image_id'])} entries): late fusion pairs detections by position")
    mine = comm.shard_range(len(dets[-1]["image"]))
    dets = [shard_j1(d, mine) for d in dets]
    with open(val_json) as f:
        hw = {im["id"]: (im["height"], im["width"]) for im in json.load(f)["images"]}
    main_rank = comm.is_main_process()
    ev = FLIREvaluator(args.dataset_name, cfg, world > 1 or comm.is_distributed(), output_dir=args.outfolder if main_rank else None, save_eval=main_rank,
                       out_eval_path=os.path.join(args.outfolder, "FLIR_probEn_eval.json"))
    _warn_fitted(opts, [i for d in dets for i in d["image_id"]])
    fused = [] if args.write_fused else None
    stats = {"skipped": 0}
    res = apply_late_fusion_and_evaluate(cfg, ev, dets[0], dets[1], [args.score_fusion, args.box_fusion],
                                         det_3=dets[2] if len(dets) > 2 else "", image_hw=hw, device=str(dev), names=files,
                                         fused_out=fused, options=opts, iou_thresh=args.wbf_iou if opts.wbf else None, stats=stats)
    res.update(opts.named(names))
    if opts.wbf:
        res["wbf_iou"] = args.wbf_iou
    if fused is not None:
        from ..late_fusion import fused_to_j1, wbf_to_j1
        part = (wbf_to_j1(dets, fused), stats["skipped"]) if opts.wbf else fused_to_j1(dets, fused)
        _write_fused(args.write_fused, [part], main_rank, "rows skipped" if opts.wbf else "background rows dropped")
    if main_rank:
        print(json.dumps(res, indent=1))
    if comm.is_distributed():
        launch.shutdown()
    return res


def _write_fused(path, parts, main_rank, left_out="background rows dropped"):
    """--write_fused: this rank's (prediction dict, dropped rows) parts, in image order, gathered to rank 0 (rank order == dataset
    order) and written as one prediction file.  left_out words the count: "wbf" drops no background rows, it skips input rows."""
    from ..late_fusion import J1_KEYS, write_j1
    gathered = comm.gather(parts, dst=0)
    if not main_rank:
        return
    parts = [p for g in gathered for p in g]
    pred = {k: sum((p[k] for p, _ in parts), []) for k in J1_KEYS}
    folder = os.path.dirname(path)
    if folder:
        os.makedirs(folder, exist_ok=True)
    write_j1(path, pred)
    print(f"fused detections: {path}: {sum(len(r) for r in pred['scores'])} rows on {len(pred['image'])} images written, "
          f"{sum(d for _, d in parts)} {left_out}")


def _warn_fitted(opts, image_ids):
    """The calibration file records the images its temperatures were fitted on: say so when the evaluation includes them."""
    seen = opts.fitted & set(image_ids)
    if seen and comm.is_main_process():
        print(f"warning: {len(seen)} of the evaluated images were used to fit the temperatures (the calibration file's holdout split): "
              "the result is optimistic on them")


def _register(args):
    val_json = os.path.join(args.dataset_path, "FLIR_thermal_RGBT_pairs_val.json")
    register_coco_instances(args.dataset_name, {}, val_json, os.path.join(args.dataset_path, "thermal_8_bit"))
    DatasetCatalog.get(args.dataset_name)
    cfg = get_cfg()
    cfg.OUTPUT_DIR = args.outfolder
    cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.5
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = 3
    cfg.DATASETS.TEST = (args.dataset_name,)
    return cfg


def detector_cfgs(args, names, paths, device_type="cuda"):
    """--one-pass: one cfg per --detectors entry, as save_predictions.build_cfg builds it for that fusion method and weights file; the
    run's --var_voting [SIGMA_T] goes to every detector."""
    import argparse
    from .save_predictions import build_cfg
    cfgs = []
    for m, p in zip(names, paths):
        c = build_cfg(argparse.Namespace(fusion_method=m, model_path=p, var_voting=getattr(args, "var_voting", None)))
        c.MODEL.DEVICE = device_type
        cfgs.append(c)
    return cfgs


def one_pass(args, names, world, dev, opts):
    """`opts`: the run's FusionOptions (FusionOptions.from_args).  loader -> FramePairPipeline (one DefaultPredictor model per --detectors entry, cfg as save_predictions.build_cfg) ->
    ProbEn -> evaluation rows on the device (late_fusion.fused_rows_device) -> one all-gather -> FLIREvaluator on rank 0."""
    import time
    import torch
    from ..data import PairFrames, resize_shortest_edge_shape
    from ..late_fusion import fused_device_to_j1, fused_rows_device, predictions_to_j1, wbf_device_to_j1, write_j1
    from ..pipeline import FramePairPipeline, HostFeeder
    from ..predictor import DefaultPredictor
    from ..stream import FlirPairLoader, check_workers
    if "rgb_only" in names:
        raise ValueError("--one-pass does not run rgb_only: that detector sees the RGB frame at its own size while the frame-pair "
                         "pipeline shares one output size over its detectors.  Use the two-stage route: save_predictions per "
                         "detector, then demo_probEn without --one-pass.")
    paths = args.model_paths.split(",") if args.model_paths else [args.model_path] * len(names)
    if len(paths) != len(names):
        raise ValueError(f"--model_paths lists {len(paths)} weights for {len(names)} --detectors")
    workers = check_workers(args.workers)
    main_rank = comm.is_main_process()
    if main_rank:
        os.makedirs(args.outfolder, exist_ok=True)
    cfg = _register(args)
    preds = [DefaultPredictor(c) for c in detector_cfgs(args, names, paths, dev.type)]
    need_rgb = any(p.input_format in ("BGRT", "BGRTTT") for p in preds)
    loader = FlirPairLoader(args.dataset_path, args.batch, need_rgb=need_rgb, workers=workers)
    _warn_fitted(opts, [loader.items[i]["id"] for i in loader.mine])
    pipe = FramePairPipeline([p.model for p in preds], options=opts, iou_thresh=args.wbf_iou if opts.wbf else None)
    fused_parts = []
    j1 = [([], [], []) for _ in names]       # per detector: names, ids, instances
    rows = []
    feeder, feed_key, host = None, None, None
    pending = None
    timed = {"pairs": 0, "t0": None, "wait0": 0.0}

    def finish(p):
        dets, fused, batch = p
        rows.append(fused_rows_device(fused, batch.ids))        # the batch's one host synchronisation
        if args.write_fused:
            fused_parts.append((wbf_device_to_j1 if opts.wbf else fused_device_to_j1)(fused, batch.names, batch.ids))
        if args.write_predictions:
            for d, det, (nm, ids, insts) in zip(preds, dets, j1):
                nm += batch.names
                ids += batch.ids
                insts += [o["instances"] for o in d.model.to_instances(det)]

    for batch in loader:          # the loader assembles batch i+1 while the GPU runs batch i
        key = (tuple(batch.thermal.shape), None if batch.rgb is None else tuple(batch.rgb.shape))
        if pending is not None:
            finish(pending)          # waits for batch i only: batch i+1 is not enqueued yet
            pending = None
        if key != feed_key:
            # a new batch shape (a size change, the last partial batch): a fresh feeder, once nothing reads the old one's buffers
            torch.cuda.current_stream().synchronize()
            feeder = HostFeeder(lambda: host, dev)
            feed_key = key
        host = [batch.thermal] + ([batch.rgb] if batch.rgb is not None else [])
        up = feeder.next()
        h, w = batch.hw
        n = len(batch)
        frames = PairFrames(up[0], up[1] if len(up) > 1 else None)
        dets, fused = pipe([frames] * len(preds), [(h, w)] * n, resize_shortest_edge_shape(h, w, preds[0].min_size, preds[0].max_size))
        feeder.mark_consumed()
        pending = (dets, fused, batch)
        if timed["t0"] is None:      # the first batch warms up (allocations, tables): the timed part starts after it
            finish(pending)
            pending = None
            timed["t0"], timed["wait0"] = time.perf_counter(), loader.wait_s
        else:
            timed["pairs"] += n
    if pending is not None:
        finish(pending)
    wall = time.perf_counter() - timed["t0"] if timed["t0"] is not None else 0.0
    stats = {"pairs": len(loader), "timed_pairs": timed["pairs"], "pairs_per_s": timed["pairs"] / wall if wall > 0 else float("nan"),
             "decode_wait_fraction": (loader.wait_s - timed["wait0"]) / wall if wall > 0 else float("nan"), "workers": workers,
             "batch": args.batch, "world_size": world}
    mine = torch.cat(rows) if rows else torch.zeros((0, 7), dtype=torch.float64)
    all_rows = comm.gather_rows(mine)             # one padded all-gather on the device, rank order == dataset order
    if args.write_predictions:
        pdir = args.prediction_path or args.outfolder
        for m, (nm, ids, insts) in zip(names, j1):
            pred = predictions_to_j1(nm, ids, insts)
            gathered = comm.gather(pred, dst=0)
            if main_rank:
                os.makedirs(pdir, exist_ok=True)
                write_j1(os.path.join(pdir, f"val_{m}_predictions.json"), {k: sum((g[k] for g in gathered), []) for k in pred})
    if args.write_fused:
        _write_fused(args.write_fused, fused_parts, main_rank, "rows skipped" if opts.wbf else "background rows dropped")
    res = {}
    if main_rank:
        print(f"one-pass: {stats['timed_pairs']} pairs timed, {stats['pairs_per_s']:.1f} pairs/s, GPU side waited on decode "
              f"{100 * stats['decode_wait_fraction']:.1f}% of the wall time ({workers} workers, batch {args.batch}, {world} rank(s))")
        ev = FLIREvaluator(args.dataset_name, cfg, False, output_dir=args.outfolder, save_eval=True,
                           out_eval_path=os.path.join(args.outfolder, "FLIR_probEn_eval.json"))
        ev.process_rows(all_rows.numpy())
        res = ev.evaluate()
        res["one_pass"] = stats
        res.update(opts.named(names))
        if opts.wbf:
            res["wbf_iou"] = args.wbf_iou
        print(json.dumps(res, indent=1))
    if comm.is_distributed():
        launch.shutdown()
    return res


if __name__ == "__main__":
    main()
