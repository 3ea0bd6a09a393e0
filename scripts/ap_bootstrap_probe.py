"""Cost of the AP bootstrap (profiles/ap_bootstrap.txt) on a FLIR-sized synthetic case: 1 366 images, 3 classes,
about 100 detections per image (proben_amd.synthetic.synth_detections, two detectors' rows together), ground truth = a detector's
confident rows.  Times pe_ap_bootstrap at B = 2 000 replicates over the 18 summary cells (2 warm-up launches, then 10 launches between
device events: the median), and the native evaluator (pe_cocoeval_bbox: matching AND accumulate, all threads) on the explicitly
duplicated dataset of a few dozen of the same replicates, scaled to B.  Checks on the way that replicate 0 is the evaluator's table.

    python scripts/ap_bootstrap_probe.py [--images 1366] [--replicates 2000] [--cpu-replicates 24]
    rocprofv3 --kernel-trace --stats -d OUT -o ap_bootstrap --output-format csv -- python scripts/ap_bootstrap_probe.py --cpu-replicates 0
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proben_amd  # noqa: E402,F401
from proben_amd import _lib, bootstrap  # noqa: E402
from proben_amd.evaluation import COCOevalBBox  # noqa: E402
from proben_amd.synthetic import synth_detections  # noqa: E402


def dataset(n_images, seed=27):
    xywh = lambda b: [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]      # noqa: E731
    anns, res = [], []
    for i, (d0, d1) in enumerate(synth_detections(n_images, seed, kdet=2, nmax=100, K=3), 1):
        for j, (box, s, c) in enumerate(zip(d0["bbox"], d0["score"], d0["class"])):
            if s > 0.9 and j % 2 == 0:
                w = xywh(box)
                anns.append({"id": len(anns) + 1, "image_id": i, "category_id": int(c) + 1, "bbox": w, "area": w[2] * w[3], "iscrowd": 0})
        for d in (d0, d1):
            res += [{"image_id": i, "category_id": int(c) + 1, "bbox": xywh(b), "score": float(s)} for b, s, c in zip(d["bbox"], d["score"], d["class"])]
    gt = {"images": [{"id": i, "height": 512, "width": 640} for i in range(1, n_images + 1)], "annotations": anns,
          "categories": [{"id": c} for c in (1, 2, 3)]}
    return gt, res


def duplicated_arrays(args, mult):
    """The arrays of COCOevalBBox._native_arrays for the dataset with mult[i] adjacent copies of image i."""
    out = list(args)
    start = np.concatenate([[0], np.cumsum(mult)])
    for img_at, rows_at, n_at in ((0, (1, 2, 3, 4, 5), 6), (7, (8, 9, 10), 11)):
        img = args[img_at]
        reps = mult[img]
        copy = np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps)
        out[img_at] = (np.repeat(start[img], reps) + copy).astype(np.int32)
        for r in rows_at:
            out[r] = np.ascontiguousarray(np.repeat(args[r], reps, axis=0))
        out[n_at] = int(reps.sum())
    out[5] = np.arange(1, out[6] + 1, dtype=np.int64)           # annotation ids renumbered
    out[12] = int(mult.sum())
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=1366)
    p.add_argument("--replicates", type=int, default=2000)
    p.add_argument("--cpu-replicates", type=int, default=24)
    a = p.parse_args()
    gt, res = dataset(a.images)
    t0 = time.perf_counter()
    m = bootstrap.export_matches(gt, res)
    t_export = time.perf_counter() - t0
    ev = m["evaluator"]
    I, K, A, T, R = len(ev.img_ids), len(ev.cat_ids), len(ev.area_rng), len(ev.iou_thrs), len(ev.rec_thrs)
    L = int(m["list_off"][-1])
    mult = bootstrap.resample_multiplicities(I, a.replicates, 0)
    print(f"{I} images, {len(res)} detections ({len(res) / I:.1f} per image), {len(gt['annotations'])} ground-truth boxes, list lengths "
          f"{np.diff(m['list_off']).tolist()}, largest multiplicity {mult.max()}; export_matches {t_export * 1e3:.1f} ms (host, once)")
    run = bootstrap.ap_bootstrap(m, mult[:2], full_table=True)
    ev.evaluate()
    ev.accumulate()
    want = np.stack([ev.eval["precision"][:, :, k, ar, md] for k in range(K) for ar, md in bootstrap.SUMMARY_CELLS])
    assert run["precision"][0].tobytes() == want.tobytes(), "replicate 0 is not the evaluator's table"

    dev = torch.device("cuda")
    up = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev)      # noqa: E731
    d = {k: up(m[k]) for k in ("list_off", "list_img", "list_rank", "list_flags", "npig")}
    cells = bootstrap.summary_cells(m)
    d_mult, d_cells, d_thr = up(np.ascontiguousarray(mult, dtype=np.uint8)), up(cells), up(np.ascontiguousarray(ev.rec_thrs))
    B, C = mult.shape[0], len(cells)
    psum, recall = (torch.empty((B, C, T), dtype=torch.float64, device=dev) for _ in range(2))
    valid = torch.empty((B, C), dtype=torch.int32, device=dev)
    launch = lambda: _lib.check(_lib.lib().pe_ap_bootstrap(      # noqa: E731
        _lib.ptr(d["list_off"]), _lib.ptr(d["list_img"]), _lib.ptr(d["list_rank"]), _lib.ptr(d["list_flags"]), L, _lib.ptr(d["npig"]),
        _lib.ptr(d_mult), B, I, K, A, T, _lib.ptr(d_thr), R, _lib.ptr(d_cells), C, _lib.ptr(psum), _lib.ptr(recall), _lib.ptr(valid), None,
        _lib.stream()), "pe_ap_bootstrap")
    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    # what one (replicate, cell, threshold) wavefront reads: two walks of its category's list, 9 bytes per entry (image 4, rank 1, flags 4)
    entries = int(sum(int(m["list_off"][k + 1] - m["list_off"][k]) for k, _, _ in cells)) * T * B
    read = 2 * 9 * entries
    print(f"pe_ap_bootstrap B = {B}, {C} cells, T = {T}: median {ms:.2f} ms of 10 launches (min {min(times):.2f}, max {max(times):.2f}); "
          f"{ms * 1e3 / B:.1f} us per replicate; {entries / ms / 1e6:.1f} G list entries / s per pass pair; list bytes read (from cache: the lists are "
          f"{9 * L + 4 * (A - 1) * L} bytes) {read / 1e9:.2f} GB -> {read / ms / 1e9:.2f} TB/s")
    chunks = [-(-int(m["list_off"][k + 1] - m["list_off"][k]) // 64) for k in range(K)]
    print(f"64-entry chunks per wavefront walk: {chunks}; workgroups {B * C} of {T} wavefronts")

    if a.cpu_replicates:
        base = ev._native_arrays()
        prec, rec = np.empty((T, R, K, A, 3)), np.empty((T, K, A, 3))
        cpu = []
        for b in range(1, a.cpu_replicates + 1):
            arrs = duplicated_arrays(base, mult[b])
            t0 = time.perf_counter()
            ev._native_call("pe_cocoeval_bbox", arrs + [prec, rec])
            cpu.append(time.perf_counter() - t0)
            if b <= 2:
                got = bootstrap.ap_bootstrap(m, mult[b:b + 1], full_table=True)["precision"][0]
                want = np.stack([prec[:, :, k, ar, md] for k in range(K) for ar, md in bootstrap.SUMMARY_CELLS])
                assert got.tobytes() == want.tobytes(), f"replicate {b} is not the evaluator on the duplicated dataset"
        c = float(np.median(cpu))
        print(f"pe_cocoeval_bbox on the duplicated dataset ({os.cpu_count()} CPUs visible, its default thread count): median {c * 1e3:.1f} ms of "
              f"{len(cpu)} replicates (matching and accumulate) -> {c * B:.1f} s for B = {B}; GPU {ms:.1f} ms: ratio {c * B * 1e3 / ms:.0f}")


if __name__ == "__main__":
    main()
