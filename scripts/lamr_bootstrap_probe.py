"""Cost of the LAMR bootstrap (profiles/lamr_bootstrap.txt) on a KAIST-sized synthetic case: 2 252 images
(1 455 day), about one pedestrian per image, a result list of a few rows per image (jittered copies of the pedestrians and random
boxes).  Times pe_lamr_bootstrap at B = 2 000 replicates over the 3 cells all / day / night (2 warm-up launches, then 10 launches between
device events: the median), the export's one-off cost, a vectorised NumPy statement of the same rule on the host per replicate on the
same lists, and KAISTPedEval (evaluate and accumulate for all / day / night, as evaluate() runs them) on the explicitly duplicated
dataset of a few of the same replicates.  Checks on the way that the kernel's integers are the NumPy rule's and that the figures are
the duplicated evaluator's, bit for bit.

    python scripts/lamr_bootstrap_probe.py [--images 2252] [--per-image 4] [--replicates 2000] [--numpy-replicates 200] [--evaluator-replicates 3]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proben_amd  # noqa: E402,F401
from proben_amd import _lib, lamr_bootstrap as LB  # noqa: E402
from proben_amd.bootstrap import resample_multiplicities  # noqa: E402
from proben_amd.evalKAIST.evaluation_script import KAIST, KAISTPedEval  # noqa: E402


def dataset(n_images, per_image, seed=28):
    rng = np.random.default_rng(seed)
    anns, res = [], []
    for i in range(n_images):
        gts = []
        for _ in range(rng.poisson(1.0)):
            h = float(rng.uniform(40, 140))
            box = [float(rng.uniform(5, 560)), float(rng.uniform(5, 500 - h)), float(0.41 * h), h]
            gts.append(box)
            anns.append({"id": len(anns), "image_id": i, "category_id": 1, "bbox": box, "height": h, "occlusion": int(rng.integers(0, 3)), "ignore": 0})
        rows = []
        for g in gts:
            for _ in range(rng.binomial(2, 0.6)):
                b = np.array(g) + rng.normal(0, 0.08, 4) * np.array([g[2], g[3], g[2], g[3]])
                rows.append((b.tolist(), float(rng.beta(5, 2))))
        for _ in range(rng.poisson(max(per_image - 1.2, 0.0))):
            h = float(rng.uniform(40, 140))
            rows.append(([float(rng.uniform(5, 560)), float(rng.uniform(5, 500 - h)), 0.41 * h, h], float(rng.beta(2, 4))))
        rows.sort(key=lambda r: -r[1])
        res += [{"image_id": i, "category_id": 1, "bbox": [float(v) for v in b], "score": s} for b, s in rows]
    ann = {"images": [{"id": i, "im_name": str(i), "height": 512, "width": 640} for i in range(n_images)], "annotations": anns,
           "categories": [{"id": 1, "name": "person"}]}
    return ann, res


def numpy_replicate(m, matches, cells, thr):
    """The rule of DESIGN.md 28 for one multiplicity row and every cell, vectorised over the list: (tp_at [C, R], totals [C, 4])."""
    img, flags, npig = matches["list_img"], matches["list_flags"], matches["npig"]
    matched, counted = (flags & 1) != 0, (flags & 2) == 0
    tp_at, totals = np.zeros((len(cells), len(thr)), dtype=np.int64), np.zeros((len(cells), 4), dtype=np.int64)
    for c, (lo, hi) in enumerate(cells):
        w = np.where((img >= lo) & (img < hi) & counted, m[img], 0)
        wf = np.where(matched, 0, w)
        wt = w - wf
        F = np.cumsum(wf) - wf
        N, NP = int(m[lo:hi].sum()), int((m[lo:hi] * npig[lo:hi]).sum())
        TP, FP = int(wt.sum()), int(wf.sum())
        totals[c] = N, NP, TP, FP
        if NP == 0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            x = F.astype(np.float64) / np.float64(N)
            tp_at[c] = ((x[:, None] <= thr[None, :]) * wt[:, None]).sum(0)
            if TP + FP > 0:
                j = int(np.flatnonzero(w)[0])
                first = np.float64(0 if matched[j] else 1) / np.float64(N) <= thr
                tp_at[c][~first] = TP
    return tp_at, totals


def duplicated(ann, res, m):
    by_img_a, by_img_r = {}, {}
    for a in ann["annotations"]:
        by_img_a.setdefault(a["image_id"], []).append(a)
    for r in res:
        by_img_r.setdefault(r["image_id"], []).append(r)
    images, anns, rows = [], [], []
    for im in ann["images"]:
        for c in range(int(m[im["id"]])):
            nid = im["id"] * 1000 + c
            images.append(dict(im, id=nid))
            anns += [dict(a, image_id=nid, id=len(anns) + k) for k, a in enumerate(by_img_a.get(im["id"], []))]
            rows += [dict(r, image_id=nid) for r in by_img_r.get(im["id"], [])]
    return {"images": images, "annotations": anns, "categories": ann["categories"]}, rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=2252)
    p.add_argument("--per-image", type=float, default=4.0)
    p.add_argument("--replicates", type=int, default=2000)
    p.add_argument("--numpy-replicates", type=int, default=200)
    p.add_argument("--evaluator-replicates", type=int, default=3)
    a = p.parse_args()
    ann, res = dataset(a.images, a.per_image)
    t0 = time.perf_counter()
    m = LB.export_lamr_matches(ann, res)
    t_export = time.perf_counter() - t0
    I, L = len(m["npig"]), len(m["list_img"])
    cells = LB.lamr_cells(I)
    thr = np.ascontiguousarray(m["evaluator"].params.fppiThrs, dtype=np.float64)
    mult = resample_multiplicities(I, a.replicates, 0)
    B, C, R = mult.shape[0], len(cells), len(thr)
    print(f"{I} images ({int(cells[1, 1])} day), {len(res)} result rows ({len(res) / I:.2f} per image), {len(ann['annotations'])} ground-truth boxes "
          f"({int(m['npig'].sum())} not ignored), list {L} entries = {-(-L // 64)} chunks of 64, largest multiplicity {mult.max()}; "
          f"export_lamr_matches {t_export * 1e3:.0f} ms (host, once per file and setup)")

    run = LB.lamr_bootstrap(m, mult, cells)
    dev = torch.device("cuda")
    up = lambda x: torch.from_numpy(x).to(dev)      # noqa: E731
    d_img, d_flags, d_npig, d_mult, d_cells, d_thr = (up(x) for x in (m["list_img"], m["list_flags"], m["npig"], np.ascontiguousarray(mult, dtype=np.uint8), cells, thr))
    tp_at = torch.empty((B, C, R), dtype=torch.int64, device=dev)
    totals = torch.empty((B, C, 4), dtype=torch.int64, device=dev)
    valid = torch.empty((B, C), dtype=torch.int32, device=dev)
    launch = lambda: _lib.check(_lib.lib().pe_lamr_bootstrap(      # noqa: E731
        _lib.ptr(d_img), _lib.ptr(d_flags), L, _lib.ptr(d_npig), _lib.ptr(d_mult), B, I, _lib.ptr(d_thr), R, _lib.ptr(d_cells), C, _lib.ptr(tp_at),
        _lib.ptr(totals), _lib.ptr(valid), _lib.stream()), "pe_lamr_bootstrap")
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
    assert tp_at.cpu().numpy().tobytes() == run["tp_at"].tobytes()
    print(f"pe_lamr_bootstrap B = {B}, {C} cells, R = {R}: median {ms:.3f} ms of 10 launches (min {min(times):.3f}, max {max(times):.3f}); "
          f"{ms * 1e3 / B:.2f} us per replicate; {B} workgroups of {C} wavefronts, {B * C * -(-L // 64)} wavefront-chunks, "
          f"{B * C * L * 5 / ms / 1e6:.1f} GB/s of list bytes (5 per entry, from cache: the list is {5 * L} bytes)")
    t0 = time.perf_counter()
    stats = LB.lamr_statistics(run, m)
    t_stats = time.perf_counter() - t0
    print(f"lamr_statistics (host, row by row): {t_stats * 1e3:.0f} ms for {B} x {C}; MR of the dataset {stats['MR'][0].tolist()}, "
          f"standard errors {stats['MR'][1:].std(0, ddof=1).tolist()}")

    if a.numpy_replicates:
        n = min(a.numpy_replicates, B)
        t0 = time.perf_counter()
        host = [numpy_replicate(mult[b], m, cells.tolist(), thr) for b in range(n)]
        t_np = (time.perf_counter() - t0) / n
        for b, (t, tot) in enumerate(host):
            assert t.tobytes() == run["tp_at"][b].tobytes() and tot.tobytes() == run["totals"][b].tobytes(), f"replicate {b}: the kernel is not the NumPy rule"
        print(f"NumPy rule on the host, the same lists: {t_np * 1e3:.3f} ms per replicate over {n} (equal integers) -> {t_np * B:.2f} s for B = {B}; "
              f"GPU {ms:.3f} ms: ratio {t_np * B * 1e3 / ms:.0f}")
    if a.evaluator_replicates:
        cpu = []
        for b in range(1, a.evaluator_replicates + 1):
            ann2, res2 = duplicated(ann, res, mult[b])
            gt = KAIST()
            gt.dataset = ann2
            gt._index()
            dt = gt.loadRes(res2)
            ids = sorted(gt.getImgIds())
            t0 = time.perf_counter()
            mrs = []
            for lo, hi in cells.tolist():
                ev = KAISTPedEval(gt, dt, "bbox")
                ev.params.imgIds = [i for i in ids if lo <= i // 1000 < hi]
                ev.evaluate(0)
                ev.accumulate()
                mrs.append(ev.summarize(0))
            cpu.append(time.perf_counter() - t0)
            assert np.array(mrs).tobytes() == stats["MR"][b].tobytes(), f"replicate {b} is not the evaluator on the duplicated dataset: {mrs} vs {stats['MR'][b]}"
        c = float(np.median(cpu))
        print(f"KAISTPedEval on the duplicated dataset (evaluate + accumulate for all / day / night): median {c:.2f} s of {len(cpu)} replicates "
              f"(equal MR bytes) -> {c * B / 60:.0f} min for B = {B}; GPU {ms:.3f} ms: ratio {c * B * 1e3 / ms:.0f}")


if __name__ == "__main__":
    main()
