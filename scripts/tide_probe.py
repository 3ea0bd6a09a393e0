"""Cost of the TIDE decomposition (profiles/tide.txt) on the FLIR-sized synthetic case of
scripts/ap_bootstrap_probe.py: 1 366 images, 3 classes, about 100 detections per image.  Times pe_tide_classify (one launch per file)
and the nine-variant pe_ap_bootstrap launch at B = 2 000 replicates (27 cells, T = 1), each as the median of 10 launches between device
events after 2 warm-up launches, and the host steps around them once.  Checks on the way that variant 0 of replicate 0 is the
evaluator's AP50 column.

    python scripts/tide_probe.py [--images 1366] [--replicates 2000]
    rocprofv3 --kernel-trace --stats -d OUT -o tide --output-format csv -- python scripts/tide_probe.py
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proben_amd  # noqa: E402,F401
from ap_bootstrap_probe import dataset  # noqa: E402
from proben_amd import _lib, bootstrap, tide  # noqa: E402


def timed(launch):
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
    return float(np.median(times)), min(times), max(times)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--images", type=int, default=1366)
    p.add_argument("--replicates", type=int, default=2000)
    a = p.parse_args()
    gt, res = dataset(a.images)
    # the synthetic set holds a few inverted boxes (negative width or height): the evaluator ignores them (area outside its range "all",
    # never matched) and tide.layout refuses such a set, so they are dropped here
    n_all = len(res)
    res = [r for r in res if r["bbox"][2] >= 0 and r["bbox"][3] >= 0]
    print(f"{n_all - len(res)} of {n_all} synthetic rows dropped (inverted boxes)")
    wall = {}
    t0 = time.perf_counter()
    m = bootstrap.export_matches(gt, res)
    wall["export_matches"] = time.perf_counter() - t0
    ev = m["evaluator"]
    t0 = time.perf_counter()
    lay = tide.layout(m)
    wall["layout"] = time.perf_counter() - t0
    I, K = len(ev.img_ids), len(ev.cat_ids)
    M, G = len(lay["det_cat"]), len(lay["gt_cat"])
    per_d, per_g = np.diff(lay["det_off"]), np.diff(lay["gt_off"])
    print(f"{I} images, {len(res)} detections, {M} list entries (largest image {per_d.max()}), {G} ground-truth boxes (largest image {per_g.max()}), "
          f"{K} classes; export_matches {wall['export_matches'] * 1e3:.1f} ms, layout {wall['layout'] * 1e3:.1f} ms (host, once per file)")

    dev = torch.device("cuda")
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(dev)      # noqa: E731
    d_box, d_cat, g_box = up(lay["det_box"], np.float64), up(lay["det_cat"], np.int32), up(lay["gt_box"], np.float64)
    g_cat, g_crowd = up(lay["gt_cat"], np.int32), up(lay["gt_crowd"], np.uint8)
    d_off, g_off = np.ascontiguousarray(lay["det_off"], dtype=np.int32), np.ascontiguousarray(lay["gt_off"], dtype=np.int32)
    ws = torch.empty(2 * (I + 1), dtype=torch.int32, device=dev)
    outs = [torch.empty(M, dtype=torch.int32, device=dev) for _ in range(4)] + [torch.empty(G, dtype=torch.int32, device=dev)]
    classify = lambda: _lib.check(_lib.lib().pe_tide_classify(      # noqa: E731
        _lib.ptr(d_box), _lib.ptr(d_cat), d_off.ctypes.data, _lib.ptr(g_box), _lib.ptr(g_cat), _lib.ptr(g_crowd), g_off.ctypes.data, I, K, M, G,
        0.5, 0.1, _lib.ptr(ws), *[_lib.ptr(o) for o in outs], _lib.stream()), "pe_tide_classify")
    ms, lo, hi = timed(classify)
    print(f"pe_tide_classify (with its two offset copies): median {ms:.3f} ms of 10 launches (min {lo:.3f}, max {hi:.3f}); {I} workgroups of 256; "
          f"{ms * 1e3 / I:.2f} us per image")

    t0 = time.perf_counter()
    cl = tide.classify(gt, res, matches=m)
    wall["classify"] = time.perf_counter() - t0
    assert np.array_equal(outs[1].cpu().numpy(), cl["type"][lay["order"]]), "the timed launch and classify() disagree"
    t0 = time.perf_counter()
    lists = tide.variant_lists(cl)
    wall["variant_lists"] = time.perf_counter() - t0
    c = cl["counts"]
    print("types " + ", ".join(f"{n} {int(c['types'][t].sum())}" for t, n in enumerate(tide.TYPES)) + f", missed {int(c['missed'].sum())}, "
          f"unmatched {int(c['unmatched'].sum())}, moved copies {int(lists['moved'].sum())}; classify() {wall['classify'] * 1e3:.1f} ms, "
          f"variant_lists() {wall['variant_lists'] * 1e3:.1f} ms (host)")

    mult = bootstrap.resample_multiplicities(I, a.replicates, 0)
    first = tide.price(lists, mult[:2], full_table=True)
    ev.evaluate()
    ev.accumulate()
    assert np.ascontiguousarray(first["precision"][0][:, 0, :].T).tobytes() == ev.eval["precision"][0, :, :, 0, 2].tobytes(), \
        "variant 0 of replicate 0 is not the evaluator's AP50 column"
    V, R, B = len(tide.VARIANTS), len(lists["rec_thrs"]), mult.shape[0]
    L = int(lists["list_off"][-1])
    cells = np.array([[k, v, lists["max_det"]] for k in range(K) for v in range(V)], dtype=np.int32)
    upl = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev)      # noqa: E731
    d = {k: upl(lists[k]) for k in ("list_off", "list_img", "list_rank", "list_flags", "npig")}
    d_mult, d_cells, d_thr = upl(np.ascontiguousarray(mult, dtype=np.uint8)), upl(cells), upl(lists["rec_thrs"])
    C = len(cells)
    psum, recall = (torch.empty((B, C, 1), dtype=torch.float64, device=dev) for _ in range(2))
    valid = torch.empty((B, C), dtype=torch.int32, device=dev)
    accumulate = lambda: _lib.check(_lib.lib().pe_ap_bootstrap(      # noqa: E731
        _lib.ptr(d["list_off"]), _lib.ptr(d["list_img"]), _lib.ptr(d["list_rank"]), _lib.ptr(d["list_flags"]), L, _lib.ptr(d["npig"]),
        _lib.ptr(d_mult), B, I, K, V, 1, _lib.ptr(d_thr), R, _lib.ptr(d_cells), C, _lib.ptr(psum), _lib.ptr(recall), _lib.ptr(valid), None,
        _lib.stream()), "pe_ap_bootstrap")
    ms, lo, hi = timed(accumulate)
    print(f"pe_ap_bootstrap, nine variants: B = {B}, {C} cells, T = 1, list lengths {np.diff(lists['list_off']).tolist()}: median {ms:.2f} ms of 10 "
          f"launches (min {lo:.2f}, max {hi:.2f}); {ms * 1e3 / B:.1f} us per replicate; workgroups {B * C} of 1 wavefront")
    ap = first["ap"][0]
    print("AP50 " + f"{ap[0]:.6f}; dAP " + ", ".join(f"{n} {ap[v] - ap[0]:+.6f}" for v, n in enumerate(tide.VARIANTS) if v))


if __name__ == "__main__":
    main()
