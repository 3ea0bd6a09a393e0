"""PDQ pair quality on a FLIR-sized synthetic set (profiles/pdq.txt): kernel time of pe_pdq_pair_quality.

    python scripts/pdq_probe.py [--images 256] [--gts 6] [--dets 8] [--launches 10]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/pdq_probe.py

Images of 640 x 512; per image --gts ground-truth boxes (20 .. 160 pixels wide, 20 .. 130 high) and --dets detections: one jittered copy
per ground truth (while they last) and random boxes for the rest, variances 10^U(-1.5, 0.5) in box-delta units, label distributions from
random logits.  Prints the workload (pairs, ground-truth pixels per pair, support pixels per detection) and the device-event time of
--launches launches after 3 warm-up launches."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proben_amd  # noqa: E402,F401
from proben_amd import pdq  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--gts", type=int, default=6)
    ap.add_argument("--dets", type=int, default=8)
    ap.add_argument("--launches", type=int, default=10)
    a = ap.parse_args()
    rng = np.random.default_rng(30)
    H, W, K = 512, 640, 3
    B, G, M = a.images, a.gts, a.dets

    def boxes(n):
        x1, y1 = rng.uniform(0, W - 170, n), rng.uniform(0, H - 140, n)
        return np.stack([x1, y1, x1 + rng.uniform(20, 160, n), y1 + rng.uniform(20, 130, n)], 1)
    gt = boxes(B * G).reshape(B, G, 4)
    det = boxes(B * M).reshape(B, M, 4)
    n = min(G, M)
    det[:, :n] = gt[:, :n] + rng.normal(0, 2.0, (B, n, 4))
    var = 10.0 ** rng.uniform(-1.5, 0.5, B * M)
    z = rng.normal(0, 2, (B * M, K + 1))
    lp = z - np.log(np.exp(z).sum(1, keepdims=True))
    t = lambda x, dt: torch.as_tensor(x, dtype=dt).cuda()      # noqa: E731
    args = (t(det.reshape(-1, 4), torch.float64), t(var, torch.float64), t(lp, torch.float64), np.arange(B + 1) * M,
            t(gt.reshape(-1, 4), torch.float64), t(rng.integers(0, K, B * G), torch.int32), t(np.zeros(B * G), torch.int32), np.arange(B + 1) * G,
            t(np.tile([H, W], (B, 1)), torch.int32))
    for _ in range(3):
        out = pdq.pair_quality(*args)
    times = []
    for _ in range(a.launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pdq.pair_quality(*args)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    area = ((np.clip(gt[..., 2], 0, W) - np.clip(gt[..., 0], 0, W)) * (np.clip(gt[..., 3], 0, H) - np.clip(gt[..., 1], 0, H))).mean()
    q = out["q"].cpu().numpy()
    print(f"{B} images of {W} x {H}, {G} ground truths and {M} detections each: {B * M} workgroups, {q.size} pairs, {area:.0f} ground-truth pixels "
          f"per pair on average; {out['excluded_detections']} detections excluded, {out['ignored_ground_truths']} ground truths ignored; mean q "
          f"{q.mean():.4f}, largest {q.max():.4f}")
    print(f"pair_quality (uploads of the offsets, the launch, the flags' read-back), device events: median {np.median(times):.3f} ms, min {min(times):.3f}, "
          f"max {max(times):.3f} over {a.launches} calls")


if __name__ == "__main__":
    main()
