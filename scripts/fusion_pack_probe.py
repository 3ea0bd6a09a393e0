"""Batch-32 fusion-input packs, for `rocprofv3 --kernel-trace --stats`: pe_fusion_input_pack from uint8 thermal + RGB frames
(early fusion: one group, middle fusion: two) next to pe_preprocess_pack_batch (preprocess_pack_kernel) on the host-built float32
frames of the same batch, each launched --reps times.  Prints per-launch event times and the bytes each launch moves (from the
shapes: frames read once + NHWC4 fp16 written).

    python scripts/fusion_pack_probe.py [--batch 32] [--reps 20] [--rgb 512x640]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rgb", type=str, default="512x640", help="RGB frame size HxW (thermal 512x640)")
    args = ap.parse_args()
    import torch
    import proben_amd  # noqa: F401
    from proben_amd import layers as L
    n, (th_h, th_w) = args.batch, (512, 640)
    rgb_h, rgb_w = (int(v) for v in args.rgb.split("x"))
    dst, pad = (800, 1000), (800, 1024)
    rng = np.random.default_rng(0)
    th = torch.from_numpy(rng.integers(0, 256, (n, th_h, th_w, 3), dtype=np.uint8)).cuda()
    rgb = torch.from_numpy(rng.integers(0, 256, (n, rgb_h, rgb_w, 3), dtype=np.uint8)).cuda()
    out = torch.empty((n,) + pad + (4,), dtype=torch.float16, device="cuda")
    mean = [103.53, 116.28, 123.675, 135.438]
    res = []

    def timed(name, fn, nbytes):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1000 / args.reps
        res.append({"launch": name, "us": round(us, 1), "bytes": nbytes, "GB_per_s": round(nbytes / us / 1e3, 1)})

    w_out = out.numel() * 2
    for method, groups in (("early", [(0, 4)]), ("middle", [(0, 3), (3, 3)])):
        C = 4 if method == "early" else 6
        f32 = torch.empty((n, th_h, th_w, C), dtype=torch.float32, device="cuda").uniform_(0, 255).floor_()
        for ch0, nch in groups:
            rd = th.numel() + (rgb.numel() if ch0 < 3 else 0)
            timed(f"pe_fusion_input_pack {method} ch[{ch0},{ch0 + nch}) rgb {rgb_h}x{rgb_w}",
                  lambda: L.fusion_input_pack(th, rgb if ch0 < 3 else None, out, ch0=ch0, nch=nch, dst_hw=dst,
                                              mean=mean[:nch], std=[1.0] * nch), rd + w_out)
            timed(f"pe_preprocess_pack_batch f32 {method} ch[{ch0},{ch0 + nch})",
                  lambda: L.preprocess_pack_batch(f32, out, src_kind=1, ch0=ch0, nch=nch, flip_rgb=False, dst_hw=dst,
                                                  mean=mean[:nch], std=[1.0] * nch), f32.numel() * 4 + w_out)
    for r in res:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
