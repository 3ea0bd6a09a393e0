"""File-driven throughput of `demo_probEn --one-pass`: frame pairs decoded from JPEG files by worker processes, fusion inputs
built on the GPU (pe_fusion_input_pack), two R101-FPN detectors (thermal_only + early_fusion) + ProbEn + evaluation rows.

    python scripts/stream_bench.py [--pairs 320] [--batch 32] [--workers 4,8,15] [--rgb 512x640,1600x1800]

Writes --pairs seeded synthetic JPEG pairs (thermal 640x512, RGB at each --rgb size HxW, quality 95) into a temporary directory
and prints one JSON line per (RGB size, worker count): pairs/s over the timed part (after the first batch) and the fraction of
that wall time the GPU side waited on decode.  bench.py measures the same detectors on frames already resident in HBM."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_pairs(root, n, th_hw, rgb_hw, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "thermal_8_bit"))
    os.makedirs(os.path.join(root, "RGB"))
    images = []
    # a few distinct smooth-plus-noise frames, cycled: decode cost of a real-looking JPEG, not of white noise
    base_t = [(rng.normal(0, 1, th_hw).cumsum(0).cumsum(1) % 256).astype(np.uint8) for _ in range(4)]
    for i in range(n):
        stem = f"FLIR_{i:05d}"
        t = np.repeat(base_t[i % 4][:, :, None], 3, axis=2)
        t = np.clip(t.astype(np.int16) + rng.integers(-8, 9, t.shape), 0, 255).astype(np.uint8)
        r = np.clip(rng.normal(0, 1, rgb_hw + (3,)).cumsum(0).cumsum(1) * 0.5 % 256 + rng.integers(0, 16, rgb_hw + (3,)), 0, 255)
        Image.fromarray(t).save(os.path.join(root, "thermal_8_bit", stem + ".jpeg"), quality=95)
        Image.fromarray(r.astype(np.uint8)).save(os.path.join(root, "RGB", stem + ".jpg"), quality=95)
        images.append({"id": i, "file_name": f"thermal_8_bit/{stem}.jpeg", "height": th_hw[0], "width": th_hw[1]})
    with open(os.path.join(root, "FLIR_thermal_RGBT_pairs_val.json"), "w") as f:
        json.dump({"images": images, "categories": [{"id": 1, "name": "person"}, {"id": 2, "name": "bicycle"}, {"id": 3, "name": "car"}]}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=320)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--workers", type=str, default="4,8,15")
    ap.add_argument("--rgb", type=str, default="512x640,1600x1800", help="RGB frame sizes HxW (thermal is 512x640)")
    args = ap.parse_args()
    import proben_amd  # noqa: F401
    from proben_amd.cli import demo_probEn
    th_hw = (512, 640)
    with tempfile.TemporaryDirectory() as tmp:
        for rgb in args.rgb.split(","):
            rgb_hw = tuple(int(v) for v in rgb.split("x"))
            root = os.path.join(tmp, f"val_{rgb}")
            t0 = time.perf_counter()
            write_pairs(root, args.pairs, th_hw, rgb_hw)
            print(f"# wrote {args.pairs} pairs, RGB {rgb}, in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
            for w in args.workers.split(","):
                res = demo_probEn.main(["--one-pass", "--dataset_path", root, "--detectors", "thermal_only,early_fusion",
                                        "--model_paths", "synthetic://1,synthetic://2", "--workers", w, "--batch", str(args.batch),
                                        "--outfolder", os.path.join(tmp, "out"), "--dataset_name", f"stream_{rgb}_{w}"])
                st = res["one_pass"]
                print(json.dumps({"metric": "file-driven frame-pairs/s (thermal_only + early_fusion R101-FPN + ProbEn)",
                                  "pairs_per_s": round(st["pairs_per_s"], 1), "decode_wait_fraction": round(st["decode_wait_fraction"], 3),
                                  "workers": int(w), "batch": args.batch, "thermal_hw": list(th_hw), "rgb_hw": list(rgb_hw),
                                  "pairs": st["pairs"], "timed_pairs": st["timed_pairs"]}), flush=True)


if __name__ == "__main__":
    main()
