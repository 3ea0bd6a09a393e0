"""Kernel-trace workload for the posterior outputs of the fusion (profiles/posterior_trace.txt): the 32-image,
two-detector step of scripts/pool_probe.py (D = 100 rows per detector and image, 60-100 live, half of them overlapping the other
detector's, K = 3), 50 times each of the log-posterior fusion and the pooled fusion (proben_fuse_kernel<true, true, false / true, false>)
and, beside them, the same two with the posterior outputs (proben_fuse_kernel<true, true, false / true, true>).

    rocprofv3 --kernel-trace --stats -d OUT -o posterior --output-format csv -- python scripts/posterior_probe.py

--lib PATH loads another build of the library (a parent commit's, for the yardstick); --without-posterior leaves the new entry point
alone, which such a library does not export.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proben_amd  # noqa: E402,F401
from proben_amd import _lib, fusion as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--without-posterior", action="store_true")
args = ap.parse_args()
if args.lib:
    _lib.LIB_PATH = os.path.abspath(args.lib)
if args.without_posterior:
    _lib.SIGNATURES.pop("pe_proben_fuse_batch_posterior")

B, D, K, G = 32, 100, 3, 12
rng = np.random.default_rng(3)
x1 = rng.uniform(0, 520, (B, G)); y1 = rng.uniform(0, 400, (B, G))
gt = np.stack([x1, y1, x1 + rng.uniform(20, 120, (B, G)), y1 + rng.uniform(20, 100, (B, G))], 2)
dets = []
for d in range(2):
    cnt = rng.integers(60, 101, B).astype(np.int32)
    x1 = rng.uniform(0, 520, (B, D)); y1 = rng.uniform(0, 400, (B, D))
    bx = np.stack([x1, y1, x1 + rng.uniform(20, 120, (B, D)), y1 + rng.uniform(20, 100, (B, D))], 2)
    bx[:, :48] = np.tile(gt, (1, 4, 1)) + rng.normal(0, 2, (B, 48, 4))          # half of the rows sit on ground truth (and on each other)
    lg = rng.normal(0, 3, (B, D, K + 1)).astype(np.float32)
    cls = lg[:, :, :K].argmax(2).astype(np.int32)
    if d == 1:
        cls[:, :48] = dets[0]["classes"].cpu().numpy()[:, :48]
    e = np.exp(lg - lg.max(2, keepdims=True)); p = (e / e.sum(2, keepdims=True)).astype(np.float32)
    dets.append({"boxes": torch.from_numpy(bx.astype(np.float32)).cuda(), "scores": torch.from_numpy(np.take_along_axis(p, cls[..., None].astype(np.int64), 2)[..., 0].copy()).cuda(),
                 "classes": torch.from_numpy(cls).cuda(), "prob_score": torch.from_numpy(p[:, :, :K].copy()).cuda(),
                 "class_logits": torch.from_numpy(lg).cuda(), "vars": torch.from_numpy((10.0 ** rng.uniform(-3, -1, (B, D))).astype(np.float32)).cuda(),
                 "counts": torch.from_numpy(cnt).cuda()})
prior = [0.2, 0.1, 0.3, 0.4]
W = F.pool_weight_tensor([0.6, 0.3], 2, "cuda")
post = {}
for it in range(50):
    plain = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior)
    pooled = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, pool_weights=W)
    if not args.without_posterior:
        post = {"plain": F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, with_posterior=True),
                "pooled": F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, pool_weights=W, with_posterior=True)}
torch.cuda.synchronize()
print("step: fused rows", int(plain["counts"].sum()), "pooled", int(pooled["counts"].sum()),
      "| with the posterior:", {k: (int(v["counts"].sum()), int(v["members"].sum())) for k, v in post.items()})
