"""Kernel-trace workload for the correlated box fusion (profiles/boxcorr_trace.txt): section 15's 32-image,
two-detector step (D = 100 rows per detector and image, 60-100 live, half of them overlapping the other detector's, K = 3), 50 times
each of: the pooled fusion and the pooled posterior fusion at v-avg as they were, and the same two at c-avg (the same fusion kernel,
then box_gls_kernel); then 10 x pe_box_pair_stats over 10^5 two-row clusters (box_residual_kernel, box_pair_kernel and the second
pass of csrc/reduce2.h).

    rocprofv3 --kernel-trace --stats -d OUT -o boxcorr --output-format csv -- python scripts/boxcorr_probe.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proben_amd  # noqa: E402,F401
from proben_amd import calibration as C, fusion as F  # noqa: E402

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
W = F.pool_weight_tensor([1.0, 1.0], 2, "cuda")
P = C.box_correlation_tensor([[0.6, 0.5], [0.5, 0.6]], 2, "cuda")
for it in range(50):
    v_plain = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, pool_weights=W)
    v_post = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, pool_weights=W, with_posterior=True)
    c_plain = F.fuse_detections(dets, "probEn-log", "c-avg", class_prior=prior, box_correlation=P)
    c_post = F.fuse_detections(dets, "probEn-log", "c-avg", class_prior=prior, pool_weights=W, with_posterior=True, box_correlation=P)
torch.cuda.synchronize()
Cn = 100_000
x1 = rng.uniform(0, 400, Cn); y1 = rng.uniform(0, 300, Cn)
g = np.stack([x1, y1, x1 + rng.uniform(20, 200, Cn), y1 + rng.uniform(20, 200, Cn)], 1)
rows = np.repeat(g, 2, 0) + rng.normal(0, 1.5, (2 * Cn, 4))
args = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (
    rows, 10.0 ** rng.uniform(-3, -1, 2 * Cn), np.tile(np.array([0, 1], np.int32), Cn), np.arange(2 * Cn, dtype=np.int32),
    np.arange(0, 2 * Cn + 1, 2, dtype=np.int32), np.arange(Cn, dtype=np.int32), g)]
for it in range(10):
    st = C.box_pair_stats(*args, 2)
torch.cuda.synchronize()
moved = int((c_post["members"] >= 2).sum())
print("step: fused rows", int(v_post["counts"].sum()), "of them clusters of two or more rows", moved, "| box differs on",
      int((c_post["boxes"] != v_post["boxes"]).any(1).sum()), "rows | 10^5 clusters: pairs", int(st["pairs"][0, 1]), "excluded", st["excluded"])
