"""Kernel-trace workload for the pooling-weight kernels (profiles/pool_trace.txt): one 32-image, two-detector
step (D = 100 rows per detector and image, 60-100 live, half of them overlapping the other detector's, K = 3), 50 times each of: the
log-posterior pack and fusion (proben_pack_kernel<LOGITS_LOGP>, proben_fuse_kernel<*, true>) and the pooled pack and fusion beside
them (out_source, the weights, out_cluster); then 10 x pe_pool_nll at 10^5 clusters of 2 or 3 rows, with 1 + D candidates (a Newton
round of the fit) and with 64.

    rocprofv3 --kernel-trace --stats -d OUT -o pool --output-format csv -- python scripts/pool_probe.py
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
W = F.pool_weight_tensor([0.6, 0.3], 2, "cuda")
for it in range(50):
    plain = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior)                      # LOGITS_LOGP pack + fuse<*, true>
    pooled = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, pool_weights=W)     # the pooled pack + fuse
torch.cuda.synchronize()
Cn = 100_000
size = rng.integers(2, 4, Cn)
offs = np.concatenate([[0], np.cumsum(size)]).astype(np.int32)
N = int(offs[-1])
z = rng.normal(0, 2, (N, K + 1))
lp = torch.from_numpy(z - np.log(np.exp(z).sum(1, keepdims=True))).cuda()
src = torch.from_numpy(((np.arange(N) - np.repeat(offs[:-1], size)) % 2).astype(np.int32)).cuda()
mem = torch.arange(N, dtype=torch.int32, device="cuda")
lab = torch.from_numpy(rng.integers(0, K + 1, Cn).astype(np.int32)).cuda()
doffs = torch.from_numpy(offs).cuda()
for it in range(10):
    few = C.pool_nll(lp, src, mem, doffs, lab, rng.uniform(0.1, 1.2, (3, 2)))
    many = C.pool_nll(lp, src, mem, doffs, lab, rng.uniform(0.1, 1.2, (64, 2)))
torch.cuda.synchronize()
print("step: fused rows", int(plain["counts"].sum()), "pooled", int(pooled["counts"].sum()), "rows in a cluster", int((pooled["cluster"] >= 0).sum()),
      "| 10^5 clusters: excluded", few[2], many[2], "NLL per cluster", float(many[0][0]) / Cn)
