"""Kernel-trace workload for the presence-evidence kernels (profiles/presence_trace.txt): section 15's 32-image,
two-detector step (D = 100 rows per detector and image, 60-100 live, half of them overlapping the other detector's, K = 3), 50 times
each of: the log-posterior fusion and the pooled fusion as they were (proben_fuse_kernel<true, true, false, false, false> and
<true, true, true, false, false>), and beside them the presence fusion score-only (<true, true, false, false, true>) and with pool
weights and the posterior outputs (<true, true, true, true, true>); then 10 x pe_bias_nll at 10^5 clusters with 1 + K candidates (a
Newton round of the fit), with 40 (its line search) and with 64.

    rocprofv3 --kernel-trace --stats -d OUT -o presence --output-format csv -- python scripts/presence_probe.py
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
T = C.presence_table([[0.0] * 4, [-0.1, -0.9, 0.0, 0.0], [-1.3, 0.0, 0.3, 0.0], [1.6, 1.5, 1.1, 0.0]], 2, K + 1, "cuda")
for it in range(50):
    plain = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior)
    pooled = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, pool_weights=W)
    pres = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, presence=T)
    full = F.fuse_detections(dets, "probEn-log", "v-avg", class_prior=prior, pool_weights=W, with_posterior=True, presence=T)
torch.cuda.synchronize()
Cn = 100_000
z = rng.normal(0, 2, (Cn, K + 1))
base = torch.from_numpy(z - np.log(np.exp(z).sum(1, keepdims=True))).cuda()
lab = torch.from_numpy(rng.integers(0, K + 1, Cn).astype(np.int32)).cuda()
for it in range(10):
    few = C.bias_nll(base, lab, rng.normal(0, 1, (1 + K, K + 1)))
    line = C.bias_nll(base, lab, rng.normal(0, 1, (40, K + 1)))
    many = C.bias_nll(base, lab, rng.normal(0, 1, (64, K + 1)))
torch.cuda.synchronize()
print("step: fused rows", int(plain["counts"].sum()), "pooled", int(pooled["counts"].sum()), "presence", int(pres["counts"].sum()),
      "lone rows", int((full["members"] == 1).sum()), "| 10^5 clusters: excluded", few[2], line[2], many[2], "NLL per cluster", float(many[0][0]) / Cn)
