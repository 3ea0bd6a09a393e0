"""Kernel-trace workload for the log-posterior ProbEn kernels (no trace is recorded yet): one 32-image, two-detector fusion step (D = 100 rows per detector and
image, 60-100 live, half of them overlapping the other detector's, K = 3), 50 times each of: the plain route, the temperature route,
the log-posterior route without and with a class prior.

    rocprofv3 --kernel-trace --stats -d OUT -o logp --output-format csv -- python scripts/proben_logp_probe.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proben_amd  # noqa: E402,F401
from proben_amd import fusion as F  # noqa: E402

B, D, K = 32, 100, 3
rng = np.random.default_rng(3)
dets = []
base = None
for d in range(2):
    cnt = rng.integers(60, 101, B).astype(np.int32)
    x1 = rng.uniform(0, 520, (B, D)); y1 = rng.uniform(0, 400, (B, D))
    bx = np.stack([x1, y1, x1 + rng.uniform(20, 120, (B, D)), y1 + rng.uniform(20, 100, (B, D))], 2)
    if base is None:
        base = bx
    else:
        bx[:, :50] = base[:, :50] + rng.normal(0, 2, (B, 50, 4))        # half of the rows overlap the other detector's
    lg = rng.normal(0, 3, (B, D, K + 1)).astype(np.float32)
    cls = lg[:, :, :K].argmax(2).astype(np.int32)
    if d == 1:
        cls[:, :50] = dets[0]["classes"].cpu().numpy()[:, :50]
    e = np.exp(lg - lg.max(2, keepdims=True)); p = (e / e.sum(2, keepdims=True)).astype(np.float32)
    dets.append({"boxes": torch.from_numpy(bx.astype(np.float32)).cuda(), "scores": torch.from_numpy(np.take_along_axis(p, cls[..., None].astype(np.int64), 2)[..., 0].copy()).cuda(),
                 "classes": torch.from_numpy(cls).cuda(), "prob_score": torch.from_numpy(p[:, :, :K].copy()).cuda(),
                 "class_logits": torch.from_numpy(lg).cuda(), "vars": torch.from_numpy(rng.uniform(0.5, 3, (B, D)).astype(np.float32)).cuda(),
                 "counts": torch.from_numpy(cnt).cuda()})
T = (1.5, 0.8)
prior = F.log_class_prior([0.2, 0.5, 0.2, 0.1], K + 1, "cuda")
for it in range(50):
    F.fuse_detections(dets)                                                   # proben_pack_kernel<PROBS> + proben_fuse_kernel (probEn)
    F.fuse_detections(dets, temperatures=T)                                   # proben_pack_kernel<LOGITS> + proben_fuse_kernel
    F.fuse_detections(dets, "probEn-log", temperatures=T)                     # proben_pack_kernel<LOGITS_LOGP> + logp fuse, uniform prior
    F.fuse_detections(dets, "probEn-log", temperatures=T, class_prior=prior)  # ... with a prior
torch.cuda.synchronize()
out = F.fuse_detections(dets, "probEn-log", temperatures=T)
torch.cuda.synchronize()
print("rows in", int(out["in_counts"].sum()), "fused rows", int(out["counts"].sum()), "finite", bool(torch.isfinite(out["scores"][(torch.arange(out["stride"], device="cuda")[None] < out["counts"][:, None]).reshape(-1)]).all()))
