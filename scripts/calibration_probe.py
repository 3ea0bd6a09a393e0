"""rocprofv3 --kernel-trace --stats -- python scripts/calibration_probe.py  (profiles/calibration_trace.txt)
32-image, two-detector pack (parent kernel and calibrated kernel on the same detections, D = 100, 60-100 rows live) and
pe_temperature_nll at M = 10^6, n_t = 64: run under rocprofv3 --kernel-trace --stats."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import proben_amd  # noqa: F401
from proben_amd import fusion as F
from proben_amd.calibration import temperature_nll, calibrated_probs

rng = np.random.default_rng(0)
B, D, K = 32, 100, 3
dets = []
for d in range(2):
    x1 = rng.uniform(0, 500, (B, D)); y1 = rng.uniform(0, 400, (B, D))
    box = np.stack([x1, y1, x1 + 50, y1 + 60], 2).astype(np.float32)
    lg = rng.normal(0, 3, (B, D, K + 1)).astype(np.float32)
    e = np.exp(lg - lg.max(2, keepdims=True)); p = (e / e.sum(2, keepdims=True)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    dets.append({"boxes": t(box), "scores": t(p[..., :K].max(2)), "classes": t(p[..., :K].argmax(2).astype(np.int32)),
                 "prob_score": t(np.ascontiguousarray(p[..., :K])), "class_logits": t(lg), "vars": t(np.ones((B, D), np.float32)),
                 "counts": t(rng.integers(60, 101, B).astype(np.int32))})
for _ in range(50):
    F.pack_rows(dets, 2)
    F.pack_rows(dets, 2, (1.5, 0.8))
torch.cuda.synchronize()
M = 1_000_000
lg = torch.from_numpy(rng.normal(0, 3, (M, K + 1)).astype(np.float32)).cuda()
y = torch.from_numpy(rng.integers(0, K + 1, M).astype(np.int32)).cuda()
ts = np.exp(np.linspace(np.log(0.05), np.log(20), 64))
for _ in range(10):
    temperature_nll(lg, y, ts)
    calibrated_probs(lg, 1.5)
torch.cuda.synchronize()
print("profile workload done")
