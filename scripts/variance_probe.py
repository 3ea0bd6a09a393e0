"""Kernel-trace workload for the variance-calibration kernels (profiles/variance_trace.txt): one 32-image,
two-detector step (D = 100 rows per detector and image, 60-100 live, half of them overlapping the other detector's, K = 3), 50 times
each of: the plain pack, the calibrated pack (probabilities and logits routes), ground-truth matching of the step's detections
(32 images, 12 ground-truth boxes each) and the variance statistics of the matched rows; then 10 x the statistics at 10^6 rows.

    rocprofv3 --kernel-trace --stats -d OUT -o variance --output-format csv -- python scripts/variance_probe.py
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
# detector 0's live rows as flat matching input
cnt = dets[0]["counts"].cpu().numpy()
live = torch.from_numpy((np.arange(D)[None] < cnt[:, None])).cuda()
db = dets[0]["boxes"][live].double()
dv = dets[0]["vars"][live].double()
doff = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)).cuda()
gb = torch.from_numpy(gt.reshape(-1, 4)).cuda()
goff = torch.arange(0, B * G + 1, G, dtype=torch.int32, device="cuda")
gcls = torch.from_numpy(rng.integers(0, K, B * G).astype(np.int32)).cuda()
T, S = (1.5, 0.8), (0.4, 2.5)
for it in range(50):
    F.pack_rows(dets, 2)                                             # proben_pack_kernel<PROBS>
    F.pack_rows(dets, 2, variance_scales=S)                          # proben_pack_kernel<PROBS>, scaled (one launch)
    F.pack_rows(dets, 2, temperatures=T, variance_scales=S)          # proben_pack_kernel<LOGITS>, scaled (one launch)
    lab, match, iou = C.match_rows_device(db, doff, gb, goff, gcls, None, 0.5, K)     # match_ground_truth_kernel
    st = C.variance_stats(db, match, gb, dv)                         # variance_stats_kernel + variance_stats_finish_kernel
torch.cuda.synchronize()
M = 1_000_000
big = rng.integers(0, B * G, M)
bdet = gb[torch.from_numpy(big).cuda()] + torch.randn((M, 4), dtype=torch.float64, device="cuda") * 2
bvar = torch.rand((M,), dtype=torch.float64, device="cuda") * 0.1 + 1e-3
bm = torch.from_numpy(big.astype(np.int32)).cuda()
for it in range(10):
    big_st = C.variance_stats(bdet, bm, gb, bvar)
torch.cuda.synchronize()
print("step rows", int(db.shape[0]), "matched", int((match >= 0).sum()), "used", st["n"], "excluded", st["excluded"], "| 10^6 rows: used", big_st["n"])
