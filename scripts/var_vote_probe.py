"""Variance voting after the box-head NMS (profiles/var_voting.txt): what pe_boxhead_var_vote costs next to
pe_boxhead_finalize on a 32-image step at the bench's box-head settings, and what it does to the boxes of a pseudo-trained head.

    python scripts/var_vote_probe.py [--images 32] [--objects 8] [--launches 20] [--sigma_t 0.025]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/var_vote_probe.py

Box-head settings of bench.py's detectors (rcnn.DetectorConfig defaults, K = 3): 1 000 proposals per image, SCORE_THRESH_TEST 0.5 (so at
most 1 000 candidates), NMS 0.5, 100 detections, 800 x 1 000 resized images rescaled to 512 x 640.  There are no trained heads offline, so
the head is written by hand ("pseudo-trained"): per image --objects ground-truth boxes; 85 % of the proposals are jittered copies of a
ground-truth box, the rest random; a proposal with IoU >= 0.5 to a ground truth gets that object's class with a confident logit, its
deltas are the exact regression target plus N(0, var) noise per delta and its log-variance is log(var), var log-uniform in [1e-2, 1] in
box-delta units - a head whose variance is honest.  The step goes through GeneralizedRCNN._roi_heads(head=...): candidates, NMS, (vote,)
finalize.  Every image's candidates fit one PE_VAR_VOTE_TILE, so the kernel stages them once - the regime of the detectors' settings, not
the re-staging one of lists beyond 4 096 candidates.  Prints the workload, device-event times of the whole box-head step with and without voting, and the mean IoU to the ground
truth of the matched detections (best IoU >= 0.5, same class) with and without voting - a figure of this synthetic head, no AP claim."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proben_amd  # noqa: E402,F401
from proben_amd.rcnn import DetectorConfig, GeneralizedRCNN  # noqa: E402
from proben_amd.synthetic import synthetic_state_dict  # noqa: E402


def iou_matrix(a, b):
    w = np.clip(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0, None)
    h = np.clip(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0, None)
    inter = w * h
    area = lambda x: (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])      # noqa: E731
    return inter / np.maximum(area(a)[:, None] + area(b)[None, :] - inter, 1e-12)


def build(rng, N, P, K, G, stride, hw):
    ih, iw = hw
    head = np.zeros((N, P, stride), dtype=np.float32)
    props = np.zeros((N, P, 4), dtype=np.float32)
    gts, gcls = [], []
    for n in range(N):
        x1, y1 = rng.uniform(0, iw - 260, G), rng.uniform(0, ih - 260, G)
        gt = np.stack([x1, y1, x1 + rng.uniform(40, 250, G), y1 + rng.uniform(40, 250, G)], 1)
        cls = rng.integers(0, K, G)
        g = rng.integers(0, G, P)
        wh = np.stack([gt[g, 2] - gt[g, 0], gt[g, 3] - gt[g, 1]] * 2, 1)
        p = gt[g] + rng.normal(0, 0.12, (P, 4)) * wh
        rnd = rng.random(P) > 0.85
        rx, ry = rng.uniform(0, iw - 200, P), rng.uniform(0, ih - 200, P)
        p[rnd] = np.stack([rx, ry, rx + rng.uniform(30, 200, P), ry + rng.uniform(30, 200, P)], 1)[rnd]
        p = np.stack([np.clip(p[:, 0], 0, iw - 8), np.clip(p[:, 1], 0, ih - 8), p[:, 2], p[:, 3]], 1)
        p[:, 2], p[:, 3] = np.clip(np.maximum(p[:, 2], p[:, 0] + 8), 0, iw), np.clip(np.maximum(p[:, 3], p[:, 1] + 8), 0, ih)
        iou = iou_matrix(p, gt)
        best = iou.argmax(1)
        fg = iou[np.arange(P), best] >= 0.5
        t = gt[best]
        pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
        target = np.stack([10 * ((t[:, 0] + t[:, 2]) / 2 - (p[:, 0] + p[:, 2]) / 2) / pw, 10 * ((t[:, 1] + t[:, 3]) / 2 - (p[:, 1] + p[:, 3]) / 2) / ph,
                           5 * np.log((t[:, 2] - t[:, 0]) / pw), 5 * np.log((t[:, 3] - t[:, 1]) / ph)], 1)
        var = np.exp(rng.uniform(np.log(1e-2), np.log(1.0), P))
        d = target + rng.normal(0, 1, (P, 4)) * np.sqrt(var)[:, None]
        head[n, :, :K + 1] = rng.normal(0, 0.3, (P, K + 1))
        head[n, np.arange(P), np.where(fg, cls[best], K)] += rng.uniform(3, 6, P)
        for k in range(K):
            head[n, :, K + 1 + 4 * k:K + 5 + 4 * k] = d
        head[n, :, 5 * K + 1] = np.log(var)
        props[n] = p
        gts.append(gt)
        gcls.append(cls)
    return head, props, gts, gcls


def matched_iou(det, gts, gcls, scale):
    """Mean IoU to the ground truth of the detections whose best same-class ground truth has IoU >= 0.5; the number of such detections."""
    tot, cnt = 0.0, 0
    counts = det["counts"].cpu().numpy()
    boxes, classes = det["boxes"].cpu().numpy().astype(np.float64), det["classes"].cpu().numpy()
    for n, m in enumerate(counts):
        if m == 0:
            continue
        iou = iou_matrix(boxes[n, :m], gts[n] * scale)
        iou = np.where(classes[n, :m, None] == gcls[n][None, :], iou, 0.0)
        b = iou.max(1)
        tot, cnt = tot + b[b >= 0.5].sum(), cnt + int((b >= 0.5).sum())
    return tot / max(cnt, 1), cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--sigma_t", type=float, default=0.025)
    a = ap.parse_args()
    rng = np.random.default_rng(31)
    N, K, hw, out_hw = a.images, 3, (800, 1000), (512, 640)
    cfgs = {v: DetectorConfig(num_classes=K, var_voting=v, var_voting_sigma_t=a.sigma_t, fix_vars=True) for v in (False, True)}
    model = GeneralizedRCNN(cfgs[False], synthetic_state_dict(50, K, 3, seed=1))
    P = cfgs[False].post_nms_topk
    head, props, gts, gcls = build(rng, N, P, K, a.objects, model.w.head_stride, hw)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()      # noqa: E731
    ins = (dev(props), dev(np.full(N, P, dtype=np.int32)), dev(np.tile(np.array(hw, dtype=np.int32), (N, 1))),
           dev(np.tile(np.array(out_hw, dtype=np.int32), (N, 1))))
    hd = dev(head.reshape(N * P, -1))
    res = {}
    for v in (False, True):
        model.cfg = cfgs[v]
        for _ in range(3):
            det = model._roi_heads(None, *ins, N, head=hd)
        times = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            det = model._roi_heads(None, *ins, N, head=hd)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        res[v] = (det, times)
    cand = (res[True][0]["cand_total"].cpu().numpy(), res[True][0]["counts"].cpu().numpy())
    print(f"{N} images of {hw[1]} x {hw[0]} -> {out_hw[1]} x {out_hw[0]}, {P} proposals and {a.objects} objects each, K = {K}: candidates per image "
          f"mean {cand[0].mean():.0f} (min {cand[0].min()}, max {cand[0].max()}), detections per image mean {cand[1].mean():.1f}; sigma_t {a.sigma_t}")
    for v in (False, True):
        t = res[v][1]
        print(f"box-head step (candidates, NMS, {'vote, ' if v else ''}finalize; allocations included), device events: median "
              f"{np.median(t) * 1e3:.1f} us, min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f} over {a.launches} steps")
    scale = np.array([out_hw[1] / hw[1], out_hw[0] / hw[0]] * 2)
    for v in (False, True):
        m, c = matched_iou(res[v][0], gts, gcls, scale)
        print(f"mean IoU to ground truth of matched detections, var_voting {'on ' if v else 'off'}: {m:.4f} over {c} detections")
    off, on = res[False][0], res[True][0]
    counts = off["counts"].cpu().tolist()
    same = torch.equal(off["counts"], on["counts"]) and all(
        torch.equal(off[k][n, :m], on[k][n, :m]) for k in ("scores", "classes", "class_logits", "prob_score", "vars", "rows") for n, m in enumerate(counts))
    print("every field but the boxes is identical with and without voting (over the detections of every image):", same)


if __name__ == "__main__":
    main()
