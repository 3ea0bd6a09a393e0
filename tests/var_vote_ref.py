"""The variance-voting rule of DESIGN.md section 31 (csrc/varvote.hip, pe_boxhead_var_vote), restated in NumPy float64 with exactly
rounded sums (math.fsum), and the small case builders tests/test_var_vote_cpu.py and tests/test_var_vote_gpu.py share.  No GPU.

For a kept candidate b of one image the voters are the candidates i with class_i == class_b, IoU(b, i) > 0 (finetune.pairwise_iou's
expression, float64) and a variance that is finite and > 0; p_i = exp(-(1 - IoU)^2 / sigma_t), w_i = p_i / var_i, and every
coordinate of b becomes sum(w_i x_i) / sum(w_i), rounded once to float32.  A kept box that is no voter of itself keeps its bits.
The variances are float32 numbers (exp of the candidate's own log-variance, taken in float32), sigma_t is the float32 the C-ABI
receives; both are widened to float64 before anything is computed."""
import math

import numpy as np

F32 = np.float32


def own_variances(head, orow, K):
    """var_c = exp(head[orow_c, 5K+1]) in float32: head [P, stride] float32 of one image, orow [C] -> [C] float32."""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(head, dtype=F32)[np.asarray(orow, dtype=np.int64), 5 * K + 1]).astype(F32)


def iou64(b, boxes):
    """finetune.pairwise_iou's expression for one box against [C, 4], float64: inter > 0 ? inter / union : 0."""
    b = np.asarray(b, dtype=np.float64)
    x = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        area_b = (b[2] - b[0]) * (b[3] - b[1])
        area = (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
        w = np.maximum(np.minimum(b[2], x[:, 2]) - np.maximum(b[0], x[:, 0]), 0.0)
        h = np.maximum(np.minimum(b[3], x[:, 3]) - np.maximum(b[1], x[:, 1]), 0.0)
        inter = w * h
        union = area_b + area - inter
        return np.where(inter > 0, inter / np.where(inter > 0, union, 1.0), 0.0)


def voters(boxes, classes, variances, b):
    """-> (ids of b's voters, ascending; their IoU with b)."""
    boxes = np.asarray(boxes, dtype=F32)
    v = np.asarray(variances, dtype=F32).astype(np.float64)
    iou = iou64(boxes[b], boxes)
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(classes) == np.asarray(classes)[b]) & (iou > 0) & np.isfinite(v) & (v > 0)
    ids = np.nonzero(ok)[0]
    return ids, iou[ids]


def vote_one(boxes, classes, variances, b, sigma_t):
    """The voted box of kept candidate b as float64 [4] (before the rounding to float32), or None when b is no voter of itself."""
    ids, iou = voters(boxes, classes, variances, b)
    if b not in ids.tolist():
        return None
    s = float(F32(sigma_t))
    x = np.asarray(boxes, dtype=F32).astype(np.float64)[ids]
    v = np.asarray(variances, dtype=F32).astype(np.float64)[ids]
    w = [math.exp(-((1.0 - float(u)) ** 2) / s) / float(q) for u, q in zip(iou, v)]
    sw = math.fsum(w)
    return np.array([math.fsum(wi * float(xi) for wi, xi in zip(w, x[:, c])) / sw for c in range(4)], dtype=np.float64)


def vote(boxes, classes, variances, keep, sigma_t):
    """One image: boxes [C, 4] float32, classes [C], variances [C] float32, keep = candidate ids -> out [C, 4] float32: the input with
    every kept row replaced by its voted box.  A keep id outside [0, C) is skipped."""
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    out = boxes.copy()
    for b in np.asarray(keep, dtype=np.int64).tolist():
        if not 0 <= b < len(boxes):
            continue
        r = vote_one(boxes, classes, variances, b, sigma_t)
        if r is not None:
            out[b] = r.astype(F32)
    return out


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32)


def within_one_ulp(got, want):
    """Every float32 of `got` is `want` or one of its two float32 neighbours."""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


# ------------------------------------------------------------------------------------------------ case builders
def random_pile(rng, count, K, image_hw=(512, 640), clusters=None, bad_fraction=0.0):
    """`count` clipped float32 boxes with positive extent around a few centres (so that many overlap), classes in [0, K), and float32
    log-variances in [-9, -2] (variances 1e-4 .. 0.1); bad_fraction of them -inf, +inf or NaN in turn (variance 0, inf, NaN)."""
    ih, iw = image_hw
    clusters = clusters or max(1, count // 12)
    cx, cy = rng.uniform(40, iw - 40, clusters), rng.uniform(40, ih - 40, clusters)
    sw, sh = rng.uniform(20, 120, clusters), rng.uniform(20, 120, clusters)
    g = rng.integers(0, clusters, count)
    x1 = cx[g] - 0.5 * sw[g] + rng.normal(0, 0.08, count) * sw[g]
    y1 = cy[g] - 0.5 * sh[g] + rng.normal(0, 0.08, count) * sh[g]
    x2 = cx[g] + 0.5 * sw[g] + rng.normal(0, 0.08, count) * sw[g]
    y2 = cy[g] + 0.5 * sh[g] + rng.normal(0, 0.08, count) * sh[g]
    boxes = np.stack([np.clip(x1, 0, iw), np.clip(y1, 0, ih), np.clip(x2, 0, iw), np.clip(y2, 0, ih)], 1).astype(F32)
    assert (boxes[:, 2] > boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all()
    classes = ((g + rng.integers(0, 2, count) * (rng.random(count) < 0.2)) % K).astype(np.int32)
    logvar = rng.uniform(-9.0, -2.0, count).astype(F32)
    bad = np.nonzero(rng.random(count) < bad_fraction)[0]
    logvar[bad] = np.array([-np.inf, np.inf, np.nan], dtype=F32)[np.arange(len(bad)) % 3]
    return boxes, classes, logvar


def recovery_piles(rng, piles=2000, per_pile=12, size=(100.0, 60.0)):
    """The recovery experiment of DESIGN.md section 31: per pile a ground-truth box of 100 x 60 and 12 candidates whose corner errors
    are N(0, var_i * size^2) per coordinate (size = the box's width for x, height for y), var_i log-uniform in [1e-4, 1e-2]; boxes and
    variances rounded to float32.  -> gt [piles, 4], boxes [piles, 12, 4] float32, variances [piles, 12] float32."""
    w, h = size
    x0, y0 = rng.uniform(50, 400, piles), rng.uniform(50, 300, piles)
    gt = np.stack([x0, y0, x0 + w, y0 + h], 1)
    var = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), (piles, per_pile)))
    scale = np.array([w, h, w, h])
    boxes = gt[:, None, :] + rng.normal(0.0, 1.0, (piles, per_pile, 4)) * np.sqrt(var)[..., None] * scale
    return gt, boxes.astype(F32), var.astype(F32)
