"""Two restatements of weighted boxes fusion (Solovyev, Wang, Gabruseva 2021) for tests/test_wbf_{cpu,gpu}.py, both
written from the rule as DESIGN.md states it, and the seeded inputs the two files share.

numpy_rule   float64, every operation of the rule in the rule's order, each rounded on its own: what csrc/wbf.hip computes, bit for bit.
textbook     keeps member LISTS and recomputes each fused box from all its members in np.longdouble whenever a row joins, as the
             published implementation does; IoUs and conf in longdouble too.  The value the float64 running sums are measured against.

Both take one image: boxes [n, 4], scores [n], classes [n], source [n], the detector weights u [D], thr, skip, K, and return a dict:
  boxes f64 [M, 4] (textbook: longdouble), scores f32 [M] (textbook: "conf" longdouble only), classes f32 [M], members i32 [M],
  cluster i32 [n] (-1 = skipped), count M, skipped, "rows": per output row the input rows of its cluster in joining order,
  "margin": the smallest |iou - thr| over every IoU the walk evaluated (inf when it evaluated none)."""
import numpy as np

U53 = 2.0 ** -53


def _kept(boxes, scores, classes, source, u, skip, K, dtype):
    """s per row and the rows that take part, in visiting order: s descending, ties by original index descending."""
    D = len(u)
    s = np.zeros(len(scores), dtype=dtype)
    keep = []
    with np.errstate(all="ignore"):
        for r in range(len(scores)):
            ok = 0 <= source[r] < D and 0 <= classes[r] < K
            if ok:
                s[r] = dtype(scores[r]) * dtype(u[source[r]])
            ok = ok and bool(np.all(np.isfinite(boxes[r]))) and bool(np.isfinite(s[r])) and bool(s[r] > 0) and not bool(s[r] < skip)
            if ok:
                keep.append(r)
    keep.sort(key=lambda r: (-s[r], -r))
    return s, keep


def _iou(F, b, dtype):
    """IoU of the fused boxes F [m, 4] with the box b [4]: continuous areas, C's fmax / fmin, every operation rounded on its own."""
    zero = dtype(0)
    w = np.fmax(zero, np.fmin(F[:, 2], b[2]) - np.fmax(F[:, 0], b[0]))
    h = np.fmax(zero, np.fmin(F[:, 3], b[3]) - np.fmax(F[:, 1], b[1]))
    inter = w * h
    return inter / ((F[:, 2] - F[:, 0]) * (F[:, 3] - F[:, 1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def _first_max(iou):
    """(index, value) of the first maximum, a NaN never winning; (-1, -inf) when nothing exceeds -inf."""
    best, at = -np.inf, -1
    for j, v in enumerate(iou):
        if v > best:
            best, at = v, j
    return at, best


def _finish(clusters, conf, n_rows, skipped, margin, box_dtype):
    """Output order (conf descending - a NaN first -, class ascending, creation ascending) and the result dict."""
    order = sorted(range(len(clusters)), key=lambda i: (0 if conf[i] != conf[i] else 1, -float(conf[i]) if conf[i] == conf[i] else 0.0,
                                                        clusters[i]["class"], clusters[i]["created"]))
    cluster = np.full(n_rows, -1, dtype=np.int32)
    for pos, i in enumerate(order):
        cluster[clusters[i]["rows"]] = pos
    return {"boxes": np.array([clusters[i]["F"] for i in order], dtype=box_dtype).reshape(-1, 4),
            "conf": np.array([conf[i] for i in order], dtype=box_dtype),
            "scores": np.array([np.float32(conf[i]) for i in order], dtype=np.float32),
            "classes": np.array([clusters[i]["class"] for i in order], dtype=np.float32),
            "members": np.array([len(clusters[i]["rows"]) for i in order], dtype=np.int32),
            "cluster": cluster, "count": len(order), "skipped": skipped, "rows": [list(clusters[i]["rows"]) for i in order],
            "margin": margin}


def numpy_rule(boxes, scores, classes, source, u, thr=0.55, skip=0.0, K=3):
    f8 = np.float64
    boxes = np.asarray(boxes, dtype=f8).reshape(-1, 4)
    scores, classes, source = np.asarray(scores, dtype=f8), np.asarray(classes, dtype=np.int64), np.asarray(source, dtype=np.int64)
    u = np.asarray(u, dtype=f8)
    U = f8(0)
    for x in u:
        U = U + x
    s, keep = _kept(boxes, scores, classes, source, u, skip, K, f8)
    per_class, clusters, margin = {}, [], np.inf
    with np.errstate(all="ignore"):
        for r in keep:
            mine = per_class.setdefault(int(classes[r]), [])
            b = boxes[r]
            at, best = -1, -np.inf
            if mine:
                iou = _iou(np.array([c["F"] for c in mine], dtype=f8), b, f8)
                at, best = _first_max(iou)
                finite = iou[np.isfinite(iou)]
                margin = min(margin, float(np.min(np.abs(finite - thr)))) if finite.size else margin
            if at >= 0 and best > thr:
                c = mine[at]
            else:
                c = {"S": f8(0), "X": np.zeros(4, dtype=f8), "rows": [], "class": int(classes[r]), "created": len(mine)}
                mine.append(c)
                clusters.append(c)
            c["S"] = c["S"] + s[r]
            c["X"] = c["X"] + s[r] * b              # the product rounded, then the add
            c["rows"].append(r)
            c["F"] = c["X"] / c["S"]
        conf = [((c["S"] / f8(len(c["rows"]))) * np.fmin(f8(len(c["rows"])), U)) / U for c in clusters]
    return _finish(clusters, conf, len(scores), len(scores) - len(keep), margin, f8)


def textbook(boxes, scores, classes, source, u, thr=0.55, skip=0.0, K=3):
    ld = np.longdouble
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4).astype(ld)
    scores, classes, source = np.asarray(scores, dtype=np.float64), np.asarray(classes, dtype=np.int64), np.asarray(source, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64).astype(ld)
    U = u.sum()
    s, keep = _kept(boxes, scores, classes, source, u, ld(skip), K, ld)
    per_class, clusters, margin = {}, [], np.inf
    with np.errstate(all="ignore"):
        for r in keep:
            mine = per_class.setdefault(int(classes[r]), [])
            at, best = -1, -np.inf
            if mine:
                iou = _iou(np.array([c["F"] for c in mine], dtype=ld), boxes[r], ld)
                at, best = _first_max(iou)
                finite = iou[np.isfinite(iou)]
                margin = min(margin, float(np.min(np.abs(finite - ld(thr))))) if finite.size else margin
            if at >= 0 and best > ld(thr):
                c = mine[at]
            else:
                c = {"rows": [], "class": int(classes[r]), "created": len(mine)}
                mine.append(c)
                clusters.append(c)
            c["rows"].append(r)
            w = s[c["rows"]]
            c["F"] = (w[:, None] * boxes[c["rows"]]).sum(axis=0) / w.sum()         # from all the members, every time
        conf = [s[c["rows"]].sum() / ld(len(c["rows"])) * min(ld(len(c["rows"])), U) / U for c in clusters]
    return _finish(clusters, conf, len(scores), len(scores) - len(keep), margin, ld)


# The three hand cases of DESIGN.md section 29: D = 2, u = 1, 1, one class, rows in detector order.
HAND = {
    "joins_the_fused_box_only": dict(boxes=[[0, 0, 100, 100], [-1, -4, 68, 109], [18, -8, 83, 133]], scores=[0.9, 0.89, 0.88], thr=0.55),
    "matches_the_pivot_not_the_fused_box": dict(boxes=[[0, 0, 100, 100], [-31, -1, 98, 80], [10, 29, 102, 100]], scores=[0.9, 0.89, 0.88],
                                                thr=0.55),
    "exactly_at_the_threshold": dict(boxes=[[0, 0, 3, 1], [1, 0, 4, 1]], scores=[0.9, 0.8], thr=0.5),
}


def hand_case(name):
    c = HAND[name]
    n = len(c["scores"])
    return dict(boxes=np.array(c["boxes"], dtype=np.float64), scores=np.array(c["scores"], dtype=np.float64),
                classes=np.zeros(n, dtype=np.int32), source=np.array([0, 1, 0][:n], dtype=np.int32), u=[1.0, 1.0], thr=c["thr"], skip=0.0,
                K=1)


WEIGHTS3 = [1.0, 0.7, 1.3]


def random_set(seed, max_rows=200, K=3, D=3):
    """A seeded image of up to max_rows rows: objects at shared centres (all coordinates positive), each seen by some of the D detectors
    with a jittered box, a few detectors seeing one twice, and some clutter; rows in detector order."""
    rng = np.random.default_rng(seed)
    n_obj = int(rng.integers(max_rows // 8, max_rows // 3))
    cx, cy = rng.uniform(80, 560, n_obj), rng.uniform(80, 440, n_obj)
    w, h = rng.uniform(20, 90, n_obj), rng.uniform(20, 90, n_obj)
    cls = rng.integers(0, K, n_obj)
    rows = []
    for d in range(D):
        for o in range(n_obj):
            for _ in range(int(rng.choice([0, 1, 1, 1, 2]))):
                j = rng.normal(0.0, 0.05, 4) * np.array([w[o], h[o], w[o], h[o]])
                box = [cx[o] - w[o] / 2 + j[0], cy[o] - h[o] / 2 + j[1], cx[o] + w[o] / 2 + j[2], cy[o] + h[o] / 2 + j[3]]
                rows.append((d, box, rng.uniform(0.05, 1.0), int(cls[o]) if rng.random() < 0.9 else int(rng.integers(0, K))))
        for _ in range(int(rng.integers(0, 6))):
            x, y = rng.uniform(10, 560), rng.uniform(10, 440)
            rows.append((d, [x, y, x + rng.uniform(5, 60), y + rng.uniform(5, 60)], rng.uniform(0.05, 0.6), int(rng.integers(0, K))))
    if len(rows) > max_rows:            # thin evenly, keeping the detector order
        rows = [rows[i] for i in sorted(rng.choice(len(rows), max_rows, replace=False))]
    return dict(boxes=np.array([r[1] for r in rows], dtype=np.float64), scores=np.array([r[2] for r in rows], dtype=np.float64),
                classes=np.array([r[3] for r in rows], dtype=np.int32), source=np.array([r[0] for r in rows], dtype=np.int32),
                u=WEIGHTS3[:D], thr=0.55, skip=0.0, K=K)
