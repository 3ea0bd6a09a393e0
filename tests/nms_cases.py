"""Shared code of tests/test_nms_edges_gpu.py (asserts on csrc/nms.hip) and tests/test_nms_edges_cpu.py (asserts on this file and
on oracle/nms.py): case builders for the places where an index-exact NMS goes wrong without a random test noticing - IoU exactly
at the threshold, degenerate boxes, non-finite scores and coordinates, and the size seams of the kernels.  Plain numpy, no GPU.

A case is the argument list of layers.nms_batched_raw plus what it claims to contain:
    Case(boxes [B,n,4] f32, scores [B,n] f32, idxs [B,n] i32 | None, counts [B] i32 | None, valid [B,n] u8 | None,
         thr, mode (0 = coordinate trick, 1 = per class), max_out, claims)
get(name) builds a case once, want(name) is the oracle's keep list per image (row ids of the call, first max_out of them), and
expected(case, rule) restates the same call under a deliberately WRONG rule (Rule): a case earns its place only if some wrong
rule keeps something else than the right one (tests/test_nms_edges_cpu.py).

Exactness of the threshold family.  Pair k is [0, 4k, q, 4k+1] and [0, 4k, p, 4k+1] with integers p < q <= 4096: both areas, the
intersection p and the union q + p - p are integers below 2^24, exact in float32 in any order of evaluation, so the only rounding
is the division and the IoU is fl(p / q).  Pairs are 4 apart in y and never touch.  The coordinate trick adds
idx * (max_coord + 1) <= 79 * 9218, an integer: everything stays an exact integer below 2^24."""
import functools
import math
from fractions import Fraction
from typing import NamedTuple, Optional

import numpy as np

from oracle import nms as O

F32 = np.float32
NAN_BITS = [0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFFFFFFF]     # the four of tests/test_rpn_select_gpu.py::NAN_BITS
INF = float("inf")


class Case(NamedTuple):
    boxes: np.ndarray
    scores: np.ndarray
    idxs: Optional[np.ndarray]
    counts: Optional[np.ndarray]
    valid: Optional[np.ndarray]
    thr: float
    mode: int
    max_out: int
    claims: dict


def bits_f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def seed_of(*key):
    s = 0
    for c in repr(key):
        s = (s * 131 + ord(c)) % (2 ** 31 - 1)
    return s


def n_pad_of(n):
    p = 64
    while p < n:
        p <<= 1
    return p


# ------------------------------------------------------------------------------------------------ the call under a rule
class Rule(NamedTuple):
    order: str = "torch"      # "torch" | "nan_last" | "nan_by_sign" | "tie_high"
    ge: bool = False          # suppress at IoU >= thr
    f64: bool = False         # IoU and comparison in float64
    plus_one: bool = False    # the legacy pixel convention: widths and heights + 1


RIGHT = Rule()
NAN_LAST = Rule(order="nan_last")         # what a negated-key argsort does
NAN_BY_SIGN = Rule(order="nan_by_sign")   # what a sign-magnitude integer key does: +NaN above +Inf, -NaN below -Inf
TIE_HIGH = Rule(order="tie_high")         # an unstable sort that lets the later row win a tie
GE = Rule(ge=True)
F64 = Rule(f64=True)
PLUS_ONE = Rule(plus_one=True)


def order_under(scores, rule):
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    if rule.order == "torch":
        return O.order_desc_stable(s)
    if rule.order == "nan_last":
        return np.argsort(-s.astype(np.float64), kind="stable")
    if rule.order == "nan_by_sign":
        u = f32_bits(np.where(s == 0, F32(0), s)).astype(np.int64)
        key = np.where(u >> 31 != 0, u ^ 0xFFFFFFFF, u ^ 0x80000000)
        return np.argsort(-key, kind="stable")
    if rule.order == "tie_high":
        return (len(s) - 1 - O.order_desc_stable(s[::-1])).astype(np.int64)
    raise AssertionError(rule.order)


def nms_under(boxes, scores, thr, rule):
    """oracle.nms.nms_f32 with the rule's order, comparison, precision and width convention (RIGHT reproduces it)."""
    dt = np.float64 if rule.f64 else np.float32
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4).astype(dt)
    n = len(b)
    if n == 0:
        return np.zeros((0,), dtype=np.int64)
    one, zero, t = dt(1 if rule.plus_one else 0), dt(0), dt(np.float32(thr))
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    order = order_under(scores, rule)
    suppressed = np.zeros(n, dtype=bool)
    keep = []
    with np.errstate(all="ignore"):
        areas = (x2 - x1 + one) * (y2 - y1 + one)
        for _i in range(n):
            i = order[_i]
            if suppressed[i]:
                continue
            keep.append(i)
            rest = order[_i + 1:]
            rest = rest[~suppressed[rest]]
            if len(rest) == 0:
                continue
            w = np.maximum(zero, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + one)
            h = np.maximum(zero, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + one)
            inter = w * h
            ovr = inter / (areas[i] + areas[rest] - inter)
            suppressed[rest[(ovr >= t) if rule.ge else (ovr > t)]] = True
    return np.asarray(keep, dtype=np.int64)


def batched_under(boxes, scores, idxs, thr, mode, rule, restate=False):
    """One image's call: the oracle itself under RIGHT (restate: this file's restatement of it, which the wrong rules go
    through), the restatement under any other rule."""
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    if boxes.size == 0:
        return np.zeros((0,), dtype=np.int64)
    with np.errstate(all="ignore"):
        if rule == RIGHT and not restate:
            return O.batched_nms_f32(boxes, scores, idxs, thr, mode="trick" if mode == 0 else "vanilla")
        if mode == 0:
            offsets = idxs.astype(np.float32) * (boxes.max() + np.float32(1))
            return nms_under(boxes + offsets[:, None], scores, thr, rule)
    keep_mask = np.zeros(len(scores), dtype=bool)
    for c in np.unique(idxs):
        sel = np.nonzero(idxs == c)[0]
        keep_mask[sel[nms_under(boxes[sel], scores[sel], thr, rule)]] = True
    kept = np.nonzero(keep_mask)[0]
    return kept[order_under(scores[kept], rule)]


def live_rows(case, b):
    n = case.scores.shape[1]
    m = np.ones(n, dtype=bool)
    if case.counts is not None:
        m &= np.arange(n) < min(int(case.counts[b]), n)
    if case.valid is not None:
        m &= case.valid[b] != 0
    return np.nonzero(m)[0]


def class_ids(case, b):
    return case.idxs[b] if case.idxs is not None else np.zeros(case.scores.shape[1], dtype=np.int32)


def expected(case, rule=RIGHT, all_survivors=False):
    """Per image: the rows the call keeps, in output order (the first max_out unless all_survivors)."""
    out = []
    for b in range(case.scores.shape[0]):
        live = live_rows(case, b)
        k = batched_under(case.boxes[b][live], case.scores[b][live], class_ids(case, b)[live], case.thr, case.mode, rule)
        out.append(live[k] if all_survivors else live[k][:case.max_out])
    return out


def zero_dead_rows(case):
    """The same call with every row that does not take part zeroed (boxes and scores)."""
    boxes, scores = case.boxes.copy(), case.scores.copy()
    for b in range(scores.shape[0]):
        dead = np.ones(scores.shape[1], dtype=bool)
        dead[live_rows(case, b)] = False
        boxes[b][dead] = 0
        scores[b][dead] = 0
    return case._replace(boxes=boxes, scores=scores)


def single(boxes, scores, idxs, thr, mode, max_out=None, **claims):
    n = len(scores)
    return Case(np.ascontiguousarray(boxes, dtype=np.float32).reshape(1, n, 4), np.ascontiguousarray(scores, dtype=np.float32).reshape(1, n),
                None if idxs is None else np.ascontiguousarray(idxs, dtype=np.int32).reshape(1, n), None, None,
                float(thr), mode, n if max_out is None else max_out, claims)


# ------------------------------------------------------------------------------------------------ threshold
THRESHOLDS = {"0.5": F32(0.5), "0.7": F32(0.7), "0.3": F32(0.3), "third": F32(1) / F32(3)}
QMAX = 4096


def classify(p, q, thr):
    """Which other ways of taking the decision fl(p/q) > thr get this pair wrong: "a" the quotient equals the threshold (a >=
    would suppress); "b" the exact rational comparison, "c" p * fl(1/q) > thr, "d" p > fl(thr * q) decide otherwise."""
    quot = F32(p) / F32(q)
    fp = bool(quot > thr)
    cls = "a" if quot == thr else ""
    if (Fraction(p, q) > Fraction(float(thr))) != fp:
        cls += "b"
    if bool(F32(p) * (F32(1) / F32(q)) > thr) != fp:
        cls += "c"
    if bool(F32(p) > thr * F32(q)) != fp:
        cls += "d"
    return cls


@functools.lru_cache(maxsize=None)
def threshold_pairs(tname):
    """Every (p, q, classes of classify()) with q <= QMAX whose float32 quotient is within 2 ulp of the threshold."""
    thr = THRESHOLDS[tname]
    tb = int(thr.view(np.int32))
    out = []
    for q in range(2, QMAX + 1):
        c = int(round(float(thr) * q))
        for p in (c - 1, c, c + 1):
            if not 1 <= p < q:
                continue
            quot = F32(p) / F32(q)
            if abs(int(quot.view(np.int32)) - tb) > 2:
                continue
            out.append((p, q, classify(p, q, thr)))
    return tuple(out)


WIDE = ("0.7", "0.3")       # the thresholds that have class (d) pairs with 2 q < 2^24 (0.5 has none at any size, 1/3 none below 2^23)
WIDE_PAIRS = 48


@functools.lru_cache(maxsize=None)
def threshold_pairs_wide(tname):
    """Class (d) has no member with q <= QMAX (tests/test_nms_edges_cpu.py says why), so it gets pairs of its own: the first
    WIDE_PAIRS (p, q) with 2^20 <= q < 2^23 at which p > fl(thr * q) decides otherwise than fl(p/q) > thr.  Still exact: the
    areas p and q and q + p are integers below 2^24 (one class only: the trick's offsets would not be)."""
    thr = THRESHOLDS[tname]
    out = []
    for q0 in range(1 << 20, 1 << 23, 1 << 18):
        q = np.arange(q0, q0 + (1 << 18), dtype=np.int64)
        p = np.floor(float(thr) * q).astype(np.int64) + 1
        dis = ((p.astype(np.float32) / q.astype(np.float32)) > thr) != (p.astype(np.float32) > thr * q.astype(np.float32))
        for pp, qq in zip(p[dis].tolist(), q[dis].tolist()):
            out.append((pp, qq, classify(pp, qq, thr)))
            if len(out) == WIDE_PAIRS:
                return tuple(out)
    raise AssertionError(tname)


def build_threshold_wide(tname):
    fam = threshold_pairs_wide(tname)
    pairs = []
    for j, (p, q, cls) in enumerate(fam):
        pairs.append((p, q, cls))
        if j % 8 == 0:
            pairs += [(p + 1000, q, "control"), (p - 1000, q, "control")]        # clearly above, clearly below
    m = len(pairs)
    rng = np.random.default_rng(seed_of("threshold wide", tname))
    boxes = np.zeros((2 * m, 4), dtype=np.float32)
    for k, (p, q, _) in enumerate(pairs):
        boxes[2 * k] = [0, 4 * k, q, 4 * k + 1]
        boxes[2 * k + 1] = [0, 4 * k, p, 4 * k + 1]
    scores = (rng.permutation(2 * m) + 1).astype(np.float32) / np.float32(8192)
    perm = rng.permutation(2 * m)
    thr = THRESHOLDS[tname]
    n_sup = sum(bool(F32(p) / F32(q) > thr) for p, q, _ in pairs)
    return single(boxes[perm], scores[perm], np.zeros(2 * m), thr, 1, family=len(fam), n_keep=2 * m - n_sup,
                  classes={c: sum(c in cls for _, _, cls in fam) for c in "abcd"},
                  wrong_d=sum(bool(F32(p) > thr * F32(q)) != bool(F32(p) / F32(q) > thr) for p, q, _ in pairs))


def build_threshold(tname, spread):
    """The family of threshold_pairs(tname), one pair per k, plus controls that are no part of the family: every 8th pair is
    followed by (p + 1, q), which IS suppressed - without them a kernel that never suppresses would pass.  spread: pairs over
    classes 0..79 in coordinate-trick mode; else one class."""
    fam = threshold_pairs(tname)
    pairs = []
    for j, (p, q, cls) in enumerate(fam):
        pairs.append((p, q, cls))
        if j % 8 == 0 and p + 1 < q:
            pairs.append((p + 1, q, "control"))
    m = len(pairs)
    rng = np.random.default_rng(seed_of("threshold", tname, spread))
    boxes = np.zeros((2 * m, 4), dtype=np.float32)
    pair_of = np.repeat(np.arange(m), 2)
    for k, (p, q, _) in enumerate(pairs):
        boxes[2 * k] = [0, 4 * k, q, 4 * k + 1]
        boxes[2 * k + 1] = [0, 4 * k, p, 4 * k + 1]
    scores = (rng.permutation(2 * m) + 1).astype(np.float32) / np.float32(8192)     # distinct, exact
    perm = rng.permutation(2 * m)
    boxes, scores, pair_of = boxes[perm], scores[perm], pair_of[perm]
    idxs = (pair_of % 80 if spread else np.zeros(2 * m)).astype(np.int32)
    n_control = sum(c == "control" for _, _, c in pairs)
    assert boxes.max() + 79 * (boxes.max() + 1) < 2 ** 24 and 2 * m * 4 <= 20000
    return single(boxes, scores, idxs, THRESHOLDS[tname], 0 if spread else 1, family=len(fam), controls=n_control,
                  classes={c: sum(c in cls for _, _, cls in fam) for c in "abcd"}, n_keep=2 * m - n_control)


# ------------------------------------------------------------------------------------------------ clusters
def clusters(rng, n_clusters, m_lo, m_hi, pitch=100, side=40, jitter=3):
    """n_clusters groups of m_lo..m_hi boxes, a side x side square moved by 0..jitter per coordinate: inside a group every IoU
    is at least (37 / 43)^2 ... > 0.74, groups are pitch apart and never touch.  Integer coordinates >= 0."""
    cols = int(math.ceil(math.sqrt(n_clusters)))
    boxes, cl = [], []
    for c in range(n_clusters):
        x0, y0 = (c % cols) * pitch, (c // cols) * pitch
        for _ in range(int(rng.integers(m_lo, m_hi + 1))):
            j = rng.integers(0, jitter + 1, 4)
            boxes.append([x0 + j[0], y0 + j[1], x0 + side + j[2], y0 + side + j[3]])
            cl.append(c)
    return np.asarray(boxes, dtype=np.float32), np.asarray(cl)


def distinct_scores(rng, n, lo=-1.0, hi=1.0):
    s = (lo + (hi - lo) * (rng.permutation(n) + 1) / (n + 1)).astype(np.float32)
    assert len(np.unique(s)) == n
    return s


# ------------------------------------------------------------------------------------------------ degenerate
def build_degenerate(spread):
    """Seven translated copies (1000 apart, so more than one 64-row tile) of: exact duplicates with tied and untied scores, zero-area
    boxes stacked on each other (0 / 0), a zero-area box inside a large one, inverted boxes (x2 < x1, and both axes), a box inside
    another at IoU 0.16."""
    proto = [
        ([10, 10, 50, 50], 0.8), ([10, 10, 50, 50], 0.8), ([10, 10, 50, 50], 0.8),          # duplicates, tied: the lowest row wins
        ([10, 110, 50, 150], 0.3), ([10, 110, 50, 150], 0.6),                                # duplicates, untied
        ([100, 100, 100, 100], 0.5), ([100, 100, 100, 100], 0.4), ([100, 100, 100, 100], 0.7),   # stacked points: 0 / 0, all stay
        ([120, 100, 120, 140], 0.2), ([120, 100, 120, 140], 0.9),                            # stacked zero-width segments
        ([200, 200, 300, 300], 0.75), ([250, 250, 250, 250], 0.1),                           # a point inside a large box: IoU 0
        ([400, 10, 380, 50], 0.65), ([400, 10, 380, 50], 0.55),                              # inverted in x, duplicates: area < 0, inter 0
        ([370, 0, 410, 60], 0.45),                                                           # a proper box over the inverted ones
        ([400, 150, 380, 110], 0.35), ([400, 150, 380, 110], 0.25),                          # inverted in both axes: area > 0, inter 0
        ([500, 500, 600, 600], 0.15), ([520, 520, 560, 560], 0.85),                          # contained, IoU 1600 / 10000
    ]
    rng = np.random.default_rng(seed_of("degenerate", spread))
    boxes, scores, idxs = [], [], []
    for j in range(7):
        order = rng.permutation(len(proto)) if j else np.arange(len(proto))
        for r in order:
            bx, s = proto[r]
            boxes.append([bx[0] + 1000 * j, bx[1], bx[2] + 1000 * j, bx[3]])
            scores.append(s)
            idxs.append(j % 3 if spread else 0)
    return single(boxes, scores, idxs, 0.5, 0 if spread else 1, n_keep=7 * (len(proto) - 3))


# ------------------------------------------------------------------------------------------------ non-finite scores
def special_scores():
    return np.concatenate([bits_f32(NAN_BITS), np.asarray([INF, -INF, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40], dtype=np.float32)])


def build_nonfinite_scores(variant):
    """Clusters of mutually suppressing boxes whose scores mix finite values with the four NaN patterns, +-Inf, +-0 and
    subnormals: exactly one row of a cluster survives, the first in the order.  variant "mixed": 5 classes, trick mode, rows in
    random order.  "row0_nan" / "row0_inf": >= 1024 rows handed over in (class, score) order - the presorted shortcut's input -
    with a NaN / +Inf score on row 0 of class 0."""
    rng = np.random.default_rng(seed_of("nonfinite_scores", variant))
    big = variant != "mixed"
    boxes, cl = clusters(rng, 300 if big else 60, 3, 5)
    n = len(cl)
    scores = distinct_scores(rng, n)
    sp = special_scores()
    if variant == "row0_inf":
        sp = sp[len(NAN_BITS):]
    starts = np.nonzero(np.r_[True, cl[1:] != cl[:-1]])[0]
    fixed = [[-0.0, 0.0, -1e-45], [0.0, -0.0, -1e-40], [NAN_BITS[1], NAN_BITS[0], INF], [INF, NAN_BITS[3], 0.5], [1e-45, 0.0, -0.0],
             [-INF, NAN_BITS[2], NAN_BITS[3]], [1e-40, 1e-45, 0.0], [-INF, -1.0, -1e-45]]
    t = 0
    for c, r0 in enumerate(starts):
        if c < len(fixed):
            vals = [bits_f32([v])[0] if isinstance(v, int) else np.float32(v) for v in fixed[c]]
            if variant == "row0_inf":
                vals = [v for v in vals if not np.isnan(v)]
            scores[r0:r0 + len(vals)] = vals
        else:
            m = (starts[c + 1] if c + 1 < len(starts) else n) - r0
            for r in rng.choice(m, size=2, replace=False):
                scores[r0 + r] = sp[t % len(sp)]
                t += 1
    idxs = (cl % 5).astype(np.int32)
    if big:
        rank = np.empty(n, dtype=np.int64)
        rank[O.order_desc_stable(scores)] = np.arange(n)
        perm = np.lexsort((rank, idxs))
        boxes, scores, idxs, cl = boxes[perm], scores[perm], idxs[perm], cl[perm]
    else:
        perm = rng.permutation(n)
        boxes, scores, idxs, cl = boxes[perm], scores[perm], idxs[perm], cl[perm]
    return single(boxes, scores, idxs, 0.5, 0, n_keep=len(starts), cluster=cl, presorted=big,
                  bits=sorted({int(b) for b in f32_bits(scores)[np.isnan(scores)]}))


# ------------------------------------------------------------------------------------------------ non-finite boxes
BAD = {"pinf": INF, "ninf": -INF, "nan": float("nan")}


def _bad_clusters(rng, n_clusters, ncls, val, m_lo=3, m_hi=5):
    """Clusters with finite, distinct scores; in every third cluster the best row gets `val` in one coordinate."""
    boxes, cl = clusters(rng, n_clusters, m_lo, m_hi)
    scores = distinct_scores(rng, len(cl), 0.0, 1.0)
    bad = []
    for c in range(0, n_clusters, 3):
        rows = np.nonzero(cl == c)[0]
        r = rows[np.argmax(scores[rows])]
        boxes[r, (c // 3) % 4] = val
        bad.append(r)
    perm = rng.permutation(len(cl))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return boxes[perm], scores[perm], (cl[perm] % ncls).astype(np.int32), cl[perm], np.sort(inv[np.asarray(bad)])


def build_nonfinite_boxes(form, vname):
    """form "nms": one class, no trick (the layers.nms route);  "trick": 5 classes, coordinate trick;  "class": 5 classes and more
    than 20000 box elements, batched_nms's per-class form;  "raw0" / "raw1": nms_batched_raw with counts and a row mask in trick
    / per-class mode."""
    rng = np.random.default_rng(seed_of("nonfinite_boxes", form, vname))
    val = BAD[vname]
    if form in ("nms", "trick", "class"):
        nc = {"nms": 60, "trick": 60, "class": 1300}[form]
        boxes, scores, idxs, cl, bad = _bad_clusters(rng, nc, 1 if form == "nms" else 5, val, *((4, 4) if form == "class" else (3, 5)))
        return single(boxes, scores, idxs, 0.5, 0 if form == "trick" else 1, clusters=nc, cluster=cl, bad=bad, value=vname)
    mode = {"raw0": 0, "raw1": 1}[form]
    parts = [_bad_clusters(rng, 70, 4, val) for _ in range(2)]
    n = min(len(p[1]) for p in parts)
    boxes = np.stack([p[0][:n] for p in parts])
    scores = np.stack([p[1][:n] for p in parts])
    idxs = np.stack([p[2][:n] for p in parts])
    counts = np.asarray([n - 17, n], dtype=np.int32)
    valid = (rng.random((2, n)) > 0.1).astype(np.uint8)
    bad = [p[4][p[4] < n] for p in parts]
    for b in range(2):
        valid[b, bad[b][::2]] = 1                      # half of the planted rows certainly take part
    return Case(boxes, scores, idxs, counts, valid, 0.5, mode, n, dict(bad=bad, value=vname))


def build_dead_rows(mode):
    """Finite clusters with coordinates >= 0; NaN, +-Inf, a -5 (it would flip the image to the all-pairs route) and a 1e30 (as
    max_coord it would swamp every coordinate of classes >= 1) sit only in rows that take no part: image 0 masks them out,
    image 1 has them beyond counts."""
    rng = np.random.default_rng(seed_of("dead_rows", mode))
    vals = [float("nan"), INF, -INF, -5.0, 1e30]
    per = []
    for _ in range(2):
        boxes, cl = clusters(rng, 70, 3, 5)
        perm = rng.permutation(len(cl))
        per.append((boxes[perm], distinct_scores(rng, len(cl), 0.0, 1.0), (cl[perm] % 4).astype(np.int32)))
    n = min(len(p[1]) for p in per)
    boxes = np.stack([p[0][:n] for p in per])
    scores = np.stack([p[1][:n] for p in per])
    idxs = np.stack([p[2][:n] for p in per])
    valid = np.ones((2, n), dtype=np.uint8)
    dead0 = rng.choice(n, size=20, replace=False)
    valid[0, dead0] = 0
    counts = np.asarray([n, n - 20], dtype=np.int32)
    dead = [dead0, np.arange(n - 20, n)]
    for b in range(2):
        for j, r in enumerate(dead[b]):
            boxes[b, r, j % 4] = vals[j % len(vals)]
        scores[b, dead[b][:4]] = bits_f32(NAN_BITS)     # the best score there is, on rows that are not there
    return Case(boxes, scores, idxs, counts, valid, 0.5, mode, n, dict(dead=dead))


# ------------------------------------------------------------------------------------------------ seams
def rand_boxes(rng, n, nseg):
    """Sides 20..80 on a square of 100 units of area per box of a class: about a third of the rows survive at IoU 0.5."""
    span = 10.0 * math.sqrt(n / nseg)
    xy = rng.uniform(0, span, (n, 2))
    return np.concatenate([xy, xy + rng.uniform(20, 80, (n, 2))], 1).astype(np.float32)


RUNS_1024 = [128, 64, 64, 1, 1] + [64] * 11 + [62]            # 17 classes, 1024 rows
SEAMS = {
    # name: n, class layout (segs = that many classes at random | runs = rows per class), max_out (None = n), rows handed over
    # in (class, score) order (the presorted shortcut fires), mode
    "n1": dict(n=1, segs=1),
    "n2": dict(n=2, segs=1),
    "n63": dict(n=63, segs=1),
    "n64": dict(n=64, segs=1, mode=1),
    "n65": dict(n=65, segs=1),
    "n128_runs64": dict(n=128, runs=[64, 64], sorted=True),
    "n129_runs64_1": dict(n=129, runs=[64, 64, 1], sorted=True, mode=1),
    "n1023_16seg": dict(n=1023, segs=16, sorted=True),
    "n1024_runs": dict(n=1024, runs=RUNS_1024, sorted=True),
    "n1024_17seg_unsorted": dict(n=1024, segs=17, mode=1),
    "n1025_1seg": dict(n=1025, segs=1, sorted=True),
    "n1025_17seg_out1": dict(n=1025, segs=17, max_out=1),
    "n1025_17seg_out63": dict(n=1025, segs=17, max_out=63, sorted=True),
    "n1025_16seg_out64": dict(n=1025, segs=16, max_out=64, sorted=True),
    "n1025_16seg_out65": dict(n=1025, segs=16, max_out=65),
    "n2049_16seg_out64": dict(n=2049, segs=16, max_out=64, sorted=True),
    "n2049_17seg": dict(n=2049, segs=17, sorted=True, mode=1),
    "n16076_16seg": dict(n=16076, segs=16, sorted=True),         # the last size at which the survivors' keys fit: merge by rank
    "n16077_16seg": dict(n=16077, segs=16),                      # the first at which they do not: sorting network
    # where that boundary stood while the bound forgot the kernel's static LDS: a call with 16128 rows was refused (LDS request)
    "n16128_16seg": dict(n=16128, segs=16, sorted=True),
    "n16129_16seg": dict(n=16129, segs=16),
    "n16384_17seg": dict(n=16384, segs=17, sorted=True),         # the row limit
}


def build_seam(name):
    """A seed whose case suppresses nothing (or everything) is no use: the small sizes take the first seed that does both."""
    for attempt in range(64):
        case = _build_seam(name, attempt)
        n = SEAMS[name]["n"]
        if n < 2 or n > 128 or 0 < len(expected(case, all_survivors=True)[0]) < n:
            return case
    raise AssertionError(name)


def _build_seam(name, attempt):
    spec = SEAMS[name]
    n = spec["n"]
    rng = np.random.default_rng(seed_of("seam", name, attempt))
    boxes = rand_boxes(rng, n, len(spec["runs"]) if "runs" in spec else spec["segs"])
    scores = distinct_scores(rng, n, 0.0, 1.0)
    if "runs" in spec:
        assert sum(spec["runs"]) == n
        idxs = rng.permutation(np.repeat(np.arange(len(spec["runs"])), spec["runs"]))
    else:
        idxs = rng.integers(0, spec["segs"], n)
        idxs[rng.permutation(n)[:min(n, spec["segs"])]] = np.arange(min(n, spec["segs"]))      # every class is there
    if spec.get("sorted"):
        perm = np.lexsort((-scores.astype(np.float64), idxs))
        boxes, scores, idxs = boxes[perm], scores[perm], idxs[perm]
    return single(boxes, scores, idxs, 0.5, spec.get("mode", 0), spec.get("max_out"), nseg=len(np.unique(idxs)),
                  presorted=bool(spec.get("sorted")), truncates=spec.get("max_out") is not None,
                  runs=sorted(np.bincount(idxs).tolist()))


def build_disjoint():
    """One class: 2100 pairwise disjoint boxes, all of which survive, then 100 low-scored copies of survivors - 50 of survivors
    past the 1024th of the kept list, which only the second gather batch of the scan sees, 50 of earlier ones.  max_out = n."""
    rng = np.random.default_rng(seed_of("disjoint"))
    m = 2100
    i = np.arange(m)
    base = np.stack([(i % 50) * 10, (i // 50) * 10, (i % 50) * 10 + 8, (i // 50) * 10 + 8], 1).astype(np.float32)
    s = distinct_scores(rng, m, 0.5, 1.0)
    by_rank = np.argsort(-s.astype(np.float64), kind="stable")
    late, early = rng.choice(by_rank[1024:], 50, replace=False), rng.choice(by_rank[:1024], 50, replace=False)
    boxes = np.concatenate([base, base[late], base[early]])
    scores = np.concatenate([s, distinct_scores(rng, 100, 0.0, 0.4)])
    perm = rng.permutation(len(scores))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return single(boxes[perm], scores[perm], np.zeros(len(scores)), 0.5, 0, n_keep=m, copies=np.sort(inv[m:]), late=np.sort(inv[m:m + 50]))


def build_batch(kind):
    """Three images of 1025 rows in 16 classes, each handed over in (class, score) order.  "counts0": the middle image has
    counts == 0;  "valid0": all its rows are masked out and the other images lose a fifth of theirs."""
    rng = np.random.default_rng(seed_of("batch", kind))
    B, n = 3, 1025
    parts = []
    for _ in range(B):
        boxes, scores, idxs = rand_boxes(rng, n, 16), distinct_scores(rng, n, 0.0, 1.0), rng.integers(0, 16, n)
        perm = np.lexsort((-scores.astype(np.float64), idxs))
        parts.append((boxes[perm], scores[perm], idxs[perm].astype(np.int32)))
    boxes, scores, idxs = (np.stack([p[j] for p in parts]) for j in range(3))
    if kind == "counts0":
        counts, valid = np.asarray([n, 0, 700], dtype=np.int32), None
    else:
        counts, valid = None, (rng.random((B, n)) > 0.2).astype(np.uint8)
        valid[1] = 0
    return Case(boxes, scores, idxs, counts, valid, 0.5, 0, 200, dict(empty=1, presorted=True))


SCRATCH_N = (1, 65, 16383)


def build_scratch(n):
    """B = 3 for the scratch-size test: one image's rows three times, with counts n, n // 2 and 1."""
    rng = np.random.default_rng(seed_of("scratch", n))
    boxes, scores, idxs = rand_boxes(rng, n, 16), distinct_scores(rng, n, 0.0, 1.0), rng.integers(0, 16, n).astype(np.int32)
    counts = np.asarray([n, n // 2, 1], dtype=np.int32)
    return Case(np.stack([boxes] * 3), np.stack([scores] * 3), np.stack([idxs] * 3), counts, None, 0.5, 0, min(n, 300), {})


# ------------------------------------------------------------------------------------------------ registry
FAMILIES = {
    "threshold": {f"threshold_{t}_{'spread' if sp else 'one'}": functools.partial(build_threshold, t, sp)
                  for t in THRESHOLDS for sp in (False, True)},
    "threshold_wide": {f"threshold_{t}_wide": functools.partial(build_threshold_wide, t) for t in WIDE},
    "degenerate": {f"degenerate_{'spread' if sp else 'one'}": functools.partial(build_degenerate, sp) for sp in (False, True)},
    "nonfinite_scores": {f"scores_{v}": functools.partial(build_nonfinite_scores, v) for v in ("mixed", "row0_nan", "row0_inf")},
    "nonfinite_boxes": {f"boxes_{f}_{v}": functools.partial(build_nonfinite_boxes, f, v)
                        for f in ("nms", "trick", "class", "raw0", "raw1") for v in BAD},
    "dead_rows": {f"dead_rows_mode{m}": functools.partial(build_dead_rows, m) for m in (0, 1)},
    "seams": {**{f"seam_{k}": functools.partial(build_seam, k) for k in SEAMS},
              "seam_disjoint2100": build_disjoint,
              "seam_batch_counts0": functools.partial(build_batch, "counts0"),
              "seam_batch_valid0": functools.partial(build_batch, "valid0")},
    "scratch": {f"scratch_n{n}": functools.partial(build_scratch, n) for n in SCRATCH_N},
}
BUILDERS = {name: fn for fam in FAMILIES.values() for name, fn in fam.items()}


def names(*families):
    return [name for f in (families or FAMILIES) for name in FAMILIES[f]]


@functools.lru_cache(maxsize=None)
def get(name):
    case = BUILDERS[name]()
    for a in (case.boxes, case.scores, case.idxs, case.counts, case.valid):
        if a is not None:
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def want(name):
    return tuple(expected(get(name)))
