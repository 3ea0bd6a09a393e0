"""Shared code of tests/test_boxhead_edges_gpu.py (asserts on csrc/boxhead.hip) and tests/test_boxhead_edges_cpu.py (asserts on this
file and on oracle/detector.py): a plain numpy restatement of the box head's two kernels and the case builders for the places
where they go wrong without a random test noticing - the three row ids (post-filter frow, original orow, candidate id c), the
block scan and the finalize ballot at their 64-lane seams, the candidate cap, drop-empty, a score exactly on the threshold, the
decode clamp at +-inf, and memory that takes no part.  No GPU.

The restatement (candidates / keep_of / finalize, together run()) follows the header comment of csrc/boxhead.hip: float64 for the
arithmetic, exact integers for the indices, every intermediate returned.  It takes a `rule`: RIGHT, or one of the deliberately
WRONG rules below, each a one-line change HERE, never in the kernel.  A case earns its place only if some wrong rule changes an
exactly compared field of its expected output (tests/test_boxhead_edges_cpu.py holds the table).

Exact inputs.  Wherever a case is about indices, float32 and float64 agree bit for bit on the boxes: proposals have integer
corners and power-of-two extents >= 8, dx and dy are 10 * m / 8 with |m| <= 8 (so fl(d / 10) = m / 8 and every product, centre
and corner is a small dyadic number), dw = dh = 0 (exp(0) = 1) or -inf (exp = 0).  The rescale is ONE float32 product per
coordinate, and the float64 product of two float32 numbers is exact, so rounding it to float32 gives the float32 product: final
boxes are compared bit for bit whenever the candidate boxes are exact, at any output size (Case.exact_boxes).  The softmax is
not exact in either format (exp): scores and probs are compared within the project's tolerances to the restatement, and every
builder keeps each foreground probability MARGIN away from the threshold (the planted ties aside) and the scores of one image
GAP apart, so that the pass / fail decisions and the score order are the same in both formats.  Logits lie on a 2^-12 grid.
Log-variance of row r is r * Case.logvar_step (1/8; 1/16 at P = 1024, where exp(r / 8) leaves float32): every variance names
its row, and var_row() reads that name back as an integer that is compared exactly."""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import nms as O

F32 = np.float32
INF = float("inf")
NAN = float("nan")
SCALE_CLAMP = float(np.float32(np.log(1000.0 / 16)))      # what the kernel receives: the float32 of rcnn.SCALE_CLAMP
REG_W = (10.0, 10.0, 5.0, 5.0)
MARGIN = 1e-4       # |p - thr| of every foreground probability that is no planted tie
GAP = 4e-6          # relative distance of any two candidate scores of one image (the tolerance on a score is 2e-6 + 1e-7)
GUARD = 8           # entries behind every output array that no kernel may touch

RIGHT = "RIGHT"
THRESH_GE = "THRESH_GE"                             # >= instead of >
LOGITS_BY_OROW = "LOGITS_BY_OROW"                   # Q4 undone
PROBS_BY_FROW = "PROBS_BY_FROW"
VARS_IGNORE_FIX = "VARS_IGNORE_FIX"                 # fix_vars ignored
VARS_BY_FROW = "VARS_BY_FROW"
NO_CARRY = "NO_CARRY"                               # `written` reset per 64-lane round
CAP_LAST = "CAP_LAST"                               # the cap keeps the last cand_max candidates
ROW_DROP_PER_CLASS = "ROW_DROP_PER_CLASS"           # a non-finite class box drops that class only
KEEP_EMPTY = "KEEP_EMPTY"                           # no drop-empty
CLIP_BEFORE_SCALE_ONLY = "CLIP_BEFORE_SCALE_ONLY"   # no second clip to out_hw
WRONG_RULES = (THRESH_GE, LOGITS_BY_OROW, PROBS_BY_FROW, VARS_IGNORE_FIX, VARS_BY_FROW, NO_CARRY, CAP_LAST, ROW_DROP_PER_CLASS,
               KEEP_EMPTY, CLIP_BEFORE_SCALE_ONLY)


class Case(NamedTuple):
    head: np.ndarray                    # [N, P, stride] f32: K+1 logits, 4K deltas (class-major), log-variance, padding
    props: np.ndarray                   # [N, P, 4] f32
    pcnt: np.ndarray                    # [N] i32 prop_counts
    image_hw: np.ndarray                # [N, 2] i32
    out_hw: np.ndarray                  # [N, 2] i32
    K: int
    thr: float
    cand_max: int
    max_det: int
    keep_mode: str                      # "nms": batched NMS at 0.5;  "order": NMS bypassed, keep = candidate ids by score, descending
    keep_counts: Optional[np.ndarray]   # "order" only: the keep_counts finalize is handed ([N] i32; None = every candidate)
    fix_vars: tuple                     # the settings the case runs under
    exact_boxes: bool                   # candidate boxes are exact in float32: boxes compared bit for bit
    logvar_step: float
    oracle: dict                        # fix_vars -> oracle/detector.py has an answer (no cap, Q3 in range)
    claims: dict


def seed_of(*key):
    s = 0
    for c in repr(key):
        s = (s * 131 + ord(c)) % (2 ** 31 - 1)
    return s


# ------------------------------------------------------------------------------------------------ the restatement
def softmax64(logits):
    """[R, K+1] float32 -> float64, the kernel's formula: the maximum skips NaN like fmaxf, so a NaN, a +inf or a row of -inf
    gives a non-finite row."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(l - np.fmax.reduce(l, axis=1, keepdims=True))
        return e / e.sum(1, keepdims=True)


def finite32(x):
    with np.errstate(all="ignore"):
        return np.isfinite(np.asarray(x, dtype=np.float64).astype(np.float32))


def decode64(deltas, props, clamp=SCALE_CLAMP):
    """deltas [R, K, 4], props [R, 4] float32 -> boxes [R, K, 4] float64 and [R, K] "finite in float32" (centre, extent and corners:
    a product that leaves float32 is inf there and the corners inf or NaN)."""
    d = np.asarray(deltas, dtype=np.float32).astype(np.float64)
    p = np.asarray(props, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        wd, ht = (p[:, 2] - p[:, 0])[:, None], (p[:, 3] - p[:, 1])[:, None]
        cx, cy = p[:, 0:1] + 0.5 * wd, p[:, 1:2] + 0.5 * ht
        dx, dy, dw, dh = d[..., 0] / REG_W[0], d[..., 1] / REG_W[1], d[..., 2] / REG_W[2], d[..., 3] / REG_W[3]
        dw, dh = np.where(dw > clamp, clamp, dw), np.where(dh > clamp, clamp, dh)         # NaN stays NaN (clamp_max_nan)
        pcx, pcy, pw, ph = dx * wd + cx, dy * ht + cy, np.exp(dw) * wd, np.exp(dh) * ht
        box = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)
    fin = finite32(pcx) & finite32(pcy) & finite32(pw) & finite32(ph) & finite32(box).all(-1)
    return box, fin


def clip64(b, hw):
    b = np.array(b, dtype=np.float64).reshape(-1, 4)
    b[:, 0::2] = np.clip(b[:, 0::2], 0.0, float(hw[1]))
    b[:, 1::2] = np.clip(b[:, 1::2], 0.0, float(hw[0]))
    return b


def live_rows(case, n):
    return min(int(case.pcnt[n]), case.head.shape[1])


def candidates(case, n, rule=RIGHT):
    """Stage 1 for image n.  probs [R, K+1], valid [R], frow_of [R], and the candidate list in kernel order (row ascending, then
    class ascending) before the cap: boxes [C, 4] clipped to image_hw, scores, classes, frow, orow; total = C; sel = the ids of
    that list which the cap keeps (the first cand_max)."""
    K, R = case.K, live_rows(case, n)
    head = case.head[n, :R]
    probs = softmax64(head[:, :K + 1])
    box, bfin = decode64(head[:, K + 1:5 * K + 1].reshape(R, K, 4), case.props[n, :R])
    valid = finite32(probs).all(1) & (bfin.all(1) | (rule == ROW_DROP_PER_CLASS))
    frow_of = np.cumsum(valid) - valid
    thr = float(np.float32(case.thr))
    with np.errstate(invalid="ignore"):
        passes = (probs[:, :K] >= thr) if rule == THRESH_GE else (probs[:, :K] > thr)
    passes = passes & valid[:, None] & (bfin | (rule != ROW_DROP_PER_CLASS))
    rows, cls = np.nonzero(passes)
    total = len(rows)
    first = max(0, total - case.cand_max) if rule == CAP_LAST else 0
    return dict(probs=probs, valid=valid, frow_of=frow_of, boxes=clip64(box[rows, cls], case.image_hw[n]), scores=probs[rows, cls],
                classes=cls.astype(np.int64), frow=frow_of[rows].astype(np.int64), orow=rows.astype(np.int64), total=total,
                sel=np.arange(first, min(total, first + case.cand_max)))


def capped(cand):
    """The candidate arrays as the kernel leaves them: list position = candidate id c."""
    return {k: cand[k][cand["sel"]] for k in ("boxes", "scores", "classes", "frow", "orow")}


def keep_of(case, n, cand):
    """The candidate ids finalize is handed for image n, and the keep_counts that go with them."""
    c = capped(cand)
    if case.keep_mode == "nms":
        with np.errstate(all="ignore"):
            keep = O.batched_nms_f32(c["boxes"].astype(np.float32), c["scores"].astype(np.float32), c["classes"], 0.5,
                                     device_type="cuda")[:case.max_det]
        return np.asarray(keep, dtype=np.int64), len(keep)
    kc = len(c["scores"]) if case.keep_counts is None else int(case.keep_counts[n])
    keep = O.order_desc_stable(c["scores"].astype(np.float32))[:min(kc, case.max_det)]
    assert len(keep) == min(kc, case.max_det), "keep_counts beyond the candidates"
    return np.asarray(keep, dtype=np.int64), kc


def finalize(case, n, cand, keep, fix_vars, rule=RIGHT):
    """Stage 2 for image n, in the kernel's rounds of 64 keep entries: rescale by float32(ow / iw), float32(oh / ih), clip to
    out_hw, drop w <= 0 or h <= 0, compact.  Logits through frow (Q4), probs through orow, the variance through the candidate id
    (Q3, clamped to per_image - 1) or through orow when fix_vars."""
    K, P = case.K, case.head.shape[1]
    c = capped(cand)
    (ih, iw), (oh, ow) = case.image_hw[n].tolist(), case.out_hw[n].tolist()
    sx, sy = float(np.float32(ow / iw)), float(np.float32(oh / ih))
    keep = np.asarray(keep, dtype=np.int64)[:case.max_det]
    slots, written = {}, 0
    for base in range(0, len(keep), 64):
        written = 0 if rule == NO_CARRY else written
        for cid in keep[base:base + 64]:
            b = c["boxes"][cid] * np.array([sx, sy, sx, sy])
            b = b if rule == CLIP_BEFORE_SCALE_ONLY else clip64(b, (oh, ow))[0]
            b32 = b.astype(np.float32)
            if not (b32[2] - b32[0] > 0 and b32[3] - b32[1] > 0) and rule != KEEP_EMPTY:
                continue
            frow, orow = int(c["frow"][cid]), int(c["orow"][cid])
            vrow = orow if (fix_vars and rule != VARS_IGNORE_FIX) else min(int(cid), P - 1)
            vrow = frow if rule == VARS_BY_FROW else vrow
            slots[written] = dict(
                boxes=b, scores=c["scores"][cid], classes=int(c["classes"][cid]), rows=orow, frow=frow, cid=int(cid), vrow=vrow,
                logits=case.head[n, orow if rule == LOGITS_BY_OROW else frow, :K + 1],
                probs=cand["probs"][frow if rule == PROBS_BY_FROW else orow, :K],
                vars=np.exp(np.float64(case.head[n, vrow, 5 * K + 1])))
            written += 1
    recs = [slots[i] for i in range(written)]
    shape = dict(boxes=(0, 4), logits=(0, K + 1), probs=(0, K))
    dt = dict(classes=np.int64, rows=np.int64, frow=np.int64, cid=np.int64, vrow=np.int64, logits=np.float32)
    return {k: (np.stack([r[k] for r in recs]).astype(dt.get(k, np.float64)) if recs else np.zeros(shape.get(k, (0,)), dt.get(k, np.float64)))
            for k in ("boxes", "scores", "classes", "rows", "frow", "cid", "vrow", "logits", "probs", "vars")} | {"count": written}


def run(case, fix_vars, rule=RIGHT):
    """Per image: (candidates, keep, keep_count, detections)."""
    out = []
    for n in range(len(case.pcnt)):
        cand = candidates(case, n, rule)
        keep, kc = keep_of(case, n, cand)
        out.append((cand, keep, kc, finalize(case, n, cand, keep, fix_vars, rule)))
    return out


def var_row(case, variances):
    """The row a variance names: log(var) / logvar_step, rounded."""
    with np.errstate(all="ignore"):
        return np.rint(np.log(np.asarray(variances, dtype=np.float64)) / case.logvar_step).astype(np.int64)


EXACT_FIELDS = ("total", "cand_classes", "cand_frow", "cand_orow", "count", "classes", "rows", "frow", "logits", "vrow")


def exact_view(case, fix_vars, rule=RIGHT):
    """What the GPU test compares exactly, as one comparable tuple per image (boxes too where the case has exact boxes)."""
    out = []
    for cand, keep, kc, det in run(case, fix_vars, rule):
        c = capped(cand)
        v = dict(total=cand["total"], cand_classes=c["classes"].tolist(), cand_frow=c["frow"].tolist(), cand_orow=c["orow"].tolist(),
                 count=det["count"], classes=det["classes"].tolist(), rows=det["rows"].tolist(), frow=det["frow"].tolist(),
                 logits=det["logits"].view(np.uint32).tolist(), vrow=det["vrow"].tolist())
        if case.exact_boxes:
            v["cand_boxes"] = c["boxes"].astype(np.float32).tolist()
            v["boxes"] = det["boxes"].astype(np.float32).tolist()
        out.append(v)
    return out


# ------------------------------------------------------------------------------------------------ builders: pieces
def grid(x):
    return np.round(np.asarray(x, dtype=np.float64) * 4096.0) / 4096.0


def draw_logits(rng, K, multi):
    """One row on the 2^-12 grid: everything in [-2, 0), then either the background or one foreground class lifted so that it
    holds most of the mass; multi: up to two more foreground classes lifted to a sizeable share."""
    l = grid(rng.uniform(-2.0, 0.0, K + 1))
    lift = grid(rng.uniform(1.0, 4.0) + np.log(K + 1.0))
    if rng.random() < 0.7:
        t = int(rng.integers(0, K))
        l[t] += lift
        if multi:
            for u in rng.permutation(K)[:2]:
                if u != t and rng.random() < 0.7:
                    l[u] += grid(lift - rng.uniform(0.2, 1.5))
    else:
        l[K] += lift
    return l


def exact_props(rng, P, hw, pitch=None):
    """Integer corners, extents 8..64 (powers of two), inside the image.  pitch: one box per cell of a pitch x pitch grid, so
    that nothing overlaps."""
    ih, iw = hw
    ext = 2 ** rng.integers(3, 7, (P, 2))
    if pitch is None:
        x1, y1 = rng.integers(8, iw - 72, P), rng.integers(8, ih - 72, P)
    else:
        cols = (iw - 16) // pitch
        assert cols * ((ih - 16) // pitch) >= P
        ext = np.minimum(ext, pitch // 2)
        x1, y1 = 8 + (np.arange(P) % cols) * pitch + pitch // 4, 8 + (np.arange(P) // cols) * pitch + pitch // 4
    return np.stack([x1, y1, x1 + ext[:, 0], y1 + ext[:, 1]], 1).astype(np.float32)


def exact_deltas(rng, P, K, amp=8):
    d = np.zeros((P, K, 4), dtype=np.float32)
    d[..., :2] = (10.0 * rng.integers(-amp, amp + 1, (P, K, 2)) / 8.0).astype(np.float32)
    return d


def new_head(N, P, K, stride, step):
    head = np.zeros((N, P, stride), dtype=np.float32)
    head[..., 5 * K + 1] = (np.arange(P) * step).astype(np.float32)
    return head


def settle_scores(rng, head, pcnt, K, thr, multi):
    """Redraw rows until every foreground probability of a live row is MARGIN away from thr and the candidate scores of one image
    are GAP apart."""
    thr = float(np.float32(thr))
    for n in range(head.shape[0]):
        R = min(int(pcnt[n]), head.shape[1])
        for _ in range(200):
            with np.errstate(all="ignore"):
                p = softmax64(head[n, :R, :K + 1])[:, :K]
                p = np.where(np.isfinite(p), p, -1.0)
            bad = set(np.nonzero((np.abs(p - thr) < MARGIN).any(1))[0].tolist())
            rows, cls = np.nonzero(p > thr)
            s = p[rows, cls]
            o = np.argsort(s)
            close = np.nonzero(np.diff(s[o]) < GAP * s[o][1:])[0]
            bad |= set(rows[o[close]].tolist()) | set(rows[o[close + 1]].tolist())
            if not bad:
                break
            for r in bad:
                head[n, r, :K + 1] = draw_logits(rng, K, multi)
        else:
            raise AssertionError("scores did not settle")


INVALID_KINDS = ("nan_delta", "inf_logit", "ninf_logits")


def plant_invalid(head, n, r, K, kind):
    if kind == "nan_delta":
        head[n, r, K + 1 + 4 * (r % K) + (r % 2)] = NAN           # dx or dy of one class
    elif kind == "inf_logit":
        head[n, r, r % (K + 1)] = INF
    else:
        head[n, r, :K + 1] = -INF


def generic(key, N, P, K, thr, pcnt=None, stride=None, multi=False, image_hw=None, out_shift=1, invalid=(), max_det=100,
            cand_max=None, fix_vars=(0, 1), pitch=None, family=None, **claims):
    """Exact inputs, random logits, NMS.  invalid: (n, r) rows that get one of INVALID_KINDS in turn."""
    rng = np.random.default_rng(seed_of(key))
    stride = 5 * K + 2 if stride is None else stride
    step = 1.0 / 16 if P > 512 else 1.0 / 8
    image_hw = np.asarray(image_hw if image_hw is not None else [(256 + 64 * n, 320 + 32 * n) for n in range(N)], dtype=np.int32)
    out_hw = (image_hw * 2 ** out_shift if out_shift >= 0 else image_hw // 2 ** -out_shift).astype(np.int32)
    pcnt = np.asarray([P] * N if pcnt is None else pcnt, dtype=np.int32)
    head = new_head(N, P, K, stride, step)
    props = np.zeros((N, P, 4), dtype=np.float32)
    for n in range(N):
        props[n] = exact_props(rng, P, image_hw[n], pitch)
        head[n, :, K + 1:5 * K + 1] = exact_deltas(rng, P, K).reshape(P, 4 * K)
        for r in range(P):
            head[n, r, :K + 1] = draw_logits(rng, K, multi)
    settle_scores(rng, head, pcnt, K, thr, multi)
    for j, (n, r) in enumerate(invalid):
        plant_invalid(head, n, r, K, INVALID_KINDS[j % 3])
    cmax = P * K if cand_max is None else cand_max
    return seal(Case(head, props, pcnt, image_hw, out_hw, K, thr, cmax, max_det, "nms", None, tuple(fix_vars), True, step, {},
                     dict(invalid=sorted(invalid), family=family, **claims)))


def seal(case):
    """Fill in Case.oracle: the reference has an answer when the cap does not bite and, without fix_vars, Q3's candidate ids stay
    below the number of live rows."""
    res = run(case, 0)
    uncapped = all(cand["total"] <= case.cand_max for cand, _, _, _ in res)
    q3 = all(len(keep) == 0 or int(keep.max()) < live_rows(case, n) for n, (_, keep, _, _) in enumerate(res))
    return case._replace(oracle={f: bool(uncapped and (f or q3)) for f in case.fix_vars})


# ------------------------------------------------------------------------------------------------ families
SCAN_P = (1, 63, 64, 65, 129, 1024)
SEAM_ROWS = (0, 62, 63, 64, 65)


def build_scan_seam(P):
    """Invalid rows at 0, 62, 63, 64, 65 and P - 1 where they exist (lane 0 and lane 63 of a wave, the first lanes of the next, the
    last thread that has a row); prop_counts from {P, P - 1, 1, 0, P + 7} in turn over the family's images."""
    N = 3
    choices = [P, P - 1, 1, 0, P + 7]
    i0 = SCAN_P.index(P) * N
    pcnt = [choices[(i0 + n) % 5] for n in range(N)]
    rows = sorted({r for r in SEAM_ROWS + (P - 1,) if r < P})
    if P == 1:
        invalid = [(0, 0)]                       # one row: invalid in image 0, absent in image 1, valid in image 2
        pcnt = [1, 0, 8]
    else:
        invalid = [(n, r) for n in range(N) for r in rows[n % 2::2] + ([P - 1] if n == 0 else [])]
    for attempt in range(64):                    # a seed at which every image with a valid live row has a candidate (P = 1: one row)
        case = generic(("scan_seams", P, attempt), N, P, 3, 0.5, pcnt=pcnt, invalid=sorted(set(invalid)),
                       image_hw=[(800, 1000)] * N if P > 129 else None, family="scan_seams", counts_drawn=pcnt)
        if all(c["total"] > 0 or not c["valid"].any() for c in (candidates(case, n) for n in range(N))):
            return case
    raise AssertionError(P)


def build_dead_memory(stride):
    """P = 65, R in {40, 0}: NaN in every head row and proposal row >= R and in the head columns 5K+2 .. stride-1 of every row."""
    case = generic(("dead_memory", stride), 3, 65, 3, 0.5, pcnt=[40, 0, 40], stride=stride, invalid=[(0, 0), (0, 39), (2, 17)],
                   family="dead_memory")
    head, props = case.head.copy(), case.props.copy()
    for n in range(3):
        R = int(case.pcnt[n])
        head[n, R:] = NAN
        props[n, R:] = NAN
    head[..., 5 * 3 + 2:] = NAN
    return seal(case._replace(head=head, props=props))


def build_quirk_indices():
    """P = 64, D = 100: 10 dropped rows among the first 40 of every image."""
    rng = np.random.default_rng(seed_of("quirk rows"))
    invalid = [(n, int(r)) for n in range(3) for r in np.sort(rng.choice(40, 10, replace=False))]
    return generic("quirk_indices", 3, 64, 3, 0.5, invalid=invalid, family="quirk_indices")


TIE_K = (1, 3, 80)


def build_threshold_tie(K):
    """P = 8, thr = 0.5.  Rows 0 and 2: logits [a, -inf .., a] with the foreground a on class 0 / class K-1 and the other a on the
    background: p == 0.5 exactly, must NOT pass.  Rows 1 and 3: the same with a + 2^-12 / a + 3 * 2^-12 on the foreground:
    passes.  Rows 4-7 generic."""
    case = generic(("threshold_tie", K), 2, 8, K, 0.5, pitch=32, family="threshold_tie")
    head = case.head.copy()
    for n in range(2):
        for r, (k, up) in enumerate([(0, 0), (0, 1), (K - 1, 0), (K - 1, 3)]):
            a = -1.0 + (4 * n + r) / 8.0
            head[n, r, :K + 1] = -INF
            head[n, r, K] = a
            head[n, r, k] = a + up / 4096.0
    case = case._replace(head=head, claims=dict(case.claims, ties=[0, 2], passes=[1, 3], tie_values=(0.5,)))
    check_scores(case, margin=5e-5)                  # sigmoid(2^-12) - 0.5 = 6.1e-5: 10^3 float32 spacings above the threshold
    return seal(case)


def build_multi_class(thr, over):
    """P = 16, K = 3.  over False: 3 rows pass all classes and 2 rows two of them (one of those with a class at a small p > 0: it
    passes at thr = 0 only), the other rows have every foreground logit at -inf (p == 0, passes at neither threshold): 12 or 13
    candidates, so Q3 stays in range.  over True: every row passes in several classes, the list is longer than R and only
    fix_vars = 1 has a reference answer."""
    N, P, K = 2, 16, 3
    rng = np.random.default_rng(seed_of("multi_class", over))
    case = generic(("multi_class", thr, over), N, P, K, 0.5, family="multi_class", fix_vars=(1,) if over else (0, 1))
    head = case.head.copy()
    for n in range(N):
        order = rng.permutation(P)
        for j, r in enumerate(order):
            l = np.full(K + 1, -INF)
            l[K] = 0.0
            if over or j < 5:
                full = over or j < 3
                l[:K] = grid(rng.permutation(K) * 0.5 + rng.uniform(0.0, 0.25, K) + 0.25 * j / P)
                if not full:
                    l[(j + n) % K] = -INF if j == 3 else grid(-3.5 + 0.125 * n)       # p == 0, or 0 < p < 0.05
            head[n, r, :K + 1] = l
    case = case._replace(head=head, thr=thr, claims=dict(case.claims, tie_values=(0.0,)))
    check_scores(case)
    return seal(case)


def check_scores(case, margin=MARGIN):
    """The builders that write logits by hand: the same conditions settle_scores establishes (claims["tie_values"]: the planted
    probabilities that sit exactly on the threshold)."""
    thr = float(np.float32(case.thr))
    for n in range(len(case.pcnt)):
        p = softmax64(case.head[n, :live_rows(case, n), :case.K + 1])[:, :case.K]
        p = p[np.isfinite(p)]
        tie = set(case.claims.get("tie_values", ()))
        assert all(abs(x - thr) >= margin or x in tie for x in p.tolist()), "a probability too close to the threshold"
        s = np.sort(p[p > thr])
        assert (np.diff(s) >= GAP * s[1:]).all(), "two scores too close"


def build_q3_overrange():
    """P = 8, R = 4 (and 5), K = 3, thr = 0.05, fix_vars = 0: every live row passes in all three classes, nothing overlaps, so the
    kept candidate ids run up to 3R - 1: past R, where THE REFERENCE HAS NO ANSWER (variance[keep] raises IndexError), and past
    P - 1.  The kernel reads the log-variance of row min(c, per_image - 1), a documented clamp that is pinned here against the
    restatement only.  Rows R .. P-1 are dead rows with finite log-variances r / 8."""
    N, P, K = 2, 8, 3
    rng = np.random.default_rng(seed_of("q3_overrange"))
    case = generic("q3_overrange", N, P, K, 0.5, pcnt=[4, 5], pitch=32, family="q3_overrange", fix_vars=(0,))
    head = case.head.copy()
    head[..., K + 1:5 * K + 1] = 0                       # zero deltas: the boxes are the disjoint proposals, every class survives NMS
    for n in range(N):
        for r in range(P):
            head[n, r, :K] = grid(rng.permutation(K) * 0.5 + rng.uniform(0.0, 0.25, K) + 0.25 * r / P)
            head[n, r, K] = 0.0
    case = case._replace(head=head, thr=0.05)
    check_scores(case)
    return seal(case)


CAP_MAX = (1, 3, 63, 64, 65)


def build_cap(cand_max):
    """P = 64, K = 3, thr = 0.05 with several classes per row: more than 65 candidates per image, cand_max below that."""
    case = generic("cap", 3, 64, 3, 0.05, multi=True, cand_max=cand_max, invalid=[(0, 3), (1, 0), (2, 20)], family="cap")
    assert all(candidates(case, n)["total"] > max(CAP_MAX) for n in range(3))
    return case


def ranked(key, N, P, K, max_det, empties, keep_counts=None, family=None, image_hw=None, out_shift=1):
    """NMS bypassed.  Every row passes in exactly one class (row % K) and the row at place j of a random permutation has the
    j-th best score (top logit 1.25 + (P - 1 - j) / 16, the other three at 0: p from 1 - 3e-4 down to 0.54), so keep position j
    is that row's candidate and keep is a non-monotonic permutation.  empties: per image {keep position: kind}; kind "out_hi" /
    "out_lo" (a proposal wholly right of / above the image: the clip collapses it) or "dw" / "dh" (delta -inf: exp gives a
    zero extent; the row stays valid)."""
    rng = np.random.default_rng(seed_of(key))
    step = 1.0 / 8
    image_hw = np.asarray(image_hw if image_hw is not None else [(512, 640)] * N, dtype=np.int32)
    out_hw = (image_hw * 2 ** out_shift).astype(np.int32)
    head = new_head(N, P, K, 5 * K + 2, step)
    props = np.zeros((N, P, 4), dtype=np.float32)
    place = np.zeros((N, P), dtype=np.int64)
    for n in range(N):
        ih, iw = image_hw[n].tolist()
        props[n] = exact_props(rng, P, (ih, iw))
        head[n, :, K + 1:5 * K + 1] = exact_deltas(rng, P, K, amp=2).reshape(P, 4 * K)
        perm = rng.permutation(P)
        place[n] = perm
        for j, r in enumerate(perm):
            k = int(r) % K
            head[n, r, :K + 1] = 0.0
            head[n, r, k] = 1.25 + (P - 1 - j) / 16.0
            kind = empties[n].get(j)
            if kind == "out_hi":
                props[n, r] = [iw + 16, 32, iw + 48, 64]
            elif kind == "out_lo":
                props[n, r] = [32, -48, 64, -16]
            elif kind in ("dw", "dh"):
                head[n, r, K + 1 + 4 * k + (2 if kind == "dw" else 3)] = -INF
            else:
                assert kind is None
    case = Case(head, props, np.full(N, P, dtype=np.int32), image_hw, out_hw, K, 0.5, P * K, max_det, "order",
                None if keep_counts is None else np.asarray(keep_counts, dtype=np.int32), (0, 1), True, step, {},
                dict(family=family, empties=empties, place=place, invalid=[]))
    check_scores(case)
    return seal(case)


EMPTY_D = (64, 65, 130)
EMPTY_KINDS = ("out_hi", "dw", "out_lo", "dh")


def build_empty_after_clip(D):
    """P = 130.  Image 0: empty boxes at keep positions 0, 63, the whole round 64..127, and 128.  Image 1: every box empty.
    Image 2: empty at 0, 63, 64, 127, 128 only."""
    P = 130
    e0 = {j: EMPTY_KINDS[j % 4] for j in [0, 63, 128] + list(range(64, 128))}
    e1 = {j: EMPTY_KINDS[j % 4] for j in range(P)}
    e2 = {j: EMPTY_KINDS[(j + 1) % 4] for j in (0, 63, 64, 127, 128)}
    return ranked(("empty_after_clip", D), 3, P, 3, D, [e0, e1, e2], family="empty_after_clip")


KEEP_D = 70


def build_keep_seams(which):
    """pe_boxhead_finalize with keep_counts of 0, 1, 64 / 65, max_det, max_det + 5 (80 candidates, max_det = 70)."""
    kc = {"low": [0, 1, 64], "high": [65, KEEP_D, KEEP_D + 5]}[which]
    return ranked(("keep_seams", which), 3, 80, 3, KEEP_D, [{2: "dw"}, {0: "out_hi"}, {63: "dh", 64: "out_lo"}], keep_counts=kc,
                  family="keep_seams")


def clamp_deltas():
    """The float32 deltas d with fl(d / 5) just below, exactly at and above SCALE_CLAMP."""
    c = np.float32(SCALE_CLAMP)
    at = np.float32(c * np.float32(5))
    for _ in range(8):
        q = np.float32(at / np.float32(5))
        if q == c:
            break
        at = np.nextafter(at, np.float32(INF if q < c else -INF), dtype=np.float32)
    assert np.float32(at / np.float32(5)) == c
    below = np.float32(at * np.float32(1 - 1e-3))
    return below, at, np.float32(at * np.float32(1.5))


DECODE_ROWS = ("below", "at", "above", "pinf", "dw_ninf", "dh_ninf", "dx_big", "dx_nbig", "on_edge", "past_edge", "negative")


def build_decode_edges():
    """P = 16, K = 3, NMS bypassed.  Rows 0-10 are DECODE_ROWS, rows 11-15 have random non-dyadic deltas.  dw just below, at and
    above the clamp and +inf (valid, clamped: the box of "above"); dw / dh = -inf (valid, zero extent: a candidate, dropped as
    empty by finalize); dx = +-1e38 on a 64 wide proposal and on a class that does NOT pass (the product leaves float32: the whole
    row goes); a proposal whose box lands on x2 == iw, y1 == 0; one with x1 == iw (empty after the clip); negative corners."""
    N, P, K = 2, 16, 3
    case = ranked("decode_edges", N, P, K, 100, [{}, {}], family="decode_edges", image_hw=[(256, 320), (384, 512)])
    head, props = case.head.copy(), case.props.copy()
    rng = np.random.default_rng(seed_of("decode_edges deltas"))
    below, at, above = clamp_deltas()
    rows = {}
    for n in range(N):
        ih, iw = case.image_hw[n].tolist()
        for r, name in enumerate(DECODE_ROWS):
            k, other = r % K, (r + 1) % K
            head[n, r, K + 1:5 * K + 1] = 0
            props[n, r] = [64 + 8 * r, 64, 80 + 8 * r, 96]
            col = K + 1 + 4 * k
            if name in ("below", "at", "above", "pinf"):
                head[n, r, col + 2 + (r + n) % 2] = dict(below=below, at=at, above=above, pinf=INF)[name]
            elif name == "dw_ninf":
                head[n, r, col + 2] = -INF
            elif name == "dh_ninf":
                head[n, r, col + 3] = -INF
            elif name in ("dx_big", "dx_nbig"):
                props[n, r] = [64, 64, 128, 96]
                head[n, r, K + 1 + 4 * other] = 1e38 if name == "dx_big" else -1e38
            elif name == "on_edge":
                props[n, r] = [iw - 16, 0, iw, 16]
            elif name == "past_edge":
                props[n, r] = [iw, 0, iw + 16, 16]
            else:
                props[n, r] = [-8, -8, 8, 8]
            rows[name] = r
        head[n, len(DECODE_ROWS):, K + 1:5 * K + 1] = rng.normal(0.0, 1.0, (P - len(DECODE_ROWS), 4 * K)).astype(np.float32)
    invalid = sorted((n, rows[k]) for n in range(N) for k in ("dx_big", "dx_nbig"))
    return seal(case._replace(head=head, props=props, exact_boxes=False,
                              claims=dict(case.claims, rows=rows, clamp_deltas=(below, at, above), invalid=invalid)))


def overshoot(size, lo):
    """The first output size >= lo at which float32(out / size) * size rounds ABOVE out in float32: a coordinate clipped to the
    image edge lands past the output edge and only the second clip brings it back."""
    for out in range(lo, lo + 4000):
        if np.float32(np.float32(out / size) * np.float32(size)) > np.float32(out):
            return out
    raise AssertionError(size)


def build_scale_edges():
    """P = 8, NMS, sizes differ per image: out_hw smaller (492 x 614 from 768 x 960, non-dyadic), equal, and larger by a
    non-dyadic factor chosen by overshoot().  Candidate boxes are exact integers, so the final boxes are compared bit for bit.
    Rows 0 and 1 of every image reach past the right / bottom edge and are clipped to it."""
    image_hw = [(768, 960), (256, 320), (800, 1000)]
    case = generic("scale_edges", 3, 8, 3, 0.5, image_hw=image_hw, pitch=64, family="scale_edges")
    props, head, out_hw = case.props.copy(), case.head.copy(), case.out_hw.copy()
    out_hw[0], out_hw[1], out_hw[2] = (492, 614), (256, 320), (overshoot(800, 1100), overshoot(1000, 1300))
    for n, (ih, iw) in enumerate(image_hw):
        props[n, 0] = [iw - 32, 16, iw + 32, 48]
        props[n, 1] = [16, ih - 32, 48, ih + 32]
        for r in (0, 1):
            head[n, r, :] = 0
            head[n, r, 5 * 3 + 1] = r / 8.0
            head[n, r, r] = 4.0 + r / 4.0 + n / 16.0               # passes in class r, deltas zero
    case = case._replace(props=props, head=head, out_hw=out_hw)
    check_scores(case)
    return seal(case)


SWEEP_K = (1, 2, 3, 80)


def build_k_sweep(K):
    """P = 8, head_stride = 5K + 2 exactly, one invalid row."""
    return generic(("k_sweep", K), 2, 8, K, 0.5, invalid=[(0, 2), (1, 0)], family="k_sweep")


# ------------------------------------------------------------------------------------------------ registry
FAMILIES = {
    "scan_seams": {f"scan_P{P}": functools.partial(build_scan_seam, P) for P in SCAN_P},
    "dead_memory": {f"dead_memory_stride{s}": functools.partial(build_dead_memory, s) for s in (24, 19)},
    "quirk_indices": {"quirk_indices": build_quirk_indices},
    "threshold_tie": {f"threshold_tie_K{K}": functools.partial(build_threshold_tie, K) for K in TIE_K},
    "multi_class": {"multi_class_thr0.05": functools.partial(build_multi_class, 0.05, False),
                    "multi_class_thr0": functools.partial(build_multi_class, 0.0, False),
                    "multi_class_over": functools.partial(build_multi_class, 0.05, True)},
    "q3_overrange": {"q3_overrange": build_q3_overrange},
    "cap": {f"cap_{c}": functools.partial(build_cap, c) for c in CAP_MAX},
    "empty_after_clip": {f"empty_after_clip_D{D}": functools.partial(build_empty_after_clip, D) for D in EMPTY_D},
    "keep_seams": {f"keep_seams_{w}": functools.partial(build_keep_seams, w) for w in ("low", "high")},
    "decode_edges": {"decode_edges": build_decode_edges},
    "scale_edges": {"scale_edges": build_scale_edges},
    "k_sweep": {f"k_sweep_K{K}": functools.partial(build_k_sweep, K) for K in SWEEP_K},
}
BUILDERS = {name: fn for fam in FAMILIES.values() for name, fn in fam.items()}
FAMILY_OF = {name: f for f, fam in FAMILIES.items() for name in fam}


def names(*families):
    return [name for f in (families or FAMILIES) for name in FAMILIES[f]]


@functools.lru_cache(maxsize=None)
def get(name):
    case = BUILDERS[name]()
    for a in (case.head, case.props, case.pcnt, case.image_hw, case.out_hw, case.keep_counts):
        if a is not None:
            a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def want(name, fix_vars):
    """The restatement under the right rule, computed once and shared."""
    return tuple(run(get(name), fix_vars))
