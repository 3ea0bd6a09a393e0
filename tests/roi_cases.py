"""Shared code of tests/test_roi_align_edges_gpu.py (asserts on csrc/roi_align.hip) and tests/test_roi_align_edges_cpu.py (asserts
on this file and on oracle/roi_align.py): case builders for the places where a ROIAlign goes wrong without a random test noticing -
samples on the validity edge, the last-row clamp, the divisor, the adaptive grid at an integer bin size, the table-size seam of the
fp16 kernels, degenerate boxes, rows that take no part, and the FPN level rule at its seams.  Numpy (and the oracle), no GPU.

A case is the argument list of layers.roi_align_nhwc in its boxes form plus what it claims:
    Case(name, hw [(H, W)] per level, scales, N, boxes [N, P, 4] f32, counts [N] i32 | None, pooled, ratio, aligned,
         exact [N*P] bool, zero [N*P] bool, tags {tag: [row, ...]})
rois5(case) is the same work as [R, 5] rows with unordered batch indices (live rows only).  features(case, C) are the maps,
oracle(case, feats) is the expectation ([R, ph, pw, C] float32, zeros on dead and negative-size rows, and the level per row, -1 on
dead rows), and ref64(case, feats, rule) restates the rule in float64 with switches for deliberately WRONG rules (Rule): a family
earns its place only if a wrong rule that bears on it changes an output bit (tests/test_roi_align_edges_cpu.py).

Exactness of the exact family.  Features are integers in [-8, 8].  Scales are powers of two and box corners are chosen so that in
feature space the start lies on a 1/8-pixel grid and every bin size is an integer b (adaptive grid b: samples on half-integers of
that grid) or one of 0.25, 0.5, 0.75, 1.5, 3.5; the fixed ratio is 0, 2 or 4.  Every sample coordinate is then a dyadic rational
with at most 5 fraction bits, every bilinear weight has at most 5, a product of two at most 10, a bin's sum stays below 2^10 * 21^2
in units of 2^-10: all exact in float32 in ANY order of summation, with or without fused multiply-adds, as taps or as separable
table sums.  Only the division by the sample count and the fp16 store round, both correctly: the tap form, both table forms, the
oracle and a float64 restatement rounded once must agree bit for bit.  Rows with `exact` False (bin size 2.125, grid 3: the sample
offsets (i + .5) * 2.125 / 3 round) are there for the grid rule; the fp32 kernel follows the reference's order of operations and
must still match it in every bit, the fp16 forms are held to the derived bound of the random family on them.
The min-size clamp of unaligned mode makes bins of 1 / pooled: those cases keep to pooled sizes 2, 4 and 8."""
import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import detector as OD
from oracle import roi_align as RA

F32 = np.float32
FPN_SCALES = [1 / 4, 1 / 8, 1 / 16, 1 / 32]
POOLED = [(7, 7), (8, 8), (3, 5), (7, 3), (1, 1), (2, 4), (9, 7), (14, 14)]
FRACTION_BINS = [0.25, 0.5, 0.75, 1.5, 3.5]
GRID_COUNT_BINS = [(1, 3), (1, 5), (2, 3), (1, 7), (3, 3), (3, 5), (3, 7)]     # sample counts 3, 5, 6, 7, 9, 15, 21


class Case(NamedTuple):
    name: str
    hw: list
    scales: list
    N: int
    boxes: np.ndarray
    counts: Optional[np.ndarray]
    pooled: tuple
    ratio: int
    aligned: bool
    exact: np.ndarray
    zero: np.ndarray
    tags: dict
    random: bool = False


class Rule(NamedTuple):
    """The reference's rule is Rule(); every switch is one way of getting it wrong."""
    edge_exclusive: bool = False      # samples at exactly -1 and exactly H / W dropped
    count_valid: bool = False         # divisor = number of samples inside the validity window
    grid_floor1: bool = False         # adaptive grid = floor(bin size) + 1 instead of ceil
    no_last_clamp: bool = False       # no clamp at the last row / column: the pixel beyond reads as zero
    no_half: bool = False             # aligned mode without its half-pixel offset
    clamp_aligned: bool = False       # the min-size clamp of unaligned mode applied in aligned mode too
    level64: bool = False             # FPN level from float64 arithmetic


WRONG_RULES = {f: Rule(**{f: True}) for f in Rule._fields}


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def seed_of(*key):
    s = 0
    for c in repr(key):
        s = (s * 131 + ord(c)) % (2 ** 31 - 1)
    return s


def live_mask(case):
    P = case.boxes.shape[1]
    cnt = np.full(case.N, P) if case.counts is None else case.counts
    return (np.arange(P)[None, :] < np.asarray(cnt)[:, None]).reshape(-1)


def rois5(case, shuffle=True):
    """The live rows as [R, 5] (batch index first), shuffled so that batch indices come unordered; returns (rois, row ids)."""
    rows = np.nonzero(live_mask(case))[0]
    if shuffle:
        rows = np.random.default_rng(seed_of(case.name, "rois5")).permutation(rows)
    P = case.boxes.shape[1]
    r = np.concatenate([(rows // P).astype(F32)[:, None], case.boxes.reshape(-1, 4)[rows]], axis=1)
    return np.ascontiguousarray(r, dtype=F32), rows


@functools.lru_cache(maxsize=None)
def _features(hw, N, C, random, seed):
    rng = np.random.default_rng(seed)
    if random:
        return tuple(rng.standard_normal((N, h, w, C)).astype(F32) for h, w in hw)
    return tuple(rng.integers(-8, 9, (N, h, w, C)).astype(F32) for h, w in hw)


def features(case, C=256):
    """NHWC float32 maps per level: integers in [-8, 8] (exact in fp16) or N(0, 1) for the random family.  A narrower C is a
    channel slice of the 256-channel maps, so one oracle run serves every channel count."""
    full = _features(tuple(case.hw), case.N, 256, case.random, seed_of(tuple(case.hw), case.N, case.random))
    return [np.ascontiguousarray(f[..., :C]) for f in full]


# ------------------------------------------------------------------------------------------------ levels
def oracle_levels(boxes):
    """oracle.detector.assign_levels on [R, 4] float32 boxes."""
    return OD.assign_levels(torch.from_numpy(np.ascontiguousarray(boxes, dtype=F32))).numpy().astype(np.int32)


def levels_restated(boxes, nudge=0, f64=False):
    """The level rule of poolers.py:13-44 restated step by step: float32 as the oracle evaluates it (with its log2 result moved
    by `nudge` float32 ulps), or float64 arithmetic on the same float32 corners."""
    b = torch.from_numpy(np.ascontiguousarray(boxes, dtype=F32))
    if f64:
        b = b.double()
    eps = float(np.finfo(np.float64).eps)
    lg = torch.log2(torch.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])) / 224 + eps)
    for _ in range(abs(nudge)):
        lg = torch.nextafter(lg, torch.full_like(lg, float("inf") if nudge > 0 else float("-inf")))
    return (torch.clamp(torch.floor(4 + lg), min=2, max=5).to(torch.int64) - 2).numpy().astype(np.int32)


def case_levels(case, rule=Rule()):
    flat = case.boxes.reshape(-1, 4)
    if len(case.scales) == 1:
        lv = np.zeros(len(flat), np.int32)
    else:
        lv = levels_restated(flat, f64=True) if rule.level64 else oracle_levels(flat)
        lv = np.where(case.zero, 0, lv)      # negative-size rows: zeros at any level (a negative area has no level)
    return np.where(live_mask(case), lv, -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ expectations
def oracle(case, feats):
    """The oracle's float32 result in the kernel's layout [R, ph, pw, C] and the level per row (-1: dead).  Dead rows and - in
    aligned mode - rows of negative size (the oracle refuses them, the kernel writes zeros) are zeros and kept out of the call."""
    lv = case_levels(case)
    flat = case.boxes.reshape(-1, 4)
    P = case.boxes.shape[1]
    C = feats[0].shape[3]
    out = np.zeros((len(flat), case.pooled[0], case.pooled[1], C), F32)
    for l, sc in enumerate(case.scales):
        rows = np.nonzero((lv == l) & ~case.zero)[0]
        if not len(rows):
            continue
        r5 = np.concatenate([(rows // P).astype(F32)[:, None], flat[rows]], axis=1)
        o = RA.roi_align_forward(torch.from_numpy(feats[l]).permute(0, 3, 1, 2).contiguous(), torch.from_numpy(r5), sc,
                                 case.pooled[0], case.pooled[1], case.ratio, case.aligned)
        out[rows] = o.permute(0, 2, 3, 1).numpy()
    return out, lv


class Axis(NamedTuple):
    W: np.ndarray        # [bins, size] float64: summed bilinear weights of the bin's valid samples per pixel
    grid: int
    nvalid: np.ndarray   # [bins] samples inside the validity window
    npx: np.ndarray      # [bins] pixels from the first to the last tap (the table's window)


def axis_table(lo_corner, hi_corner, scale, bins, ratio, aligned, size, rule=Rule(), ft=F32):
    """One axis of one ROI by ROIAlign_cpu.cpp:43-96,150-170: coordinates and weights in `ft` arithmetic in the reference's order
    of operations, weights summed per pixel in float64."""
    f = lambda v: np.asarray(v, dtype=ft)
    off = f(0.5 if aligned and not rule.no_half else 0.0)
    start, end = f(lo_corner) * f(scale) - off, f(hi_corner) * f(scale) - off
    roi = end - start
    if not aligned or rule.clamp_aligned:
        roi = np.maximum(roi, f(1.0))
    bs = roi / f(bins)
    if ratio > 0:
        grid = ratio
    else:
        q = float(roi / f(bins))
        grid = int(np.floor(q)) + 1 if rule.grid_floor1 else int(np.ceil(q))
    W = np.zeros((bins, size + 2))
    if grid <= 0:
        return Axis(W[:, :size], grid, np.zeros(bins, np.int64), np.zeros(bins, np.int64))
    p = np.arange(bins, dtype=ft)[:, None]
    i = np.arange(grid, dtype=ft)[None, :]
    y = (start + p * bs) + ((i + f(0.5)) * bs) / f(grid)
    assert y.dtype == ft
    valid = (y > -1) & (y < size) if rule.edge_exclusive else (y >= -1) & (y <= size)
    y = np.where(y <= 0, f(0), y)
    y = np.where(valid, y, f(0))
    lo = y.astype(np.int64)
    if rule.no_last_clamp:
        hi = lo + 1
    else:
        top = lo >= size - 1
        lo = np.where(top, size - 1, lo)
        hi = np.where(top, size - 1, lo + 1)
        y = np.where(top, lo.astype(ft), y)
    l = y - lo.astype(ft)
    h = f(1.0) - l
    rows = np.broadcast_to(np.arange(bins)[:, None], lo.shape)
    np.add.at(W, (rows[valid], lo[valid]), h[valid].astype(np.float64))
    np.add.at(W, (rows[valid], hi[valid]), l[valid].astype(np.float64))
    first = np.where(valid, lo, 1 << 30).min(axis=1)
    last = np.where(valid, hi, -1).max(axis=1)
    return Axis(W[:, :size], grid, valid.sum(axis=1), np.where(last >= 0, last - first + 1, 0))


def roi_axes(case, row, level, rule=Rule(), ft=F32):
    x1, y1, x2, y2 = case.boxes.reshape(-1, 4)[row]
    H, W = case.hw[level]
    sc = case.scales[level]
    return (axis_table(y1, y2, sc, case.pooled[0], case.ratio, case.aligned, H, rule, ft),
            axis_table(x1, x2, sc, case.pooled[1], case.ratio, case.aligned, W, rule, ft))


def ref64(case, feats, rule=Rule(), with_abs=False):
    """Float64 restatement: out [R, ph, pw, C] float64 (not rounded) and levels.  with_abs: also the same sum over |w * f| divided
    by the count, and per bin the table's pixel count plus grid_h + grid_w (what the fp16 bound is made of)."""
    lv = case_levels(case, rule)
    R = lv.shape[0]
    P = case.boxes.shape[1]
    C = feats[0].shape[3]
    out = np.zeros((R, case.pooled[0], case.pooled[1], C))
    A = np.zeros_like(out) if with_abs else None
    terms = np.zeros((R, case.pooled[0], case.pooled[1])) if with_abs else None
    f64 = [f.astype(np.float64) for f in feats]
    for r in np.nonzero(lv >= 0)[0]:
        ay, ax = roi_axes(case, r, lv[r], rule)
        if ay.grid <= 0 or ax.grid <= 0:
            continue
        if rule.count_valid:
            cnt = np.maximum(ay.nvalid[:, None] * ax.nvalid[None, :], 1).astype(np.float64)
        else:
            cnt = np.full((case.pooled[0], case.pooled[1]), float(max(ay.grid * ax.grid, 1)))
        f = f64[lv[r]][r // P]
        H, W = f.shape[:2]
        t = (ay.W @ f.reshape(H, W * C)).reshape(-1, W, C)
        out[r] = np.einsum("qw,pwc->pqc", ax.W, t) / cnt[:, :, None]
        if with_abs:
            t = (ay.W @ np.abs(f).reshape(H, W * C)).reshape(-1, W, C)
            A[r] = np.einsum("qw,pwc->pqc", ax.W, t) / cnt[:, :, None]
            terms[r] = ay.npx[:, None] * ax.npx[None, :] + ay.grid + ax.grid
    return (out, lv, A, terms) if with_abs else (out, lv)


def adjoint64(case, grad, rule=Rule()):
    """Float64 adjoint of ref64: grad [R, ph, pw, C] -> one [N, H, W, C] float64 gradient per level.  Like the reference's
    backward it divides by the raw grid_h * grid_w."""
    lv = case_levels(case, rule)
    P = case.boxes.shape[1]
    C = grad.shape[3]
    gin = [np.zeros((case.N, h, w, C)) for h, w in case.hw]
    for r in np.nonzero(lv >= 0)[0]:
        ay, ax = roi_axes(case, r, lv[r], rule)
        if ay.grid <= 0 or ax.grid <= 0:
            continue
        t = np.einsum("pqc,qw->pwc", grad[r].astype(np.float64), ax.W)
        gin[lv[r]][r // P] += np.einsum("ph,pwc->hwc", ay.W, t) / float(ay.grid * ax.grid)
    return gin


def oracle_backward(case, grad):
    """The oracle's backward per level: grad [R, ph, pw, C] float32 -> [N, H, W, C] float32 per level (live, non-negative rows)."""
    lv = case_levels(case)
    flat = case.boxes.reshape(-1, 4)
    P = case.boxes.shape[1]
    C = grad.shape[3]
    grad = np.asarray(grad, dtype=F32)
    gin = []
    for l, sc in enumerate(case.scales):
        rows = np.nonzero((lv == l) & ~case.zero)[0]
        H, W = case.hw[l]
        r5 = np.concatenate([(rows // P).astype(F32)[:, None], flat[rows]], axis=1)
        g = RA.roi_align_backward(torch.from_numpy(np.ascontiguousarray(grad[rows], dtype=F32)).permute(0, 3, 1, 2), torch.from_numpy(r5),
                                  sc, case.pooled[0], case.pooled[1], case.N, C, H, W, case.ratio, case.aligned)
        gin.append(g.permute(0, 2, 3, 1).contiguous().numpy())
    return gin


def pow2_count_rows(case):
    """(rows that pass gradient on exactly, rows that must pass on nothing).  Exact: live rows whose sample count grid_h * grid_w
    is a power of two - g * w / count is exact there and no order of the atomic adds can show.  Nothing: dead rows and rows
    without samples (a grid <= 0).  The rest (a count of 3, say) rounds: the tests give those rows a zero gradient."""
    lv = case_levels(case)
    ok = np.zeros(lv.shape[0], bool)
    nothing = lv < 0
    for r in np.nonzero(lv >= 0)[0]:
        ay, ax = roi_axes(case, r, lv[r])
        n = ay.grid * ax.grid
        nothing[r] = ay.grid <= 0 or ax.grid <= 0
        ok[r] = not nothing[r] and (n & (n - 1)) == 0
    return ok, nothing


def backward_grad(case, C):
    """Integer grad_output [R, ph, pw, C] in [-8, 8]: nonzero on the exact rows AND on the rows that must pass on nothing."""
    ok, nothing = pow2_count_rows(case)
    rng = np.random.default_rng(seed_of(case.name, "grad", C))
    grad = rng.integers(-8, 9, (len(ok), case.pooled[0], case.pooled[1], C)).astype(F32)
    grad[~(ok | nothing)] = 0
    return grad, ok


# ------------------------------------------------------------------------------------------------ exact family
def box_of(scale, aligned, sx, sy, roi_w, roi_h):
    """Image-space corners of the box whose feature-space start is (sx, sy) and size (roi_w, roi_h) at `scale` (a power of two:
    every step is exact for the dyadic values used here; asserted by the builders through float32 round trips)."""
    off = 0.5 if aligned else 0.0
    x1, y1 = (sx + off) / scale, (sy + off) / scale
    b = np.array([x1, y1, x1 + roi_w / scale, y1 + roi_h / scale])
    assert np.array_equal(b.astype(F32).astype(np.float64), b), b
    return b.astype(F32)


def _pack(name, hw, scales, N, rows, tags, pooled, ratio, aligned, counts=None, P=None, exact=None, zero=None, random=False):
    """rows: list per image of [k, 4] arrays; images are padded to a common P with copies of their first row (or a unit box)."""
    P = P or max(len(r) for r in rows)
    boxes = np.zeros((N, P, 4), F32)
    boxes[:, :, 2:] = 8.0
    for n, r in enumerate(rows):
        if len(r):
            boxes[n, :len(r)] = r
    if counts is None and any(len(r) != P for r in rows):
        counts = np.array([len(r) for r in rows], np.int32)
    R = N * P
    return Case(name, list(hw), list(scales), N, boxes, counts, tuple(pooled), ratio, aligned,
                np.ones(R, bool) if exact is None else exact, np.zeros(R, bool) if zero is None else zero, tags, random)


def hw_of(image_hw, scales):
    return [(int(image_hw[0] * s), int(image_hw[1] * s)) for s in scales]


def _bin_choices(ratio, pow2_only=False):
    if pow2_only:       # adaptive: grids 1, 2, 4, 8; a fixed ratio of 2 or 4 makes every bin size a power-of-two count
        return [1, 2, 4, 8, 0.25, 0.5, 0.75] if ratio == 0 else [1, 2, 3, 5, 7, 9, 12, 0.5, 0.75, 1.5, 3.5]
    return [1, 2, 3, 4, 5, 6, 7] + FRACTION_BINS


def _clamp_safe(b, p, aligned):
    """Unaligned mode clamps a ROI under one pixel to 1: the bin becomes 1 / pooled, exact only for a power of two."""
    return aligned or b * p >= 1 or (p & (p - 1)) == 0


@functools.lru_cache(maxsize=None)
def exact_single(pooled, ratio, aligned, scale=1 / 4, hw=(20, 24), pow2_only=False):
    """One level, N = 2: every named edge on both axes, then random exact boxes reaching 3 px outside the map."""
    H, W = hw
    ph, pw = pooled
    rng = np.random.default_rng(seed_of("exact_single", pooled, ratio, aligned, scale, hw, pow2_only))
    rows, tags = [], {}

    def add(tag, sx, sy, bw, bh, img=0):
        tags.setdefault(tag, []).append((img, len(rows_img[img])))
        rows_img[img].append(box_of(scale, aligned, sx, sy, bw * pw, bh * ph))

    rows_img = [[], []]
    # a bin size whose first sample offset (i = 0) is d: the first sample of bin 0 sits at start + d
    g1 = 1 if ratio == 0 else ratio
    d1 = 0.5 / g1          # bin size 1: offsets (i + .5) / grid
    step = 0.125
    for ax in (0, 1):       # 0: the edge on y, 1: on x; the other axis sits inside the map
        size = H if ax == 0 else W
        other = 2.0

        def put(tag, s):
            sx, sy = (other, s) if ax == 0 else (s, other)
            add(f"{tag}_{'yx'[ax]}", sx, sy, 1, 1)
        put("at_minus_one", -1.0 - d1)                        # first sample exactly -1.0: kept, clamped to 0
        put("below_minus_one", -1.0 - d1 - step)              # one grid step beyond: dropped, still counted
        put("in_minus_one_zero", -0.5 - d1)                   # a sample in (-1, 0]
        # the last sample of the last bin: start + (bins - 1) + (g1 - .5) / g1 = start + bins - d1
        nb = ph if ax == 0 else pw
        put("at_size", size - nb + d1)                        # last sample exactly H / W: kept, clamped to the last row
        put("beyond_size", size - nb + d1 + step)             # one step beyond: dropped, still counted
        put("in_last_pixel", size - nb + d1 - 0.5)            # a sample in [size - 1, size]
    for name, sx, sy in (("outside", W + 6.0, H + 6.0), ("half_left", -0.5 * pw * 2, 3.0), ("half_right", W - 0.5 * pw * 2, 3.0),
                         ("half_top", 3.0, -0.5 * ph * 2), ("half_bottom", 3.0, H - 0.5 * ph * 2), ("corner_tl", -1.5, -1.5),
                         ("corner_tr", W - 1.5 * pw + 0.75, -1.5), ("corner_bl", -1.5, H - 1.5 * ph + 0.75),
                         ("corner_br", W - 1.5 * pw + 0.75, H - 1.5 * ph + 0.75)):    # a bin with one sample inside, one beyond
        add(name, sx, sy, 2 if name.startswith(("half", "outside")) else 1.5, 2 if name.startswith(("half", "outside")) else 1.5)
    if not pow2_only:
        for bh, bw in GRID_COUNT_BINS:
            if ratio == 0:
                add(f"count_{bh * bw}", 1.125, 0.625, bw, bh)
    if _clamp_safe(0, ph, aligned) and _clamp_safe(0, pw, aligned):
        add("zero_area", 5.0, 4.0, 0, 0)
    choices = _bin_choices(ratio, pow2_only)
    for img in (0, 1):
        for _ in range(10):
            bh, bw = rng.choice(choices), rng.choice(choices)
            while not (_clamp_safe(bh, ph, aligned) and _clamp_safe(bw, pw, aligned)):
                bh, bw = rng.choice(choices), rng.choice(choices)
            sx = rng.integers(-8 * 3 - int(8 * bw * pw), 8 * (W + 3) + 1) / 8.0
            sy = rng.integers(-8 * 3 - int(8 * bh * ph), 8 * (H + 3) + 1) / 8.0
            add("random", sx, sy, bw, bh, img)
    rows = [np.stack(r) for r in rows_img]
    n0, n1 = len(rows[0]), len(rows[1])
    P = max(n0, n1) + 3                                       # rows beyond counts on both images
    flat_tags = {t: [i * P + k for i, k in v] for t, v in tags.items()}
    name = f"exact_single{'_pow2' if pow2_only else ''}[{ph}x{pw},ratio{ratio},{'aligned' if aligned else 'legacy'}]"
    return _pack(name, [hw], [scale], 2, rows, flat_tags, pooled, ratio, aligned, counts=np.array([n0, n1], np.int32), P=P)


@functools.lru_cache(maxsize=None)
def exact_grid_seam(aligned=True):
    """Adaptive grid at a seam, per axis independently: bin size exactly 2.0 (grid 2) and 2.125 (grid 3).  Rows with a 2.125
    axis are not exact (module docstring)."""
    pooled, scale, hw = (8, 8), 1 / 4, (24, 28)
    rows, exact, tags = [], [], {}
    for bh in (2.0, 2.125):
        for bw in (2.0, 2.125):
            for sx, sy in ((1.0, 2.0), (-1.5, 3.125), (10.125, 7.0)):
                tags.setdefault(f"bin_{bh}x{bw}", []).append(len(rows))
                rows.append(box_of(scale, aligned, sx, sy, bw * 8, bh * 8))
                exact.append(bh == 2.0 and bw == 2.0)
    return _pack(f"exact_grid_seam[{'aligned' if aligned else 'legacy'}]", [hw], [scale], 1, [np.stack(rows)], tags, pooled, 0, aligned,
                 exact=np.array(exact))


@functools.lru_cache(maxsize=None)
def exact_table_seam():
    """The table-size seam of the fp16 kernels on one 160 x 160 level, N = 1: integer bins of 19 px (a window of 20 pixels: table
    form) and of 20 px (21 pixels: tap fallback inside the table kernels), one ROI where only one axis falls back, one 19-px bin
    that starts on a half-pixel.  The largest boxes of the suite."""
    pooled, scale, hw = (7, 7), 1 / 4, (160, 160)
    spec = [("table_19x19", 2.0, 3.0, 19, 19), ("tap_20x20", 1.0, 2.0, 20, 20), ("one_axis_19x20", 4.0, 2.0, 20, 19),
            ("one_axis_20x19", 2.0, 4.0, 19, 20), ("half_pixel_19", 2.5, 3.5, 19, 19), ("over_the_edge_19", 30.0, 31.0, 19, 19)]
    rows, tags = [], {}
    for tag, sx, sy, bw, bh in spec:
        tags[tag] = [len(rows)]
        rows.append(box_of(scale, True, sx, sy, bw * 7, bh * 7))
    return _pack("exact_table_seam", [hw], [scale], 1, [np.stack(rows)], tags, pooled, 0, True)


@functools.lru_cache(maxsize=None)
def exact_min_size(pooled):
    """Unaligned mode: ROIs under one feature pixel on one axis, the other and both (min-size clamp: bins of 1 / pooled)."""
    assert pooled[0] in (2, 4, 8) and pooled[1] in (2, 4, 8)
    scale, hw = 1 / 8, (12, 14)
    rows, tags = [], {}
    for tag, w, h in (("clamp_both", 0.25, 0.5), ("clamp_w", 0.125, 2.0 * pooled[0]), ("clamp_h", 1.0 * pooled[1], 0.75), ("clamp_zero", 0.0, 0.0)):
        for sx, sy in ((3.0, 4.125), (-1.5, -1.25), (13.5, 11.625), (13.875, 12.0)):
            tags.setdefault(tag, []).append(len(rows))
            rows.append(box_of(scale, False, sx, sy, w, h))
    return _pack(f"exact_min_size[{pooled[0]}x{pooled[1]}]", [hw], [scale], 1, [np.stack(rows)], tags, pooled, 0, False)


@functools.lru_cache(maxsize=None)
def exact_negative(levels=1):
    """Aligned mode: x2 < x1, y2 < y1 and both (grid <= 0: the kernel writes zeros, the oracle refuses the box) among live rows."""
    scales = FPN_SCALES[:levels] if levels == 4 else [1 / 4]
    hw = hw_of((128, 160), scales)
    good = box_of(1 / 4, True, 2.0, 3.0, 14, 28)          # bins of 2 x 4: 8 samples, a power of two for the backward tests
    rows = [good,
            np.array([60.0, 20.0, 30.0, 50.0], F32),      # x2 < x1
            np.array([20.0, 70.0, 50.0, 30.0], F32),      # y2 < y1
            np.array([90.0, 80.0, 20.0, 10.0], F32),      # both: a positive area of a negative-size box
            box_of(1 / 4, True, 5.0, 4.0, 0, 0),          # zero area
            good + F32(8.0)]
    zero = np.array([False, True, True, True, False, False])
    tags = {"x_neg": [1], "y_neg": [2], "both_neg": [3], "zero_area": [4]}
    return _pack(f"exact_negative[{levels}]", hw, scales, 1, [np.stack(rows)], tags, (7, 7), 0, True, zero=zero)


def _level_range(l):
    return (0.0 if l == 0 else 112.0 * 2 ** (l - 1) * 1.0, float("inf") if l == 3 else 112.0 * 2 ** l)


@functools.lru_cache(maxsize=None)
def exact_fpn(pooled, ratio, aligned, pow2_only=False):
    """Four levels of a 256 x 320 image, N = 3 with counts = 0 for image 1: per level six boxes whose bins are exact AT THAT LEVEL
    and whose area puts them there (asserted against the oracle's level rule), reaching outside the map."""
    hw = hw_of((256, 320), FPN_SCALES)
    ph, pw = pooled
    rng = np.random.default_rng(seed_of("exact_fpn", pooled, ratio, aligned, pow2_only))
    choices = _bin_choices(ratio, pow2_only) + ([] if pow2_only else [9, 12])
    rows_img, tags = [[], [], []], {}
    for l, sc in enumerate(FPN_SCALES):
        lo, hi = _level_range(l)
        H, W = hw[l]
        got = 0
        for _ in range(4000):
            if got == 6:
                break
            bh, bw = rng.choice(choices), rng.choice(choices)
            side = np.sqrt(bh * ph * bw * pw) / sc
            if not (lo * 1.02 <= side < hi * 0.98) or max(bh * ph, bw * pw) > 3 * max(H, W) + 16:
                continue
            if not (_clamp_safe(bh, ph, aligned) and _clamp_safe(bw, pw, aligned)):
                continue
            sx = rng.integers(-8 * 3 - int(4 * bw * pw), 8 * W - int(4 * bw * pw) + 1) / 8.0
            sy = rng.integers(-8 * 3 - int(4 * bh * ph), 8 * H - int(4 * bh * ph) + 1) / 8.0
            img = (0, 2)[got % 2]
            tags.setdefault(f"level_{l}", []).append((img, len(rows_img[img])))
            rows_img[img].append(box_of(sc, aligned, sx, sy, bw * pw, bh * ph))
            got += 1
        assert got == 6, (pooled, ratio, l)
    n = [len(r) for r in rows_img]
    P = max(n) + 2
    flat_tags = {t: [i * P + k for i, k in v] for t, v in tags.items()}
    name = f"exact_fpn{'_pow2' if pow2_only else ''}[{ph}x{pw},ratio{ratio},{'aligned' if aligned else 'legacy'}]"
    case = _pack(name, hw, FPN_SCALES, 3, [np.stack(r) if r else np.zeros((0, 4), F32) for r in rows_img], flat_tags, pooled, ratio,
                 aligned, counts=np.array(n, np.int32), P=P)
    lv = case_levels(case)
    for l in range(4):
        assert all(lv[r] == l for r in flat_tags[f"level_{l}"]), (name, l)
    return case


EXACT_CONFIGS = [((7, 7), 0, True), ((7, 7), 2, False), ((8, 8), 0, False), ((8, 8), 4, True), ((3, 5), 2, True), ((3, 5), 0, False),
                 ((7, 3), 0, True), ((1, 1), 0, True), ((2, 4), 4, False), ((2, 4), 0, True), ((9, 7), 0, True), ((14, 14), 2, True)]


@functools.lru_cache(maxsize=None)
def exact_cases():
    """name -> builder result, every case of the exact family (rows with exact False are marked in the case)."""
    cases = [exact_single(p, r, a) for p, r, a in EXACT_CONFIGS]
    cases += [exact_fpn(p, r, a) for p, r, a in (((7, 7), 0, True), ((8, 8), 2, False), ((3, 5), 0, True), ((2, 4), 4, True))]
    cases += [exact_grid_seam(True), exact_grid_seam(False), exact_table_seam(), exact_min_size((8, 8)), exact_min_size((2, 4)),
              exact_negative(1), exact_negative(4)]
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def backward_cases():
    """The exact family restricted to sample counts that are powers of two (rows that are not are left to pow2_count_rows)."""
    cases = [exact_single((7, 7), 0, True, pow2_only=True), exact_single((2, 4), 0, False, pow2_only=True),
             exact_single((7, 7), 2, True, pow2_only=True), exact_single((2, 4), 4, True, pow2_only=True),
             exact_fpn((7, 7), 0, True, pow2_only=True), exact_fpn((2, 4), 2, False, pow2_only=True), exact_negative(4)]
    return {c.name: c for c in cases}


# ------------------------------------------------------------------------------------------------ level seams
class Seams(NamedTuple):
    boxes: np.ndarray     # [n, 4] float32
    seam: np.ndarray      # [n] j of the seam (224 * 2^j)^2 the box sits at
    k: np.ndarray         # [n] float32 ulps one side was moved by
    level: np.ndarray     # [n] the oracle's level
    kept: np.ndarray      # [n] the oracle's level survives one float32 ulp of its log2 either way
    core: np.ndarray      # [n] k in -6 .. 6 (the 156 cases the kept share is counted on); the rest are the wider steps
    far: np.ndarray       # [m, 4] boxes far from any seam, tiny boxes (p2) and whole-image boxes (p5)
    far_level: np.ndarray


@functools.lru_cache(maxsize=None)
def level_seams():
    boxes, seam, ks = [], [], []
    for j in (-1, 0, 1):
        B = 224.0 * 2.0 ** j
        for w, h in ((B, B), (B / 2, 2 * B), (B / 4, 4 * B), (7 * B / 8, 8 * B / 7)):
            assert w * h == B * B and float(F32(h)) == h
            # -6 .. 6, and wider steps: at j = -1 and j = 1 the sum 4 + log2 lands within an ulp of the integer for every k in
            # -6 .. -1, so none of those survives the one-ulp test and the low side of these two seams needs boxes further out
            for k in list(range(-6, 7)) + [-64, -16, 16, 64]:
                wk = F32(w)
                for _ in range(abs(k)):
                    wk = np.nextafter(wk, F32(np.inf if k > 0 else -np.inf), dtype=F32)
                boxes.append([0.0, 0.0, wk, h])      # corners at the origin: the side IS the corner, no subtraction rounds
                seam.append(j)
                ks.append(k)
    boxes = np.array(boxes, F32)
    level = oracle_levels(boxes)
    kept = (levels_restated(boxes, -1) == level) & (levels_restated(boxes, 1) == level)
    far = np.array([[0, 0, 40, 60], [0, 0, 150, 160], [0, 0, 300, 330], [0, 0, 640, 700], [3, 5, 3, 5], [7, 9, 7.001, 9.001],
                    [0, 0, 1e-3, 1e-3], [0, 0, 1024, 800], [0, 0, 512, 512], [10, 20, 90, 50]], F32)
    ks = np.array(ks)
    return Seams(boxes, np.array(seam), ks, level, kept, np.abs(ks) <= 6, far, oracle_levels(far))


@functools.lru_cache(maxsize=None)
def level_case():
    """The kept seam boxes and the far boxes as one boxes-form case on the four levels of a 512 x 512 image, two images, both
    with dead rows; pooled (2, 2) and one sample per bin keep the work small, and every box has a sample inside its level's map
    (boxes start at the origin), so its gradient shows where the backward kernel sent it."""
    s = level_seams()
    b = np.concatenate([s.boxes[s.kept], s.far])
    half = (len(b) + 1) // 2
    rows = [b[:half], b[half:]]
    P = half + 5
    return _pack("level_seams", hw_of((512, 512), FPN_SCALES), FPN_SCALES, 2, rows, {}, (2, 2), 1, True,
                 counts=np.array([len(rows[0]), len(rows[1])], np.int32), P=P)


# ------------------------------------------------------------------------------------------------ random family
RANDOM_CONFIGS = [((7, 7), 0, True), ((7, 7), 2, False), ((8, 8), 0, False), ((8, 8), 4, True), ((3, 5), 2, True), ((7, 3), 0, True),
                  ((1, 1), 0, True), ((2, 4), 4, False), ((9, 7), 0, True), ((14, 14), 2, True)]


@functools.lru_cache(maxsize=None)
def random_case(pooled, ratio, aligned, n_boxes=150):
    """Four levels of a 96 x 128 image (24 x 32 down to 3 x 4), N = 2, 2 x 150 boxes: sides log-uniform in [0.6, 160] px and
    independent, centres from 10 % outside the image on every side; N(0, 1) features."""
    rng = np.random.default_rng(seed_of("random", pooled, ratio, aligned))
    hw = hw_of((96, 128), FPN_SCALES)
    wh = np.exp(rng.uniform(np.log(0.6), np.log(160.0), (2, n_boxes, 2)))
    ctr = rng.uniform(-0.1, 1.1, (2, n_boxes, 2)) * np.array([128.0, 96.0])
    boxes = np.concatenate([ctr - wh / 2, ctr + wh / 2], axis=2).astype(F32)
    R = 2 * n_boxes
    name = f"random[{pooled[0]}x{pooled[1]},ratio{ratio},{'aligned' if aligned else 'legacy'}]"
    return Case(name, hw, list(FPN_SCALES), 2, boxes, np.array([n_boxes, n_boxes - 7], np.int32), tuple(pooled), ratio, aligned,
                np.zeros(R, bool), np.zeros(R, bool), {}, True)


def fp16_bound(ref, A, terms):
    """|got - ref| <= 2^-11 |ref| + 2^-25 + (npx + grid_h + grid_w + 4) * 2^-24 * A / count, per element.  The first two terms are
    the fp16 store (half an ulp of a normal, half the subnormal spacing); the last is a first-order bound for the float32 table
    sums (grid terms per axis), the products and the npx fused accumulations, and the division.  A comes divided by count."""
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + (terms[..., None] + 4) * 2.0 ** -24 * A
