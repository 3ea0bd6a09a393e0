"""Shared code of tests/test_conv_exact_gpu.py (asserts on the kernels) and tests/test_conv_exact_cpu.py (asserts on this file):
operands on dyadic grids, float64 host references, planted non-finite pixels with their footprints from geometry, the bit
comparator, and the mutants the comparator has to reject.  No GPU is touched here.

Grid construction.  Every operand is an integer times a power of two: x = xi * ux, w = wi * uw, bias and residual integers
times the product grid g = ux * uw.  Any partial sum of such terms is an integer times g, so it is exact in fp32 - in every
summation order - while  max over outputs of (sum |x w| + |b| + |res|) / g  stays under BUDGET.  An fp16 output is then one
round-to-nearest-even of an exact number and an fp32 output is the number itself.  The integer ranges are sized so that the
exact outputs have a spread of about 2^12 grid steps: fp16 keeps 11 bits, so most outputs are inexact in fp16 and a good share
are exact ties.  In a fused chain the fp16-rounded intermediate is still an integer times g (rounding only coarsens it), the
next stage lives on g times its own weight unit, and the same conditions are asserted at every rounding point."""
import dataclasses
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

BUDGET = 2 ** 20            # grid steps an exact accumulator may need: four bits under fp32's 24
MIN_INEXACT = 0.01          # share of the values at an fp16 rounding point that are not representable in fp16
MIN_TIES = 16               # values exactly halfway between two fp16 neighbours
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ operands
def ints(g, shape, amp, zeros=0.0):
    v = torch.randint(-amp, amp + 1, tuple(shape), generator=g).double()
    if zeros:
        v[torch.rand(tuple(shape), generator=g) < zeros] = 0.0
    return v


def amplitudes(K, spread=4096.0):
    """Integer amplitudes (ax, aw), powers of two, of x and w for a reduction of K terms: the exact output then spreads over
    about `spread` grid steps (uniform integers: sigma = a / sqrt(3); a quarter of the weights are zero)."""
    prod = spread * 3.0 / (math.sqrt(0.75) * math.sqrt(K))
    p = max(2, round(math.log2(prod)))
    return 2 ** ((p + 1) // 2), 2 ** (p // 2)


def seed_of(*key):
    s = 0
    for c in repr(key):
        s = (s * 131 + ord(c)) % (2 ** 31 - 1)
    return s


# ------------------------------------------------------------------------------------------------ float64 references (NHWC, OHWI)
def out_hw(H, W, k, stride):
    p = k // 2
    return (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1


def pad_zero(x, p):
    N, H, W, C = x.shape
    xp = x.new_zeros((N, H + 2 * p, W + 2 * p, C))
    xp[:, p:p + H, p:p + W] = x
    return xp


def conv_ref(x, w, b=None, stride=1, padder=pad_zero):
    """x [N,H,W,C] float64, w [Cout,k,k,Cin <= C] float64, pad k // 2: one matrix product per tap, summed in float64."""
    Co, k, _, Ci = w.shape
    N, H, W, _ = x.shape
    Ho, Wo = out_hw(H, W, k, stride)
    xp = padder(x[..., :Ci], k // 2)
    acc = torch.zeros((N * Ho * Wo, Co), dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            a = xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
            acc += a.reshape(-1, Ci) @ w[:, kh, kw].t()
    if b is not None:
        acc += b
    return acc.view(N, Ho, Wo, Co)


def conv_ref_at(x, w, b, pix, stride=1):
    """conv_ref at the output pixels pix [P,3] = (n, oh, ow) only -> [P, Cout]."""
    Co, k, _, Ci = w.shape
    xp = pad_zero(x[..., :Ci], k // 2)
    n, oh, ow = pix[:, 0], pix[:, 1], pix[:, 2]
    acc = torch.zeros((len(pix), Co), dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            acc += xp[n, oh * stride + kh, ow * stride + kw] @ w[:, kh, kw].t()
    return acc if b is None else acc + b


def upsample2(r, Ho, Wo):
    return r.repeat_interleave(2, 1).repeat_interleave(2, 2)[:, :Ho, :Wo]


def relu(y):
    """max(y, 0) that keeps NaN (torch.relu's contract, the kernels' relu_nan): -inf -> 0, +inf stays."""
    return torch.where(y < 0, torch.zeros_like(y), y)


def to_half(y):
    """One round-to-nearest-even of the exact float64 value (float64 -> fp32 is exact under the budget, so there is no double rounding)."""
    return y.float().half()


def maxpool_ref(x):
    """max_pool2d(3, 2, 1) on NHWC: NaN wins, the padding never does."""
    return torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the generator's conditions
def rounding_stats(y):
    """(share of y not representable in fp16, number of exact ties) of a finite float64 tensor."""
    a = y.detach().numpy().ravel()
    h = a.astype(np.float32).astype(np.float16)
    hd = h.astype(np.float64)
    inexact = hd != a
    toward = np.where(a > hd, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16)
    other = np.nextafter(h, toward).astype(np.float64)
    ties = inexact & (np.abs(a - hd) == np.abs(other - a))
    return float(inexact.mean()), int(ties.sum())


def check_point(name, exact, mag, grid, fp16_point=True):
    """One accumulation (+ rounding) point: `exact` the float64 value before the rounding, `mag` the float64 sum of the absolute terms."""
    assert bool(torch.isfinite(exact).all()), name
    steps = exact / grid
    assert bool((steps == steps.round()).all()), f"{name}: off the grid"
    used = float(mag.max()) / grid
    assert used < BUDGET, f"{name}: needs 2^{math.log2(used):.1f} grid steps, budget 2^{math.log2(BUDGET):.0f}"
    assert bool((exact.float().double() == exact).all()), f"{name}: not exact in fp32"
    stats = {"name": name, "log2_budget_used": math.log2(max(used, 1.0))}
    if fp16_point:
        share, ties = rounding_stats(exact)
        assert share >= MIN_INEXACT, f"{name}: only {share:.4f} of the values are inexact in fp16"
        assert ties >= MIN_TIES, f"{name}: only {ties} exact ties"
        stats.update(inexact=share, ties=ties)
    return stats


# ------------------------------------------------------------------------------------------------ comparator
def assert_bits(got, want, what=""):
    """NaN exactly where the reference has NaN; every other element the same bits (the sign of infinities and zeros included)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        bad = torch.nonzero(gn != wn)
        raise AssertionError(f"{what}: NaN masks differ at {len(bad)} elements, first {bad[0].tolist()} (kernel NaN: {bool(gn[tuple(bad[0])])})")
    iv = torch.int16 if got.dtype == torch.float16 else torch.int32
    gb = torch.where(gn, torch.zeros_like(got), got).contiguous().view(iv)
    wb = torch.where(wn, torch.zeros_like(want), want).contiguous().view(iv)
    if not torch.equal(gb, wb):
        bad = torch.nonzero(gb != wb)
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ in bits, first at {list(i)}: got {float(got[i])!r}, want {float(want[i])!r}")


def rejects(got, want):
    try:
        assert_bits(got, want)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------ planted pixels, footprints
TILE_EDGES = (31, 32, 127, 128, 255, 256)


def plant_sets(N, H, W, k=3, stride=1, min_dist=None):
    """Input pixels (n, h, w) to plant a bad value at, split into sets whose members are at least max(3, k) apart (Chebyshev) where
    they share an image, so that no receptive field holds two of them: the corners of the first and the last image, both ends of an
    interior row, the last pixel of image 0 and the first of image 1, the output pixels on either side of every tile edge
    (m = 31/32, 127/128, 255/256, M - 1) taken back to the input, one interior pixel, and - at stride 2 - a pixel no output samples."""
    d = max(3, k) if min_dist is None else min_dist
    Ho, Wo = out_hw(H, W, k, stride)
    cand = []
    for n in sorted({0, N - 1}):
        cand += [(n, 0, 0), (n, 0, W - 1), (n, H - 1, 0), (n, H - 1, W - 1)]
    hm = H // 2
    cand += [(0, hm, 0), (0, hm, W - 1), (0, hm, W // 2)]
    if N > 1:
        cand += [(0, H - 1, W - 1), (1, 0, 0)]
    M = N * Ho * Wo
    for m in TILE_EDGES + (M - 1,):
        if m < M:
            n, r = divmod(m, Ho * Wo)
            oh, ow = divmod(r, Wo)
            cand.append((n, min(oh * stride, H - 1), min(ow * stride, W - 1)))
    if stride == 2 and H > 1 and W > 1:
        cand.append((0, 1, 1))
    sets = []
    for c in dict.fromkeys(cand):
        for s in sets:
            if all(q[0] != c[0] or max(abs(q[1] - c[1]), abs(q[2] - c[2])) >= d for q in s):
                s.append(c)
                break
        else:
            sets.append([c])
    return sets


def min_spacing(pixels):
    best = 10 ** 9
    for i, a in enumerate(pixels):
        for b in pixels[i + 1:]:
            if a[0] == b[0]:
                best = min(best, max(abs(a[1] - b[1]), abs(a[2] - b[2])))
    return best


def footprint(pixels, N, H, W, k, stride):
    """Output pixels [N,Ho,Wo] whose k x k window (pad k // 2) holds a planted input pixel: from geometry alone."""
    Ho, Wo = out_hw(H, W, k, stride)
    m = torch.zeros((N, Ho, Wo), dtype=torch.bool)
    p = k // 2
    for n, h, w in pixels:
        for kh in range(k):
            for kw in range(k):
                a, b = h + p - kh, w + p - kw
                if a % stride == 0 and b % stride == 0 and 0 <= a // stride < Ho and 0 <= b // stride < Wo:
                    m[n, a // stride, b // stride] = True
    return m


def pool_footprint(mask):
    """A [N,H,W] mask through max_pool2d(3, 2, 1): the pooled pixels whose window holds a marked one."""
    N, H, W = mask.shape
    Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out = torch.zeros((N, Hp, Wp), dtype=torch.bool)
    for n, h, w in torch.nonzero(mask).tolist():
        for a in {(h + 1) // 2, h // 2}:
            for b in {(w + 1) // 2, w // 2}:
                if a < Hp and b < Wp and abs(2 * a - h) <= 1 and abs(2 * b - w) <= 1:
                    out[n, a, b] = True
    return out


def plant(x, pixels, value, channel=0):
    x = x.clone()
    for n, h, w in pixels:
        x[n, h, w, channel] = value
    return x


# ------------------------------------------------------------------------------------------------ cases: one convolution
@dataclass(frozen=True)
class Conv:
    name: str
    N: int
    H: int
    W: int
    Cin: int
    Cout: int
    k: int = 1
    stride: int = 1
    relu: bool = False
    res_mode: int = 0
    f32out: bool = False
    policy: int = -1            # tile_bits of pe_test_set_conv_policy; -1 = the library's default
    reuse: int = 1
    variant: str = ""           # the kernel that has to take the launch
    api: str = "conv"           # conv | linear | wd | wd9 | stem | stem_pool
    window: tuple = ()          # (offset, stride) of a channel-window output
    heavy: bool = False         # planted cases recompute the reference at the footprint only

    @property
    def K(self):
        return self.k * self.k * self.Cin

    @property
    def out_hw(self):
        return out_hw(self.H, self.W, self.k, self.stride)


COPY_CH = 3                     # output channel that the overflow operands turn into a copy of input channel 0 plus a bias
SIGN_ROWS = (0, 1, 2)           # output channels whose weight on input channel 0 is forced to 0, +, - (what an Inf there becomes)


def force_signs(wi, amp):
    wi[SIGN_ROWS[0], ..., 0] = 0
    wi[SIGN_ROWS[1], ..., 0] = wi[SIGN_ROWS[1], ..., 0].abs().clamp(min=1)
    wi[SIGN_ROWS[2], ..., 0] = -wi[SIGN_ROWS[2], ..., 0].abs().clamp(min=1)
    return wi


def conv_operands(c, spread=4096.0):
    """float64 operands of a Conv case: x [N,H,W,C], w [Cout,k,k,Cin] (OHWI), b [Cout], res (or None), and the grid."""
    g = torch.Generator().manual_seed(seed_of(c.N, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.res_mode))
    ax, aw = amplitudes(c.K, spread)
    ux, uw = 2.0 / ax, 1.0 / aw
    grid = ux * uw
    cx = 4 if c.api in ("stem", "stem_pool") else c.Cin
    x = torch.zeros((c.N, c.H, c.W, cx), dtype=torch.float64)
    x[..., :c.Cin] = ints(g, (c.N, c.H, c.W, c.Cin), ax) * ux
    w = force_signs(ints(g, (c.Cout, c.k, c.k, c.Cin), aw, zeros=0.25), aw) * uw
    b = ints(g, (c.Cout,), 2048) * grid
    Ho, Wo = c.out_hw
    res = None
    if c.res_mode == 1:
        res = ints(g, (c.N, Ho, Wo, c.Cout), 1023) * (8 * grid)
    elif c.res_mode == 2:
        res = ints(g, (c.N, (Ho + 1) // 2, (Wo + 1) // 2, c.Cout), 1023) * (8 * grid)
    return {"x": x, "w": w, "b": b, "res": res, "grid": grid}


def res_term(c, ops):
    Ho, Wo = c.out_hw
    if c.res_mode == 1:
        return ops["res"]
    if c.res_mode == 2:
        return upsample2(ops["res"], Ho, Wo)
    return None


def conv_exact(c, ops, at=None):
    """The exact float64 value in front of the output rounding (all of it, or at the output pixels `at` [P,3] only)."""
    if at is None:
        y = conv_ref(ops["x"], ops["w"], ops["b"], c.stride)
        r = res_term(c, ops)
    else:
        y = conv_ref_at(ops["x"], ops["w"], ops["b"], at, c.stride)
        r = res_term(c, ops)
        r = None if r is None else r[at[:, 0], at[:, 1], at[:, 2]]
    if r is not None:
        y = y + r
    return relu(y) if c.relu else y


def conv_finish(c, y):
    if c.api == "stem_pool":
        return maxpool_ref(to_half(y).double()).half()
    return y.float() if c.f32out else to_half(y)


def conv_expected(c, ops):
    return conv_finish(c, conv_exact(c, ops))


@functools.lru_cache(maxsize=None)
def _conv_clean(c):
    ops = conv_operands(c)
    exact = conv_exact(c, ops)
    return ops, exact, conv_finish(c, exact)


def _shape_key(c):
    """Cases that differ only in the kernel they select share operands and reference."""
    return dataclasses.replace(c, name="", policy=-1, reuse=1, variant="", window=(), heavy=False,
                               api=c.api if c.api in ("stem", "stem_pool") else "conv")


def conv_clean(c):
    """(operands, expected output) of a case, computed once per process and never modified (callers clone what they change)."""
    ops, _, want = _conv_clean(_shape_key(c))
    return ops, want


def conv_conditions(c):
    ops, exact, _ = _conv_clean(_shape_key(c))
    a = {"x": ops["x"].abs(), "w": ops["w"].abs(), "b": ops["b"].abs(), "res": None if ops["res"] is None else ops["res"].abs()}
    mag = conv_ref(a["x"], a["w"], a["b"], c.stride)
    r = res_term(c, a)
    if r is not None:
        mag = mag + r
    return [check_point(c.name, exact, mag, ops["grid"], fp16_point=not c.f32out)]


def with_overflow(c, ops, pixels):
    """Operands whose output channel COPY_CH is input channel 0 (one unit weight on the centre tap) plus a chosen fp32 bias, so
    that the exact accumulator is under the test's control: bias 65518 and x in {1.875, 2.0} give 65519.875 (rounds to 65504) and
    65520 (the tie that rounds to even: +inf).  With a residual the bias is 69998 and the residual -10000 at the planted pixels:
    70000 - 10000 is a finite 60000 only when the addition happens in fp32 in front of the one rounding.  b + x has one non-zero
    product and needs 22 bits, so it is exact in fp32 (asserted) although it is outside the BUDGET of the other channels."""
    o = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ops.items()}
    o["w"][COPY_CH] = 0
    o["w"][COPY_CH, c.k // 2, c.k // 2, 0] = 1.0
    o["b"][COPY_CH] = 69998.0 if c.res_mode else 65518.0
    for i, (n, h, w) in enumerate(pixels):
        o["x"][n, h, w, 0] = 2.0 if i % 2 == 0 else 1.875
    if c.res_mode:
        o["res"][..., COPY_CH] = -10000.0 + 8.0 * torch.randint(-3, 1, o["res"].shape[:-1], generator=torch.Generator().manual_seed(5)).double()
    return o


# ------------------------------------------------------------------------------------------------ cases: fused chains
@dataclass(frozen=True)
class Chain:
    name: str
    kind: str                   # head | tail | bneck
    N: int
    H: int
    W: int
    Cin: int = 64
    Cout: int = 256             # tail: conv3's outputs
    res: bool = False           # tail: with a residual
    sc: bool = False            # bneck: convolution shortcut
    nxt: bool = False           # bneck: the next block's conv1
    gen: str = "wd"             # wd | wd9
    k: int = 3
    stride: int = 1


def chain_operands(c):
    g = torch.Generator().manual_seed(seed_of(c.kind, c.N, c.H, c.W, c.Cin, c.Cout, c.res, c.sc, c.nxt))
    spread = 2048.0 if c.kind == "bneck" else 4096.0
    ax, aw = amplitudes(9 * c.Cin, spread)
    ux, uw = 2.0 / ax, 1.0 / aw
    g1 = ux * uw
    o = {"x": ints(g, (c.N, c.H, c.W, c.Cin), ax) * ux, "g1": g1}
    cmid = 64 if c.kind == "bneck" else 256
    o["w"] = force_signs(ints(g, (cmid, 3, 3, c.Cin), aw, zeros=0.25), aw) * uw
    o["b"] = ints(g, (cmid,), 1024) * g1
    u2 = 0.25
    g2 = g1 * u2
    o["g2"] = g2
    if c.kind == "head":
        o["w2"] = ints(g, (15, 256), 2, zeros=0.4) * u2
        o["b2"] = ints(g, (15,), 4096) * g2
    elif c.kind == "tail":
        o["w2"] = ints(g, (c.Cout, 256), 2, zeros=0.4) * u2
        o["b2"] = ints(g, (c.Cout,), 4096) * g2
        o["res"] = ints(g, (c.N, c.H, c.W, c.Cout), 1023) * (16 * g2) if c.res else None
    else:
        o["w2"] = ints(g, (256, 64), 1, zeros=0.5) * u2
        o["b2"] = ints(g, (256,), 1024) * g2
        if c.sc:                                    # shortcut convolution 64 -> 256 on the grid g2 = us * uws
            us = 2.0 ** math.floor(math.log2(g2) / 2)
            o["src"] = ints(g, (c.N, c.H, c.W, 64), 16) * us
            o["wsc"] = ints(g, (256, 64), 8, zeros=0.25) * (g2 / us)
            o["bsc"] = ints(g, (256,), 1024) * g2
        else:
            o["src"] = ints(g, (c.N, c.H, c.W, 256), 1023) * (2 * g2)
        if c.nxt:
            o["w3"] = ints(g, (64, 256), 1, zeros=0.5) * u2
            o["g3"] = g2 * u2
            o["b3"] = ints(g, (64,), 4096) * o["g3"]
    return o


def chain_stages(c, o, absolute=False):
    """The chain in float64 with an fp16 rounding wherever the kernel has one.  Returns a list of (name, exact value in front of the
    rounding or of the fp32 store, grid, is an fp16 rounding point) and the outputs.  absolute = the sums of absolute terms along
    the same intermediates (the budget's numerator)."""
    A = (lambda v: v.abs()) if absolute else (lambda v: v)
    mm = lambda t, w: (t.reshape(-1, t.shape[-1]) @ A(w).t()).view(*t.shape[:-1], w.shape[0])
    pts = []
    t_exact = conv_ref(A(o["x"]), A(o["w"]), A(o["b"]))
    t_exact = t_exact if absolute else relu(t_exact)
    pts.append(("t", t_exact, o["g1"], True))
    t = o["_t"] if absolute else to_half(t_exact).double()          # the magnitudes ride on the REAL rounded intermediate
    if c.kind == "head":
        y = mm(A(t), o["w2"]) + A(o["b2"])
        pts.append(("head", y, o["g2"], False))
        return pts, {"t": t, "out": y.float()}
    if c.kind == "tail":
        y = mm(A(t), o["w2"]) + A(o["b2"])
        if o["res"] is not None:
            y = y + A(o["res"])
        y = y if absolute else relu(y)
        pts.append(("out", y, o["g2"], True))
        return pts, {"t": t, "out": to_half(y)}
    y = mm(A(t), o["w2"]) + A(o["b2"])
    y = y + (mm(A(o["src"]), o["wsc"]) + A(o["bsc"]) if c.sc else A(o["src"]))
    y = y if absolute else relu(y)
    pts.append(("out", y, o["g2"], True))
    out = o["_out"] if absolute else to_half(y)
    outs = {"t": t, "out": out}
    if c.nxt:
        z = mm(A(out.double()), o["w3"]) + A(o["b3"])
        z = z if absolute else relu(z)
        pts.append(("t1_next", z, o["g3"], True))
        outs["t1_next"] = to_half(z)
    return pts, outs


def chain_expected(c, o):
    return chain_stages(c, o)[1]


def chain_conditions(c):
    o = chain_clean(c)[0]
    pts, outs = chain_stages(c, o)
    a = dict(o)
    a["_t"], a["_out"] = outs["t"], outs["out"]
    mags, _ = chain_stages(c, a, absolute=True)
    return [check_point(f"{c.name}.{n}", e, m[1], gr, f16) for (n, e, gr, f16), m in zip(pts, mags)]


@functools.lru_cache(maxsize=None)
def chain_clean(c):
    o = chain_operands(c)
    return o, chain_expected(c, o)


def chain_with_overflow(c, o, pixels):
    """The first stage's channel COPY_CH becomes a copy of input channel 0 plus 65518: t overflows to +inf in fp16 exactly where
    x is 2.0 (65520, the tie) and stays 65504 where x is 1.875, and the second stage has to carry that infinity like the reference."""
    o = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()}
    o["w"][COPY_CH] = 0
    o["w"][COPY_CH, 1, 1, 0] = 1.0
    o["b"][COPY_CH] = 65518.0
    for i, (n, h, w) in enumerate(pixels):
        o["x"][n, h, w, 0] = 2.0 if i % 2 == 0 else 1.875
    # 65504 = 2047 * 2^5 times a weight of 2^-12 is a multiple of 2^-7: on the second stage's grid and small, so that stage stays exact
    o["w2"][:, COPY_CH] = torch.sign(o["w2"][:, COPY_CH]) * 2.0 ** -12
    return o


# ------------------------------------------------------------------------------------------------ the case lists
IG64, IG128 = "conv_igemm2_kernel<128, 64, 0, 1>", "conv_igemm2_kernel<128, 128, 0, 1>"
RING = "conv1x1_ring_kernel"

CONV_CASES = [
    # the generic LDS-DMA 1x1 at <128,64> and <128,128>: one tile (the plainest case), stride 2, residual modes on odd sizes, fp32 15-of-16
    Conv("ig64_one_tile", 1, 7, 9, 64, 64, variant=IG64),
    Conv("ig64_res1", 2, 13, 15, 128, 64, relu=True, res_mode=1, variant=IG64),
    Conv("ig64_res2", 2, 13, 15, 128, 64, res_mode=2, variant=IG64),
    Conv("ig64_s2", 2, 13, 15, 64, 64, stride=2, relu=True, variant=IG64),
    Conv("ig64_f32_15", 2, 20, 24, 256, 15, f32out=True, variant=IG64),
    Conv("ig128_k2048", 1, 7, 9, 2048, 128, variant=IG128),
    Conv("ig128_s2", 3, 51, 63, 256, 128, stride=2, relu=True, variant=IG128),
    Conv("ig128_res1", 2, 13, 15, 256, 128, res_mode=1, variant=IG128),
    Conv("ig128_res2", 2, 13, 15, 256, 128, relu=True, res_mode=2, variant=IG128),
    # kw-reuse 3x3: 128-row tiles at both widths, 256-row tiles at the smallest M with 512 of them (ragged, odd width)
    Conv("rb64", 2, 9, 11, 64, 64, k=3, relu=True, variant="conv3x3rb_kernel<128, 64>"),
    Conv("rb128", 2, 13, 16, 512, 128, k=3, variant="conv3x3rb_kernel<128, 128>"),
    Conv("rb256", 1, 129, 126, 64, 1024, k=3, relu=True, variant="conv3x3rb_kernel<256, 128>", heavy=True),
    # generic per-tap 3x3
    Conv("tap64", 2, 9, 11, 64, 64, k=3, relu=True, reuse=0, variant="conv_igemm2_kernel<128, 64, 1, 1>"),
    Conv("tap128", 2, 13, 16, 128, 128, k=3, reuse=0, variant="conv_igemm2_kernel<128, 128, 1, 1>"),
    # 256x256 two-stage kernel under policy 25: 1x1 with both residual modes (stride 2 on odd sizes), ragged M, and its 3x3 form
    Conv("big_res1", 3, 67, 71, 64, 1024, relu=True, res_mode=1, policy=25, variant="conv_big_kernel<0>"),
    Conv("big_s2_res2", 3, 133, 141, 64, 1024, stride=2, res_mode=2, policy=25, variant="conv_big_kernel<0>"),
    Conv("big_3x3", 1, 129, 126, 64, 1024, k=3, relu=True, policy=25, variant="conv_big_kernel<1>", heavy=True),
    # persistent ring 1x1
    Conv("ring_k128_res1", 2, 9, 11, 128, 256, relu=True, res_mode=1, variant=RING),
    Conv("ring_k512", 1, 7, 9, 512, 256, relu=True, variant=RING),
    Conv("ring_k2048", 1, 13, 16, 2048, 512, variant=RING),
    Conv("ring_s2_odd", 3, 51, 65, 256, 1024, stride=2, relu=True, variant=RING),       # four column tiles
    Conv("ring_res2_odd", 2, 25, 31, 128, 256, res_mode=2, variant=RING),
    # linear_f16 at a ragged M: ring path and generic path
    Conv("linear_ring", 333, 1, 1, 1024, 256, relu=True, variant=RING, api="linear"),
    Conv("linear_generic", 333, 1, 1, 1024, 128, relu=True, variant=IG128, api="linear"),
    # weights-direct 3x3, both generations: half a row / one row / several rows per tile, ragged last tile, channel window, two channel tiles
    Conv("wd_half_row", 2, 5, 256, 64, 256, k=3, api="wd"),
    Conv("wd9_one_row", 2, 5, 256, 64, 256, k=3, api="wd9"),
    Conv("wd_window", 3, 3, 128, 64, 256, k=3, relu=True, api="wd", window=(256, 512)),
    Conv("wd9_window_ragged", 3, 3, 128, 64, 256, k=3, relu=True, api="wd9", window=(256, 512)),
    Conv("wd_four_rows_ragged", 3, 5, 32, 128, 512, k=3, relu=True, api="wd"),
    Conv("wd_two_rows_ragged", 3, 5, 64, 64, 256, k=3, relu=True, api="wd"),
    Conv("wd9_four_rows_ragged", 3, 5, 64, 64, 256, k=3, relu=True, api="wd9"),
    Conv("wd_two_channel_tiles", 1, 9, 64, 128, 512, k=3, api="wd"),
    Conv("wd9_two_channel_tiles", 1, 9, 64, 128, 512, k=3, api="wd9"),
    # 7x7 stem and fused stem + pool: cin 3 and 4, a pooled size (9 x 11) that is no multiple of the 4 x 16 tile
    Conv("stem_c3", 2, 36, 44, 3, 64, k=7, stride=2, relu=True, api="stem", variant="conv_igemm_kernel<128, 64, 2>"),
    Conv("stem_c4", 1, 32, 48, 4, 64, k=7, stride=2, relu=True, api="stem", variant="conv_igemm_kernel<128, 64, 2>"),
    Conv("stem_pool_c3", 2, 36, 44, 3, 64, k=7, stride=2, relu=True, api="stem_pool"),
    Conv("stem_pool_c4", 1, 32, 48, 4, 64, k=7, stride=2, relu=True, api="stem_pool"),
]

CHAIN_CASES = [
    Chain("head_wd_w64", "head", 2, 5, 64), Chain("head_wd9_w64", "head", 2, 5, 64, gen="wd9"),
    Chain("head_wd_w128", "head", 1, 3, 128), Chain("head_wd9_w128", "head", 1, 3, 128, gen="wd9"),
    Chain("head_wd_w32_ragged", "head", 3, 5, 32),
    Chain("tail_res_ragged", "tail", 3, 5, 32, res=True), Chain("tail_nores_512", "tail", 1, 5, 128, Cout=512),
    Chain("tail_res_w64", "tail", 2, 5, 64, res=True),
    Chain("bneck_sc_next", "bneck", 2, 8, 64, sc=True, nxt=True), Chain("bneck_id_next", "bneck", 1, 7, 70, nxt=True),
    Chain("bneck_id", "bneck", 3, 5, 32), Chain("bneck_sc", "bneck", 2, 13, 30, sc=True),
]

by_name = {c.name: c for c in CONV_CASES + CHAIN_CASES}


# ------------------------------------------------------------------------------------------------ mutants (tests/test_conv_exact_cpu.py)
def half_toward_zero(y):
    h = y.float().half()
    a = h.double()
    over = (a.abs() > y.abs()) & torch.isfinite(y)
    down = torch.from_numpy(np.nextafter(h.numpy(), np.float16(0)))
    return torch.where(over, down, h)


def mutant_toward_zero(c, ops):
    return half_toward_zero(conv_exact(c, ops))


def mutant_partial_fp16(c, ops):
    """The first half of the input channels' partial sum takes a detour through fp16."""
    h = c.Cin // 2
    lo = conv_ref(ops["x"][..., :h].contiguous(), ops["w"][..., :h].contiguous(), None, c.stride)
    hi = conv_ref(ops["x"][..., h:c.Cin].contiguous(), ops["w"][..., h:].contiguous(), ops["b"], c.stride)
    y = to_half(lo).double() + hi
    r = res_term(c, ops)
    y = y if r is None else y + r
    return to_half(relu(y) if c.relu else y)


def mutant_residual_after_rounding(c, ops):
    y = to_half(conv_ref(ops["x"], ops["w"], ops["b"], c.stride)).double() + res_term(c, ops)
    return to_half(relu(y) if c.relu else y)


def mutant_dropped_tap(c, ops):
    """Output pixel (0, 0, 1) loses its left neighbour's tap."""
    y = conv_ref(ops["x"], ops["w"], ops["b"], c.stride)
    y[0, 0, 1] -= ops["w"][:, c.k // 2, c.k // 2 - 1] @ ops["x"][0, 0, 0, :c.Cin]
    r = res_term(c, ops)
    y = y if r is None else y + r
    return to_half(relu(y) if c.relu else y)


def mutant_relu_drops_nan(c, ops):
    y = conv_ref(ops["x"], ops["w"], ops["b"], c.stride)
    r = res_term(c, ops)
    y = y if r is None else y + r
    return to_half(torch.where(y > 0, y, torch.zeros_like(y)))


def _pad_linear(scale):
    """A 3x3 halo taken from a linear slab of pixels: the left halo of a row is the previous row's last pixel, the right halo the
    next row's first one (inside an image), times `scale` (0: silenced by a multiply, 1: read through)."""
    def padder(x, p):
        xp = pad_zero(x, p)
        H = x.shape[1]
        xp[:, 2:H + 1, 0] = scale * x[:, :H - 1, -1]
        xp[:, 1:H, -1] = scale * x[:, 1:, 0]
        return xp
    return padder


def mutant_halo_multiplied_by_zero(c, ops):
    y = conv_ref(ops["x"], ops["w"], ops["b"], c.stride, padder=_pad_linear(0.0))
    return to_half(relu(y) if c.relu else y)


def mutant_seam_read_through(c, ops):
    y = conv_ref(ops["x"], ops["w"], ops["b"], c.stride, padder=_pad_linear(1.0))
    return to_half(relu(y) if c.relu else y)
