"""Shared code of tests/test_train_exact_gpu.py (asserts on the kernels) and tests/test_train_exact_cpu.py (asserts on this file):
the training half's references and the mutants they have to tell apart.  No GPU is touched here.

Fused SGD.  One pe_sgd_momentum_f32 call (csrc/optim.hip, built with -ffp-contract=off) restated in numpy float32, one rounding per
operation in the kernel's order, next to a longdouble restatement with a first-order error bound from the sums of the absolute terms.
The float32 restatement is what the kernel has to reproduce bit for bit; its mutants are the kernels a tolerance lets through.

HipLinear.  Operands on conv_exact's dyadic grids, sized so that all THREE products of a training step - x w^T + b over K, dY W over
N, dY^T X over M - stay under conv_exact.BUDGET grid steps: every fp32 accumulator is then the float64 sum in any summation order,
an fp16 output one round-to-nearest-even of it and an fp32 output the sum itself."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

import conv_exact as E

U = 2.0 ** -24              # half an ulp of fp32, relative: |fl(v) - v| <= U |v| for a normal result


# ------------------------------------------------------------------------------------------------ fused SGD
def sgd_scalars(lr, mu, wd, gs):
    """The Python values as the C ABI receives them: each narrowed to float once (ctypes c_float).  FusedSGD passes lr = base * factor,
    a product formed in double: form it in double here too, then narrow."""
    return tuple(np.float32(v) for v in (lr, mu, wd, gs))


def _fma(a, b, c):
    """f32(a * b + c) with the product unrounded: a product of two fp32 values is exact in float64."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


SGD_MUTANTS = ("fma_d", "fma_m", "fma_p", "reads_momentum", "tail_unwritten", "stale_shadow")


def sgd_step_f32(p, g, m, h, lr, mu, wd, gs, first, mutant=None):
    """One call on n elements -> the new (p, m, h).  p, g, m float32 arrays, h the float16 shadow before the call (only a mutant reads it).
        d = f32(g * gs) + f32(wd * p);  m = first ? d : f32(mu * m) + d;  p = p - f32(lr * m);  h = half(p)
    `mutant`: one of SGD_MUTANTS - a contracted line (fused multiply-add: the product is not rounded), the momentum buffer read on
    the first step, the n % 4 tail elements left as they were, the shadow taken from the old p."""
    assert p.dtype == g.dtype == m.dtype == np.float32 and mutant in (None,) + SGD_MUTANTS
    lr, mu, wd, gs = sgd_scalars(lr, mu, wd, gs)
    d = _fma(g, gs, wd * p) if mutant == "fma_d" else g * gs + wd * p
    if first and mutant != "reads_momentum":
        m2 = d
    else:
        m2 = _fma(m, mu, d) if mutant == "fma_m" else mu * m + d
    p2 = _fma(m2, -lr, p) if mutant == "fma_p" else p - lr * m2
    h2 = (p if mutant == "stale_shadow" else p2).astype(np.float16)
    if mutant == "tail_unwritten":
        t = len(p) - len(p) % 4
        p2[t:], m2[t:], h2[t:] = p[t:], m[t:], h[t:]
    assert p2.dtype == m2.dtype == np.float32
    return p2, m2, h2


def sgd_step_longdouble(p, g, m, lr, mu, wd, gs, first):
    """The same step from the same fp32 state and the same narrowed scalars in longdouble -> (p, m, bound on |p32 - p|, bound on |m32 - m|).
    The bounds are first order in U, one term per rounding of the float32 restatement, each scaled by its own result's magnitude:
        d:  U (|g gs| + |wd p| + |d|)                         three roundings
        m:  first step: d's;  later: d's + U (|mu m| + |m'|)   two more
        p:  lr times m's + U (|lr m'| + |p'|)                  two more   (five roundings on the first step, seven on a later one)
    times 1 + 2^-20 for the terms of second order, plus one fp32 denormal step for a result below the normal range."""
    L = np.longdouble
    lr, mu, wd, gs = (L(v) for v in sgd_scalars(lr, mu, wd, gs))
    p, g, m = p.astype(L), g.astype(L), m.astype(L)
    t1, t2 = g * gs, wd * p
    d = t1 + t2
    ed = U * (np.abs(t1) + np.abs(t2) + np.abs(d))
    if first:
        m2, em = d, ed
    else:
        t3 = mu * m
        m2 = t3 + d
        em = ed + U * (np.abs(t3) + np.abs(m2))
    t4 = lr * m2
    p2 = p - t4
    ep = lr * em + U * (np.abs(t4) + np.abs(p2))
    slack, tiny = L(1.0 + 2.0 ** -20), L(2.0 ** -149)
    return p2, m2, ep * slack + tiny, em * slack + tiny


@dataclass(frozen=True)
class Sgd:
    name: str
    lr: float
    mu: float
    wd: float
    gs: float
    shadow: bool = True


# No scalar is a power of two where it multiplies: a product with a power of two is exact and a contracted line would not show.
SGD_CONFIGS = [Sgd("wd_gscale", 0.05, 0.9, 0.01, 1.0 / (3 * 1024.0)),       # three ranks, loss scale 1024
               Sgd("wd0", 0.05, 0.9, 0.0, 1.0),
               Sgd("null_shadow", 0.02, 0.9, 0.0001, 1.0 / (3 * 1024.0), shadow=False)]
SGD_SIZES = [1, 2, 3, 4, 5, 7, 1023, 1025, 4 * 256 * 3 + 2, 4194304 + 1027]
SGD_STEPS = 3


def sgd_operands(n, cfg, seed=0):
    """p and the momentum pre-fill (what a first step must not read: finite here, the GPU test uses NaN), and SGD_STEPS gradients as
    backward leaves them: divided by the gradient scale."""
    rng = np.random.default_rng(E.seed_of("sgd", n, cfg.name, seed))
    f = lambda: rng.standard_normal(n, dtype=np.float32)
    p, m0 = f(), f()
    grads = [f() / np.float32(cfg.gs) for _ in range(SGD_STEPS)]
    return p, m0, grads


def sgd_run(p, m, h, grads, cfg, mutant=None, mutant_steps=None):
    """SGD_STEPS calls, the first with first_step = 1 -> [(p, m, h) after every step]."""
    out = []
    for s, g in enumerate(grads):
        mut = mutant if mutant_steps is None or s in mutant_steps else None
        p, m, h = sgd_step_f32(p, g, m, h, cfg.lr, cfg.mu, cfg.wd, cfg.gs, s == 0, mutant=mut)
        out.append((p, m, h))
    return out


def same_bits(got, want, what=""):
    """numpy arrays: the same dtype, shape and bytes."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        iv = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
        bad = np.nonzero(np.ascontiguousarray(got).view(iv) != np.ascontiguousarray(want).view(iv))[0]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ in bits, first at {int(bad[0])}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


def differing(a, b):
    """Share of the elements of two arrays whose bits differ."""
    iv = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return float((np.ascontiguousarray(a).view(iv) != np.ascontiguousarray(b).view(iv)).mean())


# ------------------------------------------------------------------------------------------------ HipLinear on exact operands
IG64, IG128, RING = E.IG64, E.IG128, E.RING


@dataclass(frozen=True)
class Linear:
    name: str
    M: int
    K: int
    N: int
    relu: bool
    out_f32: bool
    fwd: str                    # the kernels that have to take the three launches
    dx: str
    dw: str

    @property
    def pad(self):              # rows _pad_rows adds in front of the dW launch
        return -self.M % 64


LINEAR_CASES = [
    Linear("a_one_kstep_narrow", 50, 64, 64, False, True, IG64, IG64, IG64),
    Linear("b_ragged_tiles_relu", 130, 128, 192, True, False, IG128, IG128, IG128),
    Linear("c_predictor", 64, 1024, 64, False, True, IG64, IG128, IG128),
    Linear("d_ring_forward_relu", 333, 1024, 256, True, False, RING, IG128, IG128),
]
linear_by_name = {c.name: c for c in LINEAR_CASES}


def linear_operands(c):
    """float64 x [M,K], w [N,K], b [N], dy [M,N] and their units.  x and w get conv_exact.amplitudes of the forward reduction K; dy's
    amplitude is what the same rule gives the dX reduction (N terms, half of them masked under a ReLU) divided by w's.  Element
    (0, 0) is planted: the bias of column 0 makes its pre-activation exactly 0, and its dy is not 0."""
    g = torch.Generator().manual_seed(E.seed_of("linear", c.M, c.K, c.N, c.relu))
    ax, aw = E.amplitudes(c.K)
    da, db = E.amplitudes(c.N * (0.5 if c.relu else 1.0))
    ad = max(1, da * db // aw)
    ux, uw, ud = 2.0 / ax, 1.0 / aw, 1.0 / ad
    x = E.ints(g, (c.M, c.K), ax) * ux
    w = E.ints(g, (c.N, c.K), aw, zeros=0.25) * uw
    b = E.ints(g, (c.N,), 2048) * (ux * uw)
    dy = E.ints(g, (c.M, c.N), ad) * ud
    b[0] = -(x[0] @ w[0])
    if float(dy[0, 0]) == 0.0:
        dy[0, 0] = ud
    bk = (E.ints(g, (c.K,), 1024).abs() + 1) * (ud * uw)            # only the mutant that adds a bias to dX reads it
    return {"x": x, "w": w, "b": b, "dy": dy, "bk": bk, "ux": ux, "uw": uw, "ud": ud}


LINEAR_MUTANTS = ("mask_ge", "tail_row_zeroed", "pad_rows_counted", "bias_on_dx")


def linear_stages(c, o, mutant=None):
    """HipLinear forward + backward in float64, rounded where the kernels round.  Returns the exact values in front of every rounding
    / fp32 store and the outputs {y, dx, dw, db} in the dtypes HipLinear returns.  `+ 0.0`: an fp32 accumulator starts at +0 and
    +0 + -0 is +0 under round-to-nearest, so a sum that cancels - or whose terms are all signed zeros, as behind the mask, where
    a negative dy times 0 is -0 - is +0 in the kernel (the launches without a bias add nothing behind it)."""
    assert mutant in (None,) + LINEAR_MUTANTS
    x, w, b, dy = o["x"], o["w"], o["b"], o["dy"]
    pre = x @ w.t() + b
    y_exact = E.relu(pre) if c.relu else pre
    y = y_exact.float() if c.out_f32 else E.to_half(y_exact)
    if c.relu:
        mask = (y >= 0) if mutant == "mask_ge" else (y > 0)
        dyh = dy * mask + 0.0
    else:
        dyh = dy
    dx_exact = dyh @ w + 0.0
    if mutant == "bias_on_dx":
        dx_exact = dx_exact + o["bk"]
    dx = E.to_half(dx_exact)
    if mutant == "tail_row_zeroed":
        dx[c.M - 1] = 0.0
    dw_exact = dyh.t() @ x + 0.0
    if mutant == "pad_rows_counted":                                 # every padded row holds one grid step of dy and of x
        dw_exact = dw_exact + c.pad * o["ud"] * o["ux"]
    db_exact = dyh.sum(0) + 0.0
    exact = {"y": y_exact, "dx": dx_exact, "dw": dw_exact, "db": db_exact, "dyh": dyh}
    return exact, {"y": y, "dx": dx, "dw": dw_exact.float(), "db": db_exact.float()}


@functools.lru_cache(maxsize=None)
def linear_clean(c):
    """(operands, expected outputs) of a case, computed once per process and never modified."""
    o = linear_operands(c)
    return o, linear_stages(c, o)[1]


def linear_conditions(c):
    """conv_exact.check_point at every accumulation and rounding point of the case: y, dX, dW, db."""
    o, _ = linear_clean(c)
    exact, _ = linear_stages(c, o)
    a = {k: o[k].abs() for k in ("x", "w", "b")}
    dyh = exact["dyh"].abs()
    return [E.check_point(f"{c.name}.y", exact["y"], a["x"] @ a["w"].t() + a["b"], o["ux"] * o["uw"], fp16_point=not c.out_f32),
            E.check_point(f"{c.name}.dx", exact["dx"], dyh @ a["w"], o["ud"] * o["uw"], fp16_point=True),
            E.check_point(f"{c.name}.dw", exact["dw"], dyh.t() @ a["x"], o["ud"] * o["ux"], fp16_point=False),
            E.check_point(f"{c.name}.db", exact["db"], dyh.sum(0), o["ud"], fp16_point=False)]


# ------------------------------------------------------------------------------------------------ a small box-head batch
def box_batch(R=96, C=64, K=3, seed=11):
    """Frozen ROI features [R,7,7,C] fp16, proposals, ground-truth boxes [R,4] and classes [R] in [0, K] (K = background), on the host."""
    g = torch.Generator().manual_seed(seed)
    pooled = (torch.randn(R, 7, 7, C, generator=g).relu() / 2).half()
    xy = torch.rand(R, 2, generator=g) * 300
    prop = torch.cat([xy, xy + 20 + torch.rand(R, 2, generator=g) * 100], 1)
    gt = prop + torch.randn(R, 4, generator=g) * 4
    gt[:, 2:] = torch.maximum(gt[:, 2:], gt[:, :2] + 1)
    cls = torch.randint(0, K + 1, (R,), generator=g)
    return pooled, prop, gt, cls


def clip_rounding_margin(n, p_norm, lr, clip):
    """Relative error of the measured ||dp||_2 of a clipped tensor of n elements against lr * clip, from the roundings alone: an fp32
    tree-reduced norm (ceil(log2 n) levels), the coefficient narrowed to fp32, g * coef and g * grad_scale one rounding each (lr and
    the loss scale are powers of two), and the subtraction p - lr m, whose rounding is relative to p: at most U ||p||_2 in norm."""
    return (math.ceil(math.log2(max(n, 2))) + 3) * U + U * p_norm / (lr * clip)
