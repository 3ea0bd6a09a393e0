"""The dense NumPy float64 restatement of the PDQ rule (include/proben_hip.h) for tests/test_pdq_{cpu,gpu}.py.  There is
no published implementation to compare with offline: the rule's text is the specification and this file restates it, pixel by pixel - the
full P and Q arrays of a detection, masks for the ground truth and for the support, math.fsum for every sum.  Nothing of the kernel's
structure is here: no tables kept, no window, no B_all - B_in (the background sum runs over {P > tau} minus the ground truth itself).

    detection(box, var, H, W)      P, Q [H, W], or None for an excluded detection
    gt_pixels(box, H, W)           the boolean mask S_g [H, W]
    pair(P, Q, S, tau)             FG, BG and, for the bound, (sum |terms|, n) of the sums F, B_all and B_in the kernel forms
    pair_quality(images, K, tau)   per image q, fg, bg, label [G_b, M_b], gt_live, the flags and the bound of each of the four outputs
    pdq(images, K, tau, thresh)    the reference pipeline: pair_quality + scipy.optimize.linear_sum_assignment -> per-image records

An image is a dict: H, W, det_boxes [M, 4], det_vars [M], det_lp [M, K + 1], gt_boxes [G, 4], gt_classes [G], gt_crowd [G] (and "scores"
[M] for pdq).  One deviation from the rule's letter, the kernel's too (section 30): log max(P, eps) is taken as log1p(-Q) where P > 0.5, and
log max(Q, eps) as log1p(-P) where Q > 0.5 - the same numbers, without the cancellation of a logarithm near 1.
"""
import math

import numpy as np
from scipy.special import erfc

U = 2.0 ** -53
EPS = 1e-14
SQRT2 = 1.4142135623730951
# The per-term error allowance of the bound in units of U (erfc, the products, log): TWICE the largest error of a term of the kernel against
# 50-digit arithmetic, MEASURED on an MI355X over the arguments of the GPU tests' own cases: 1626.229 (DESIGN.md section 30;
# tests/test_pdq_gpu.py measures it again and holds it to half of this).  The figure is that large because of terms nobody sees: deep in a
# tail erfc(x) carries a relative error of about x^2 U (the rounding of x^2 inside exp(-x^2)), and a term such as log1p(-Q) = -Q with Q of
# 1e-287 inherits it.  The differences the tests observe would pass c = 16.
C_TERM = 3252.5


def Phi(z):
    return 0.5 * erfc(-z / SQRT2)


def Phic(z):
    return 0.5 * erfc(z / SQRT2)


def axis_arguments(lo, hi, s, n):
    """a, b of the rule for the n pixel centres of an axis (s > 0)."""
    i = np.arange(n, dtype=np.float64)
    return ((i + 0.5) - lo) / s, ((hi - i) - 0.5) / s


def axis(lo, hi, s, n):
    """p, q [n] of the rule for one axis."""
    if s == 0.0:
        c = np.arange(n, dtype=np.float64) + 0.5
        p = ((lo <= c) & (c <= hi)).astype(np.float64)
        return p, 1.0 - p
    a, b = axis_arguments(lo, hi, s, n)
    pa = Phi(a)
    return pa * Phi(b), Phic(a) + pa * Phic(b)


def sigmas(box, var, weights=(10.0, 10.0, 5.0, 5.0)):
    wx, wy, ww, wh = (float(np.float32(w)) for w in weights)
    sd = np.sqrt(np.float64(var))
    sx = sd * (box[2] - box[0]) * np.sqrt(1.0 / (wx * wx) + 1.0 / (4.0 * (ww * ww)))
    sy = sd * (box[3] - box[1]) * np.sqrt(1.0 / (wy * wy) + 1.0 / (4.0 * (wh * wh)))
    return float(sx), float(sy)


def excluded(box, var):
    box = np.asarray(box, dtype=np.float64)
    return not (np.all(np.isfinite(box)) and box[2] - box[0] > 0 and box[3] - box[1] > 0 and np.isfinite(var) and var >= 0)


def detection(box, var, H, W, weights=(10.0, 10.0, 5.0, 5.0)):
    box = np.asarray(box, dtype=np.float64)
    if excluded(box, var):
        return None
    sx, sy = sigmas(box, var, weights)
    with np.errstate(all="ignore"):
        px, qx = axis(box[0], box[2], sx, W)
        py, qy = axis(box[1], box[3], sy, H)
        P = py[:, None] * px[None, :]
        Q = qx[None, :] + px[None, :] * qy[:, None]
    return P, Q


def gt_pixels(box, H, W):
    cu, cv = np.arange(W) + 0.5, np.arange(H) + 0.5
    return ((box[1] <= cv) & (cv < box[3]))[:, None] & ((box[0] <= cu) & (cu < box[2]))[None, :]


def ignored(box, cls, crowd, H, W, K):
    box = np.asarray(box, dtype=np.float64)
    return bool(crowd) or not np.all(np.isfinite(box)) or not 0 <= cls < K or not gt_pixels(box, H, W).any()


def terms_fg(P, Q):
    with np.errstate(all="ignore"):
        return np.where(P > 0.5, np.log1p(-Q), np.log(np.maximum(P, EPS)))


def terms_bg(P, Q):
    with np.errstate(all="ignore"):
        return np.where(Q > 0.5, np.log1p(-P), np.log(np.maximum(Q, EPS)))


def _sum(t):
    """(fsum, sum |terms|, n) of an array of terms."""
    t = np.asarray(t, dtype=np.float64).ravel()
    return math.fsum(t), math.fsum(np.abs(t)), t.size


def sum_bound(abs_sum, n, c=C_TERM):
    """What a sum of n terms in any order may differ from their fsum by: (c + ceil(log2 n)) U sum |terms|."""
    return 0.0 if n == 0 else (c + math.ceil(math.log2(n)) if n > 1 else c) * U * abs_sum


def pair(P, Q, S, tau):
    n_g = int(S.sum())
    supp = P > tau
    F, aF, nF = _sum(terms_fg(P[S], Q[S]))
    Bo, _, _ = _sum(terms_bg(P[supp & ~S], Q[supp & ~S]))          # the rule's own background sum
    _, aAll, nAll = _sum(terms_bg(P[supp], Q[supp]))              # the two sums the kernel forms it from
    _, aIn, nIn = _sum(terms_bg(P[supp & S], Q[supp & S]))
    return {"FG": F / n_g, "BG": Bo / n_g, "n_g": n_g, "eF": sum_bound(aF, nF), "eB": sum_bound(aAll, nAll) + sum_bound(aIn, nIn)}


def output_bounds(r, QL):
    """The bound carried to fg = exp(FG), bg = exp(BG), label = Q_L and q = sqrt(exp(FG + BG) Q_L), to first order: the sums' bounds
    through / n_g, then 2 U of its own for each of the division (and the subtraction), exp, the product and sqrt."""
    eFG = r["eF"] / r["n_g"] + 2 * U * abs(r["FG"])
    eBG = r["eB"] / r["n_g"] + 2 * U * abs(r["BG"])
    fg, bg = math.exp(r["FG"]), math.exp(r["BG"])
    rel_qs = eFG + eBG + 2 * U * abs(r["FG"] + r["BG"]) + 2 * U                # FG + BG, exp
    rel_q = 0.5 * (rel_qs + 2 * U + 2 * U) + 2 * U                              # Q_L's exp, the product; sqrt halves, and rounds
    q = math.sqrt(math.exp(r["FG"] + r["BG"]) * QL)
    return {"fg": fg * (eFG + 2 * U), "bg": bg * (eBG + 2 * U), "label": QL * 2 * U, "q": q * rel_q}


def pair_quality(images, K, tau=0.0027, weights=(10.0, 10.0, 5.0, 5.0)):
    """Per image: {"q", "fg", "bg", "label"} f64 [G_b, M_b], {"bound": the same four}, "gt_live" [G_b]; and the flags
    [excluded detections, 1 + the last of them, ignored ground truths, 1 + the last] over the flat indices."""
    out, flags, d_base, g_base = [], [0, 0, 0, 0], 0, 0
    for im in images:
        H, W = im["H"], im["W"]
        M, G = len(im["det_vars"]), len(im["gt_classes"])
        res = {k: np.zeros((G, M)) for k in ("q", "fg", "bg", "label")}
        res["bound"] = {k: np.zeros((G, M)) for k in ("q", "fg", "bg", "label")}
        live = np.zeros(G, dtype=np.int32)
        masks = []
        for g in range(G):
            dead = ignored(im["gt_boxes"][g], im["gt_classes"][g], im["gt_crowd"][g], H, W, K)
            live[g] = 0 if dead else 1
            masks.append(None if dead else gt_pixels(np.asarray(im["gt_boxes"][g], dtype=np.float64), H, W))
            if dead:
                flags[2] += 1
                flags[3] = max(flags[3], g_base + g + 1)
        for d in range(M):
            PQ = detection(im["det_boxes"][d], im["det_vars"][d], H, W, weights)
            if PQ is None:
                flags[0] += 1
                flags[1] = max(flags[1], d_base + d + 1)
                continue
            for g in range(G):
                if masks[g] is None:
                    continue
                r = pair(PQ[0], PQ[1], masks[g], tau)
                QL = math.exp(float(im["det_lp"][d][im["gt_classes"][g]]))
                res["fg"][g, d], res["bg"][g, d], res["label"][g, d] = math.exp(r["FG"]), math.exp(r["BG"]), QL
                res["q"][g, d] = math.sqrt(math.exp(r["FG"] + r["BG"]) * QL)
                for k, v in output_bounds(r, QL).items():
                    res["bound"][k][g, d] = v
        res["gt_live"] = live
        out.append(res)
        d_base += M
        g_base += G
    return out, flags


def assign(q, live, take):
    """scipy's optimal assignment over the live rows and the taken columns of q [G, M]: match [G] (column or -1; a pair at q = 0 is none)."""
    from scipy.optimize import linear_sum_assignment
    match = np.full(q.shape[0], -1, dtype=np.int64)
    rows, cols = np.nonzero(live)[0], np.nonzero(take)[0]
    if len(rows) and len(cols):
        sub = q[np.ix_(rows, cols)]
        ri, ci = linear_sum_assignment(sub, maximize=True)
        for r, c in zip(ri, ci):
            if sub[r, c] > 0:
                match[rows[r]] = cols[c]
    return match


def pdq(images, K, tau=0.0027, thresh=0.5, weights=(10.0, 10.0, 5.0, 5.0)):
    """Per-image records [N, 8] (sum q, TP, FP, FN, sum Q_S, sum Q_L, sum exp FG, sum exp BG), the bound of each column summed over the
    matched pairs [8] (0 for the counts; Q_S = exp FG * exp BG to first order: fg e_bg + bg e_fg, and 2 U for the product), and PDQ."""
    res, _ = pair_quality(images, K, tau, weights)
    rec, bound = np.zeros((len(images), 8)), np.zeros(8)
    for i, (im, r) in enumerate(zip(images, res)):
        take = np.asarray(im["scores"]) >= thresh
        m = assign(r["q"], r["gt_live"], take)
        for g in np.nonzero(m >= 0)[0]:
            d = m[g]
            fg, bg, e = r["fg"][g, d], r["bg"][g, d], {k: r["bound"][k][g, d] for k in ("q", "fg", "bg", "label")}
            rec[i] += [r["q"][g, d], 1, 0, 0, fg * bg, r["label"][g, d], fg, bg]
            bound += [e["q"], 0, 0, 0, fg * e["bg"] + bg * e["fg"] + 2 * U * fg * bg, e["label"], e["fg"], e["bg"]]
        rec[i, 2] = take.sum() - rec[i, 1]
        rec[i, 3] = r["gt_live"].sum() - rec[i, 1]
    n = rec[:, 1:4].sum()
    return rec, bound, (rec[:, 0].sum() / n if n else float("nan"))
