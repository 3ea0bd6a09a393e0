"""The cluster rule of score_fusion "probEn-log" (include/proben_hip.h) restated once, in np.longdouble, with the error bounds the GPU
tests hold the kernels to: the comparator of tests/test_proben_logp_gpu.py, test_posterior_gpu.py, test_presence_gpu.py and
test_pool_gpu.py.  It is never the code under test.  NumPy only: no torch, no library, no GPU.  tests/test_fuse_ref_cpu.py pins it
to the four restatements it replaced (tests/golden/fuse_ref_parent.npz).  u = 2^-53.

The rule.  A cluster's m rows in cluster order (matches in sorted order, the pivot last), column j of K + 1:
    a_j = sum_t w_t lp_tj - (W - 1) log_prior_j + presence[P]_j,     W = sum_t w_t,
every sum sequential (seq_sum: the kernel's order), w_t = 1 and W = m without pool weights, P = the OR of 1 << source over the
members.  lq = a - max a - log(sum_j exp(a_j - max a)), score = exp(a_best - max a) / tot, class = best = the first maximum.
Without a table a cluster of one row copies its row (zero bounds); with one, a lone row is a_j = lp_j + presence[P]_j, without
weights or prior.  A member whose source is outside [0, D) under a table gives NaN, class 0, and adds no bit to P.

The bounds, first order in u, on the kernel's float64 results against this value (DESIGN.md sections 11, 17, 18 and 26).
Column j of a cluster of m >= 2 rows, A_j u absolute on a_j; a term in [] belongs to the option named:
    (m - 1) S_j                    the sequential sum: m - 1 additions of partial sums <= S_j = sum_t |w_t lp_tj|          always
    [S_j]                          x_t = w_t lp_tj rounds once per product                                                 pool weights
    [((m - 1) W + |c|) |lprior_j|] c = W - 1: W's m - 1 additions and the subtraction (unpooled: c = m - 1 is exact)       pool weights + prior
    [|c lprior_j| + |a'_j|]        the product c lprior_j rounds once, the subtraction once more (a' = the column then)    prior
    [|a_j|]                        the presence entry is an exact input; its addition rounds once                          table
A lone row under a table: one addition of two exact inputs, A_j = |a_j|.
From there alike.  top is one of the a_j; d_j = a_j - top rounds once: D_j = A_j + A_best + |d_j| absolute.  e_j = exp(d_j) within
1 ulp (<= 2 u relative) of the exp of a d_j that is D_j u off: E_j = D_j + 2 relative (the winning column: exp(0) = 1 exactly).
tot adds K roundings of partial sums <= tot to the weighted sum_j s_j E_j: T = sum_j s_j E_j + K relative.
    score = e_best / tot, one division more:   (sum_{j != best} s_j E_j) + K + 1, relative                                 score_bound
    lq_j = d_j - log(tot): T u absolute on log(tot), log's own ulp (2 |log tot| u), the subtraction (|lq_j| u):
      |lq_j - exact| <= (D_j + T + 2 |log tot| + |lq_j|) u, absolute                                                       lq_bound
The float32 exit of the score rounds once more: half an ulp32 of the expected score, which the callers add.
Fused variance and box: var_bound and box_bound below."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble
BOX = ["v-avg", "s-avg", "avg", "argmax"]


def seq_sum(rows):
    acc = np.zeros_like(rows[0])
    for r in rows:
        acc = acc + r
    return acc


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64))
    return np.exp2(np.maximum(np.floor(np.log2(np.maximum(x, 2.0 ** -126))), -126.0) - 23.0)


def log_softmax(z):
    z = np.asarray(z, np.float64)
    d = z - z.max(-1, keepdims=True)
    return d - np.log(np.exp(d).sum(-1, keepdims=True))


def clusters(boxes, scores, classes, thr=0.5):
    """Greedy clustering of demo_probEn.py:92-143 restated: [(pivot row, members in cluster order: matches in sorted order, pivot last)]."""
    from oracle.proben import order_desc
    x1, y1 = boxes[:, 0] + classes * 640.0, boxes[:, 1] + classes * 512.0
    x2, y2 = boxes[:, 2] + classes * 640.0, boxes[:, 3] + classes * 512.0
    area = (x2 - x1 + 1.0) * (y2 - y1 + 1.0)
    order = order_desc(scores)
    alive = np.ones(len(scores), bool)
    out = []
    for pos, i in enumerate(order):
        if not alive[i]:
            continue
        alive[i] = False
        rest = order[pos + 1:]
        rest = rest[alive[rest]]
        w = np.maximum(0.0, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + 1.0)
        h = np.maximum(0.0, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + 1.0)
        inter = w * h
        ovr = inter / (area[i] + area[rest] - inter)
        alive[rest[~(ovr <= thr)]] = False
        out.append((int(i), [int(q) for q in rest[ovr > thr]] + [int(i)]))
    return out


def pattern_of(src, members, D):
    """(P, every source in range): P = OR of (1 << source) over the members whose source is inside [0, D)."""
    ok = [0 <= int(src[t]) < D for t in members]
    return sum({1 << int(src[t]) for t, o in zip(members, ok) if o}), all(ok)


def restate(lp, members, *, boxes=None, scores=None, var=None, box=None, src=None, weights=None, table=None, log_prior=None):
    """The rule above for ONE cluster.  lp f64 [n, K+1]; members = the cluster's rows in cluster order; boxes f64 [n, 4], scores / var
    f64 [n] and box (one of BOX) for the fused box; src i32 [n] with weights (the pool weight PER DETECTOR) or table (f64 [2^D, K+1]);
    log_prior f64 [K+1].  Returns a dict: lq [K+1], score, cls, lq_bound [K+1] (absolute, in units of u), score_bound (relative, in
    units of u), m; with a table pattern and nan (a member's source is out of range); with box, box [4] and var."""
    m = len(members)
    k1 = lp.shape[1]
    out = {"m": m}
    if box is not None:
        b, v, sc = boxes[members].astype(LD), var[members].astype(LD), scores[members].astype(LD)
        if m == 1:
            fbox, fvar = b[0], v[0]
        elif box == "argmax":
            t = int(np.argmax(scores[members]))          # first maximum in cluster order
            fbox, fvar = b[t], v[t]
        else:
            lam = {"v-avg": (1 / v) / (1 / v).sum(), "s-avg": sc / sc.sum(), "avg": np.full(m, LD(1) / m)}[box]
            fvar = 1 / (1 / v).sum() if box == "v-avg" else (lam * lam * v).sum()
            fbox = (lam[:, None] * b).sum(0)
        out.update(box=fbox, var=fvar)
    if table is not None:
        P, ok = pattern_of(src, members, int(table.shape[0]).bit_length() - 1)
        out.update(pattern=P, nan=not ok)
        if not ok:
            out.update(lq=np.full(k1, np.nan), score=np.nan, cls=0, lq_bound=np.zeros(k1), score_bound=0.0)
            return out
        pres = table[P].astype(LD)
    if m == 1:
        a = lp[members[0]].astype(LD)
        if table is None:           # a copy; the kernel's score and class of such a row are the row's own, which the callers compare
            jb = int(np.argmax(a))
            out.update(lq=a, score=np.exp(a[jb]), cls=jb, lq_bound=np.zeros(k1), score_bound=0.0)
            return out
        a = a + pres
        A = np.abs(a.astype(np.float64))
    else:
        x = lp[members].astype(LD)
        pooled = weights is not None
        W = LD(m)
        if pooled:
            w = np.asarray(weights, np.float64)[src[members]].astype(LD)
            x = w[:, None] * x
            W = seq_sum(list(w))
        a = seq_sum(list(x))
        S = np.abs(x.astype(np.float64)).sum(0)
        A = (m - 1) * S + (S if pooled else 0.0)
        if log_prior is not None:
            c = W - LD(1)
            a = a - c * log_prior.astype(LD)
            if pooled:
                A = A + ((m - 1) * float(W) + abs(float(c))) * np.abs(log_prior)
            A = A + np.abs(float(c) * log_prior) + np.abs(a.astype(np.float64))
        if table is not None:
            a = a + pres
            A = A + np.abs(a.astype(np.float64))
    top = a.max()
    jb = int(np.argmax(a))
    d = a - top
    e = np.exp(d)
    tot = seq_sum(list(e))
    lq = d - np.log(tot)
    s = (e / tot).astype(np.float64)
    Dj = A + A[jb] + np.abs(d.astype(np.float64))
    E = Dj + 2.0
    T = float((s * E).sum()) + k1 - 1
    Es = E.copy()
    Es[jb] = 0.0
    out.update(lq=lq, score=(e / tot)[jb], cls=jb, lq_bound=Dj + T + 2.0 * abs(float(np.log(tot))) + np.abs(lq.astype(np.float64)),
               score_bound=float((s * Es).sum()) + k1 - 1 + 1)
    return out


def box_bound(box, m):
    """Bound on a fused coordinate in units of X u, X = sum_t |c_t lambda_t|: the weights carry at most (m + 1) u (v-avg: a reciprocal,
    wsum's m - 1 additions, a division; s-avg and avg less), the product one more, the m - 1 additions of partial sums <= X one each:
    (2 m + 1) X u.  argmax and single rows: a copy."""
    return 0 if (m == 1 or box == "argmax") else 2 * m + 1


def var_bound(box, m):
    """Relative bound on the kernel's fused variance in units of u.  v-avg: m reciprocals (u each), m - 1 additions of positive terms
    ((m - 1) u), one reciprocal: (m + 1) u <= (m + 3) u.  s-avg: lambda = s / wsum carries wsum's (m - 1) u and its own division
    (m u); squared 2 m u + u; times var u: (2 m + 2) u per positive term, m - 1 additions: (3 m + 1) u <= (3 m + 4) u.  avg: lambda =
    1 / m rounds once, so (m + 3) u <= (3 m + 4) u.  argmax and single rows: a copy."""
    return {"v-avg": m + 3, "s-avg": 3 * m + 4, "avg": 3 * m + 4, "argmax": 0}[box] if m > 1 else 0
