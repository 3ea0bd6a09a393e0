"""Generate tests/golden/fuse_ref_parent.npz: what the four np.longdouble restatements of the probEn-log cluster rule returned at the
commit BEFORE tests/fuse_ref.py replaced them.  tests/test_fuse_ref_cpu.py holds fuse_ref.restate to these values.

    python tests/golden/gen_fuse_ref_parent.py [--out PATH]       at that commit, on the host: no GPU is involved

The parent copies, imported in main() alone (everything above it serves the test too, which rebuilds the inputs by importing this file):
  logp       tests/test_proben_logp_gpu.py::_restate                      score, class, score bound
  posterior  tests/test_posterior_cpu.py::restate                         lq, fused box, fused variance, lq bound
  presence   tests/test_presence_cpu.py::restate                          those, score and its bound, pattern, the NaN flag
  pool       tests/test_pool_cpu.py::pooled_posterior + tests/test_pool_gpu.py::_pooled_bound       score, class, score bound

The clusters (cases()).  N of them from one seed, through rng.uniform / integers / permutation alone - no logarithm, no exponential and no
normal or gamma variate, so every machine draws the same bits: m = 1 .. 9 members picked in random order out of m .. m + 3 rows, K + 1 in
{2, 4, 63}, D = 2 .. 4, the four box rules in turn, prior / pool weights / table each on and off (a pool weight of exactly 0 in every
third pooled case), a member's source set to D or to -1 in every fourth table case, "log-posteriors" -uniform(0, margin) with margin 2,
12 or 40 and the row's own class next to 0 (the rule takes them as given; they need not be normalised).
Which copy applies (copies()): with a table the presence copy; without one the posterior copy, and for m >= 2 the logp copy (unpooled)
or the pool copy (pooled).

The file.  A longdouble x is stored as two float64 arrays, hi = float64(x) and lo = float64(x - hi): exact for a 64-bit significand (and
never as bytes: a longdouble carries padding).  Per-column arrays (lq, its bound) are concatenated over the cases in order.  The helpers:
`clusters` on cluster_images(), `ulp32` on ULP_IN and `log_softmax` on softmax_in(), as the parent's copies gave them (the copies agreed
with each other, asserted here)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LD = np.longdouble
BOX = ["v-avg", "s-avg", "avg", "argmax"]
SEED = 20261020
N = 240
ULP_IN = np.array([0.0, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, -0.75, 0.3, 6e-8, 1e-30, 3.0e38])


def cases():
    rng = np.random.default_rng(SEED)
    out = []
    pooled = tabled = 0
    for i in range(N):
        m = 1 + i % 9
        k1 = 63 if i % 10 == 9 else (2, 4)[(i // 2) % 2]
        D = 2 + (i // 3) % 3
        n = m + int(rng.integers(0, 4))
        margin = (2.0, 12.0, 40.0)[int(rng.integers(0, 3))]
        lp = -rng.uniform(0.0, margin, (n, k1))
        lp[np.arange(n), rng.integers(0, k1, n)] = -rng.uniform(0.0, 2.0 ** -6, n)
        c = {"lp": lp, "members": [int(t) for t in rng.permutation(n)[:m]], "boxes": rng.uniform(0.0, 500.0, (n, 4)),
             "scores": rng.uniform(0.05, 1.0, n), "var": rng.uniform(0.5, 4.0, n), "box": BOX[i % 4], "D": D,
             "src": rng.integers(0, D, n).astype(np.int32), "weights": None, "table": None, "log_prior": None}
        on = rng.integers(0, 2, 3)
        if on[0]:
            c["log_prior"] = -rng.uniform(0.3, 4.0, k1)
        if on[1]:
            c["weights"] = rng.uniform(0.05, 1.5, D)
            if pooled % 3 == 0:
                c["weights"][int(rng.integers(0, D))] = 0.0
            pooled += 1
        if on[2]:
            c["table"] = rng.uniform(-3.0, 3.0, (2 ** D, k1))
            c["table"][:, k1 - 1] = 0.0
            if tabled % 4 == 0:
                c["src"][c["members"][int(rng.integers(0, m))]] = D if tabled % 8 == 0 else -1
            tabled += 1
        out.append(c)
    return out


def copies(c):
    """The parent copies that apply to a case."""
    if c["table"] is not None:
        return ("presence",)
    if len(c["members"]) == 1:
        return ("posterior",)
    return ("posterior", "pool" if c["weights"] is not None else "logp")


def cluster_images():
    """(boxes f64 [n, 4], scores f64 [n], classes f64 [n]) per image: jittered rows on far-apart anchors, three classes, one tied score."""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for n_anchor in (1, 3, 6, 9):
        boxes, cls = [], []
        for a in range(n_anchor):
            x, y = 10.0 + 200.0 * (a % 3), 10.0 + 160.0 * (a // 3)
            k = 1 + int(rng.integers(0, 5))
            boxes.append(np.array([x, y, x + 60.0, y + 50.0]) + rng.uniform(-8.0, 8.0, (k, 4)))
            cls.append(rng.integers(0, 2, k).astype(np.float64))
        boxes, cls = np.concatenate(boxes), np.concatenate(cls)
        scores = rng.uniform(0.05, 1.0, len(cls))
        if len(scores) > 2:
            scores[2] = scores[0]
        out.append((boxes, scores, cls))
    return out


def softmax_in():
    rng = np.random.default_rng(SEED + 2)
    return [rng.uniform(-s, s, (17, k1)) for s, k1 in ((1.0, 2), (12.0, 4), (60.0, 63), (700.0, 4))]


def split(x):
    """longdouble -> (hi, lo) float64 with LD(hi) + LD(lo) == x; a NaN is (NaN, 0)."""
    x = np.asarray(x, LD)
    hi = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        lo = np.where(np.isnan(hi), 0.0, (x - hi.astype(LD)).astype(np.float64))
    return hi, lo


def join(hi, lo):
    return np.asarray(hi, np.float64).astype(LD) + np.asarray(lo, np.float64).astype(LD)


def main():
    assert np.finfo(LD).eps == 2.0 ** -63, "np.longdouble is not the 64-bit-significand format the file is made of"
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import test_pool_cpu as pool_cpu
    import test_pool_gpu as pool_gpu
    import test_posterior_cpu as post_cpu
    import test_posterior_gpu as post_gpu
    import test_presence_cpu as pres_cpu
    import test_presence_gpu as pres_gpu
    import test_proben_logp_gpu as logp
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "fuse_ref_parent.npz")
    cs = cases()
    z = {k: [] for k in ("lq_hi", "lq_lo", "lq_bound")}
    per = {k: np.full(len(cs), np.nan) for k in ("var_hi", "var_lo", "score_hi", "score_lo", "score_bound", "logp_hi", "logp_lo", "logp_bound",
                                                 "pool_hi", "pool_lo", "pool_bound")}
    box_hi, box_lo = np.zeros((len(cs), 4)), np.zeros((len(cs), 4))
    ints = {k: np.full(len(cs), -1, np.int32) for k in ("cls", "pattern", "nan", "logp_cls", "pool_cls")}
    seen = {}
    for i, c in enumerate(cs):
        lp, mem, lprior, w = c["lp"], c["members"], c["log_prior"], c["weights"]
        which = copies(c)
        for name in which:
            seen[name] = seen.get(name, 0) + 1
        if "presence" in which:
            r = pres_cpu.restate(lp, c["boxes"], c["scores"], c["var"], c["src"], mem, c["box"], c["table"], lprior, w)
            lq, fbox, fvar, bound = r["lq"], r["box"], r["var"], r["lq_bound"]
            per["score_hi"][i], per["score_lo"][i] = split(r["score"])
            per["score_bound"][i] = r["score_bound"]
            ints["cls"][i], ints["pattern"][i], ints["nan"][i] = r["cls"], r["pattern"], int(r["nan"])
            seen["nan"] = seen.get("nan", 0) + int(r["nan"])
            assert r["m"] == len(mem)
        else:
            lq, fbox, fvar, bound = post_cpu.restate(lp, c["boxes"], c["scores"], c["var"], mem, c["box"], lprior, None if w is None else w[c["src"]])
        for k, v in zip(("lq_hi", "lq_lo"), split(lq)):
            z[k].append(v)
        z["lq_bound"].append(np.asarray(bound, np.float64))
        box_hi[i], box_lo[i] = split(fbox)
        per["var_hi"][i], per["var_lo"][i] = split(fvar)
        for x in (lq, fbox, fvar):
            x = np.asarray(x, LD)
            ok = ~np.isnan(x)
            assert (join(*split(x))[ok] == x[ok]).all(), "hi + lo does not give the longdouble back"
        if "logp" in which:
            s, j, b = logp._restate(lp, mem, lprior)
            per["logp_hi"][i], per["logp_lo"][i] = split(s)
            per["logp_bound"][i], ints["logp_cls"][i] = b, j
        if "pool" in which:
            w_rows = [w[k] for k in c["src"][mem]]
            sp, a = pool_cpu.pooled_posterior(lp[mem], w_rows, lprior)
            j = int(np.argmax(sp))
            per["pool_hi"][i], per["pool_lo"][i] = split(sp[j])
            per["pool_bound"][i] = pool_gpu._pooled_bound(lp[mem], w_rows, lprior, sp.astype(np.float64), a.astype(np.float64))
            ints["pool_cls"][i] = j
    assert all(seen.get(k, 0) >= 20 for k in ("logp", "posterior", "presence", "pool")) and seen.get("nan", 0) >= 5, seen
    out = {k: np.concatenate(v) for k, v in z.items()}
    out.update(per, box_hi=box_hi, box_lo=box_lo, **ints)
    # the helpers
    cl = [logp._clusters(*im) for im in cluster_images()]
    out["clusters_pivots"] = np.asarray([p for c in cl for p, _ in c], np.int32)
    out["clusters_sizes"] = np.asarray([len(m) for c in cl for _, m in c], np.int32)
    out["clusters_members"] = np.asarray([t for c in cl for _, m in c for t in m], np.int32)
    out["clusters_per_image"] = np.asarray([len(c) for c in cl], np.int32)
    assert out["clusters_sizes"].max() >= 3 and (out["clusters_sizes"] == 1).any()
    ulp = logp._ulp32(ULP_IN)
    for other in (post_gpu._ulp32, pres_gpu._ulp32):
        assert np.array_equal(other(ULP_IN), ulp)
    assert [pool_gpu._ulp32(float(v)) for v in ULP_IN] == ulp.tolist()          # the scalar copy
    out["ulp32"] = ulp
    sm = [pool_cpu.log_softmax64(x) for x in softmax_in()]
    for other in (post_gpu._log_softmax, pres_gpu._log_softmax):
        assert all(np.array_equal(other(x), y) for x, y in zip(softmax_in(), sm))
    out["log_softmax"] = np.concatenate([y.reshape(-1) for y in sm])
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "clusters; copies applied:", seen)


if __name__ == "__main__":
    main()
