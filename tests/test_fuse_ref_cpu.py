"""tests/fuse_ref.py against tests/golden/fuse_ref_parent.npz: what the four restatements it replaced returned on the clusters of
tests/golden/gen_fuse_ref_parent.py (which describes them and rebuilds the inputs), and the restatement's own checks on a hand-made
cluster and of its associativity.  No GPU, no library."""
import importlib.util
import os

import numpy as np
import pytest

from fuse_ref import LD, clusters, log_softmax, restate, ulp32

EPS = 2.0 ** -63


def _generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_fuse_ref_parent.py")
    spec = importlib.util.spec_from_file_location("gen_fuse_ref_parent", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def golden(golden_dir):
    if np.finfo(np.longdouble).eps != EPS:
        pytest.skip("np.longdouble is not the 64-bit-significand format the file was recorded in")
    z = np.load(os.path.join(golden_dir, "fuse_ref_parent.npz"))
    return {k: z[k] for k in z.files}


def _same(got, hi, lo):
    """Equal by value, NaN where the file has NaN (never by bytes: a longdouble carries padding)."""
    got, want = np.asarray(got, LD), GEN.join(hi, lo)
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all() and (got[~nan] == want[~nan]).all())


def test_restate_equals_the_parent_copies(golden):
    """Per cluster and parent copy that applies: lq, score, class, fused box, fused variance, pattern and the NaN flag equal by value
    (logp, posterior, presence); the score within 2 (K + 1) longdouble epsilons relative of pooled_posterior's, which normalised with
    NumPy's blocked sum where the rule - and fuse_ref - add in sequence; every bound at most the parent's for the same options times
    (1 + 2^-40), the float64 rounding of one formula written in two orders."""
    g = golden
    slack = 1.0 + 2.0 ** -40
    at = 0
    applied = {}
    worst_gap = 0.0
    for i, c in enumerate(GEN.cases()):
        k1 = c["lp"].shape[1]
        col = slice(at, at + k1)
        at += k1
        r = restate(c["lp"], c["members"], boxes=c["boxes"], scores=c["scores"], var=c["var"], box=c["box"], src=c["src"], weights=c["weights"],
                    table=c["table"], log_prior=c["log_prior"])
        which = GEN.copies(c)
        for name in which:
            applied[name] = applied.get(name, 0) + 1
        assert r["m"] == len(c["members"])
        assert _same(r["lq"], g["lq_hi"][col], g["lq_lo"][col]), (i, which)
        assert _same(r["box"], g["box_hi"][i], g["box_lo"][i]) and _same(r["var"], g["var_hi"][i], g["var_lo"][i]), (i, which)
        assert (r["lq_bound"] <= g["lq_bound"][col] * slack).all(), (i, which)
        if "presence" in which:
            assert r["pattern"] == g["pattern"][i] and int(r["nan"]) == g["nan"][i] and r["cls"] == g["cls"][i], (i, r["pattern"], r["nan"])
            assert _same(r["score"], g["score_hi"][i], g["score_lo"][i]) and r["score_bound"] <= g["score_bound"][i] * slack, i
        else:
            assert "pattern" not in r and "nan" not in r
        if "logp" in which:
            assert _same(r["score"], g["logp_hi"][i], g["logp_lo"][i]) and r["cls"] == g["logp_cls"][i], i
            assert r["score_bound"] <= g["logp_bound"][i] * slack, i
        if "pool" in which:
            want = GEN.join(g["pool_hi"][i], g["pool_lo"][i])
            gap = float(abs(LD(r["score"]) - want) / want) / EPS
            worst_gap = max(worst_gap, gap)
            assert gap <= 2 * k1 and r["cls"] == g["pool_cls"][i], (i, gap)
            assert r["score_bound"] <= g["pool_bound"][i] * slack, i
    assert at == len(g["lq_hi"]) and all(applied.get(k, 0) >= 20 for k in ("logp", "posterior", "presence", "pool")), applied
    print(f"{applied}; largest gap to pooled_posterior {worst_gap:.1f} longdouble eps (allowed 2 (K + 1))")


def test_helpers_equal_the_parent_copies(golden):
    g = golden
    got = [clusters(*im) for im in GEN.cluster_images()]
    assert [len(c) for c in got] == g["clusters_per_image"].tolist()
    assert [p for c in got for p, _ in c] == g["clusters_pivots"].tolist()
    assert [len(m) for c in got for _, m in c] == g["clusters_sizes"].tolist()
    assert [t for c in got for _, m in c for t in m] == g["clusters_members"].tolist()
    assert np.array_equal(ulp32(GEN.ULP_IN), g["ulp32"]) and ulp32(0.3) == g["ulp32"][8]
    assert np.array_equal(np.concatenate([log_softmax(x).reshape(-1) for x in GEN.softmax_in()]), g["log_softmax"])


def test_restatement_on_a_hand_made_cluster():
    """The rule on numbers small enough to check by hand: a lone row takes lp + presence[1 << source] and may turn into background;
    a cluster of two takes the product and the 'both' row; a bad source gives NaN and adds no bit."""
    lp = np.log(np.array([[0.6, 0.4], [0.7, 0.3], [0.5, 0.5]]))
    kw = dict(boxes=np.zeros((3, 4)), scores=np.array([0.6, 0.7, 0.5]), var=np.ones(3), box="v-avg", src=np.array([0, 1, 2], np.int32),
              table=np.array([[0.0, 0.0], [-1.0, 0.0], [0.5, 0.0], [2.0, 0.0]]))
    lone = restate(lp, [0], **kw)
    want = np.array([0.6 * np.exp(-1.0), 0.4])
    assert lone["pattern"] == 1 and lone["cls"] == 1 and abs(float(lone["score"]) - want[1] / want.sum()) < 1e-15
    pair = restate(lp, [0, 1], **kw)
    want = np.array([0.6 * 0.7 * np.exp(2.0), 0.4 * 0.3])
    assert pair["pattern"] == 3 and pair["cls"] == 0 and abs(float(pair["score"]) - want[0] / want.sum()) < 1e-15
    assert abs(float(np.exp(pair["lq"]).sum()) - 1.0) < 1e-15
    bad = restate(lp, [0, 2], **kw)
    assert bad["nan"] and bad["pattern"] == 1 and bad["cls"] == 0 and np.isnan(bad["score"])
    assert restate(lp, [2], **kw)["pattern"] == 0


@pytest.mark.parametrize("with_prior", [False, True])
def test_restatement_is_associative(with_prior):
    """((A, B), C) against (A, B, C) through `restate` alone, in longdouble: v-avg boxes, variances and posteriors.  In exact arithmetic
    they are the same numbers - 1 / sum(1 / var) is the value that makes the inverse-variance mean associative, and (1 + 1) prior
    terms are the (3 - 1) of the direct fusion -, so what is left is longdouble rounding: relative, a few eps on boxes and variances
    (tolerated: 32 eps); absolute on the log-posteriors, whose sums reach magnitudes up to 2^7, where one rounding is up to 64 eps and
    each route rounds a handful of times (tolerated: 512 eps)."""
    rng = np.random.default_rng(17)
    eps = float(np.finfo(LD).eps)
    prior = np.log(np.array([0.1, 0.4, 0.2, 0.3])) if with_prior else None
    worst = {"lq": 0.0, "box": 0.0, "var": 0.0}
    for _ in range(200):
        lg = rng.normal(0, 6, (3, 4))
        lp = lg - lg.max(1, keepdims=True)
        lp = lp - np.log(np.exp(lp).sum(1, keepdims=True))
        boxes = np.array([100.0, 80.0, 160.0, 160.0]) + rng.uniform(-2, 2, (3, 4))
        var = rng.uniform(0.5, 4.0, 3)
        kw = dict(boxes=boxes, scores=np.exp(lp.max(1)), var=var, box="v-avg", log_prior=prior)
        three, two = restate(lp, [0, 1, 2], **kw), restate(lp, [0, 1], **kw)
        lq3, b3, v3 = three["lq"], three["box"], three["var"]
        lq1, b1, v1 = two["lq"], two["box"], two["var"]
        # stage two in longdouble on stage one's longdouble results
        a = lq1 + lp[2].astype(LD) - (prior.astype(LD) if with_prior else 0)
        a = a - a.max()
        lq2 = a - np.log(np.exp(a).sum())
        g = np.array([1 / v1, 1 / LD(var[2])])
        v2 = 1 / g.sum()
        b2 = (b1 * g[0] + boxes[2].astype(LD) * g[1]) / g.sum()
        worst["lq"] = max(worst["lq"], float(np.abs(lq2 - lq3).max()))
        worst["box"] = max(worst["box"], float((np.abs(b2 - b3) / np.abs(b3)).max()))
        worst["var"] = max(worst["var"], float(abs(v2 - v3) / v3))
    print(f"prior {with_prior}: largest differences in longdouble eps: lq {worst['lq'] / eps:.1f} (absolute), box {worst['box'] / eps:.1f}, "
          f"variance {worst['var'] / eps:.1f} (relative)")
    assert worst["box"] <= 32 * eps and worst["var"] <= 32 * eps and worst["lq"] <= 512 * eps
