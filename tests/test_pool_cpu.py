"""Pooling weights of score_fusion "probEn-log" without a GPU: the NumPy restatement of the NLL / gradient (shared with
tests/test_pool_gpu.py; the pooled rule itself is restated in tests/fuse_ref.py), its own recovery of known weights, weight parsing,
the calibration file, and the argument checks of the new entry points."""
import ctypes
import json

import numpy as np
import pytest

from fuse_ref import log_softmax, restate


# ---- the restatement of the fit --------------------------------------------------------------------------------------------------------

def cluster_tables(log_probs, row_source, member_rows, cluster_offsets, D, log_prior=None, dtype=np.float64):
    """G [C, D, K+1] = S_dj - n_d lp_j, n [C, D], rows per cluster [C]; every cluster's rows in member order."""
    C = len(cluster_offsets) - 1
    k1 = log_probs.shape[1]
    size = np.diff(cluster_offsets)
    cid = np.repeat(np.arange(C), size)
    G = np.zeros((C, D, k1), dtype)
    n = np.zeros((C, D), np.int64)
    src = row_source[member_rows]
    np.add.at(G, (cid, src), log_probs[member_rows].astype(dtype))
    np.add.at(n, (cid, src), 1)
    if log_prior is not None:
        G = G - n[:, :, None].astype(dtype) * log_prior.astype(dtype)[None, None, :]
    return G, n, size


def nll_grad(G, labels, w, log_prior=None, hessian=False):
    """Per-cluster NLL [C] and gradient [C, D] of the pooled posterior at w from the tables (the dtype of G), and optionally the summed
    Hessian [D, D] = sum_c Cov_s(G_d, G_e)."""
    dt = G.dtype
    a = np.einsum("d,cdj->cj", np.asarray(w, dt), G)
    if log_prior is not None:
        a = a + log_prior.astype(dt)[None, :]
    top = a.max(1, keepdims=True)
    e = np.exp(a - top)
    tot = e.sum(1, keepdims=True)
    s = e / tot
    idx = np.arange(len(labels))
    nll = np.log(tot[:, 0]) - (a[idx, labels] - top[:, 0])
    mean = np.einsum("cj,cdj->cd", s, G)
    grad = mean - G[idx, :, labels]
    if not hessian:
        return nll, grad
    H = np.einsum("cj,cdj,cej->de", s, G, G) - np.einsum("cd,ce->de", mean, mean)
    return nll, grad, H


def fit_newton(G, labels, D, rounds=100):
    """Damped Newton on the restatement (float64): halve the step until the NLL falls; clip at 0."""
    w = np.ones(D)
    for _ in range(rounds):
        nll, g, H = nll_grad(G, labels, w, hessian=True)
        f, g = nll.sum(), g.sum(0)
        if np.max(np.abs(g)) <= 1e-9 * len(labels):
            break
        p = -np.linalg.solve(H + 1e-12 * np.trace(H) * np.eye(D), g)
        t = 1.0
        while t > 1e-12:
            cand = np.clip(w + t * p, 0.0, None)
            if nll_grad(G, labels, cand)[0].sum() < f:
                break
            t *= 0.5
        else:
            break
        w = cand
    return w


def recovery_case(seed, C=20000, k1=4, w_true=(0.7, 0.4)):
    """The issue's recovery case: clusters of 2 or 3 rows with sources (0, 1) / (0, 1, 0), logits N(0, 2^2) rounded through float32,
    labels drawn from the pooled posterior at w_true.  Returns flat arrays in pe_pool_nll's layout."""
    rng = np.random.default_rng(seed)
    size = rng.integers(2, 4, C)
    offs = np.concatenate([[0], np.cumsum(size)]).astype(np.int32)
    N = int(offs[-1])
    lp = log_softmax(rng.normal(0.0, 2.0, (N, k1)).astype(np.float32))
    pos = np.arange(N) - np.repeat(offs[:-1], size)
    src = (pos % 2).astype(np.int32)                     # 0, 1, 0
    members = np.arange(N, dtype=np.int32)
    G, _, _ = cluster_tables(lp, src, members, offs, 2)
    a = np.einsum("d,cdj->cj", np.asarray(w_true), G)
    p = np.exp(a - a.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    labels = (rng.random(C)[:, None] > np.cumsum(p, 1)).sum(1).clip(0, k1 - 1).astype(np.int32)
    return {"log_probs": lp, "row_source": src, "member_rows": members, "cluster_offsets": offs, "labels": labels, "G": G,
            "w_true": np.asarray(w_true)}


def dependence_case(seed, C=20000, k1=4):
    """The issue's dependence case: detector 0 has logits z0 ~ N(0, 2^2), every other row of the cluster is z0 + N(0, 1); labels are
    drawn from softmax(z0).  Clusters of 2 or 3 rows, sources (0, 1) / (0, 1, 0) as in the recovery case."""
    rng = np.random.default_rng(1000 + seed)
    size = rng.integers(2, 4, C)
    offs = np.concatenate([[0], np.cumsum(size)]).astype(np.int32)
    N = int(offs[-1])
    pos = np.arange(N) - np.repeat(offs[:-1], size)
    z0 = rng.normal(0.0, 2.0, (C, k1))
    z = np.repeat(z0, size, axis=0) + np.where(pos[:, None] > 0, rng.normal(0.0, 1.0, (N, k1)), 0.0)
    lp = log_softmax(z.astype(np.float32))
    src = (pos % 2).astype(np.int32)                     # 0, 1, 0: the third row is a noisy row of detector 0
    p = np.exp(log_softmax(z0))
    labels = (rng.random(C)[:, None] > np.cumsum(p, 1)).sum(1).clip(0, k1 - 1).astype(np.int32)
    return {"log_probs": lp, "row_source": src, "member_rows": np.arange(N, dtype=np.int32), "cluster_offsets": offs, "labels": labels}


def standard_errors(G, labels, w):
    _, _, H = nll_grad(G, labels, w, hessian=True)
    return np.sqrt(np.diag(np.linalg.inv(H)))


# ---- tests ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_recovers_the_weights(seed):
    """20 000 clusters, K + 1 = 4, labels from the pooled posterior at w = (0.7, 0.4): the restatement's own fit is within 4 standard
    errors (inverse Hessian at the truth) of the truth."""
    case = recovery_case(seed)
    w_hat = fit_newton(case["G"], case["labels"], 2)
    se = standard_errors(case["G"], case["labels"], case["w_true"])
    z = (w_hat - case["w_true"]) / se
    print(f"seed {seed}: w_hat {w_hat}, se {se}, z {z}")
    assert (np.abs(z) <= 4).all(), (w_hat, se)
    assert (se < 0.02).all()


def np_ece(p, labels, bins=15):
    """ECE of the top label (first index among equal maxima) over `bins` bins of equal width on [0, 1]."""
    top = p.argmax(1)
    conf, hit = p[np.arange(len(p)), top], top == labels
    b = np.minimum((conf * bins).astype(int), bins - 1)
    return sum(abs(hit[b == i].mean() - conf[b == i].mean()) * (b == i).sum() for i in range(bins) if (b == i).any()) / len(p)


def test_restatement_on_dependent_detectors():
    """Detector 1 a noisy copy of detector 0, labels from softmax(z0): the restatement's fit on 20 000 clusters lowers the NLL per
    cluster and the ECE (15 bins, top label) of 20 000 held-out ones, and every fitted weight is below 1.  Prints the figures that
    DESIGN.md section 15 quotes."""
    fit, held = dependence_case(0), dependence_case(1)
    G, _, _ = cluster_tables(fit["log_probs"], fit["row_source"], fit["member_rows"], fit["cluster_offsets"], 2)
    w = fit_newton(G, fit["labels"], 2)
    H, _, _ = cluster_tables(held["log_probs"], held["row_source"], held["member_rows"], held["cluster_offsets"], 2)
    out = []
    for ww in (np.ones(2), w):
        a = np.einsum("d,cdj->cj", ww, H)
        p = np.exp(a - a.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        out.append((nll_grad(H, held["labels"], ww)[0].mean(), np_ece(p, held["labels"])))
    print(f"fitted weights {w}; held-out NLL per cluster {out[0][0]:.4f} -> {out[1][0]:.4f}; ECE {out[0][1]:.4f} -> {out[1][1]:.4f}")
    assert out[1][0] < out[0][0] and out[1][1] < out[0][1] and (w < 1).all()


def test_weights_of_one_are_the_plain_rule():
    """fuse_ref.restate with a pool weight of 1.0 gives the unpooled columns value for value: sum_t lp_t - (m - 1) log_prior."""
    rng = np.random.default_rng(3)
    lp = log_softmax(rng.normal(0, 3, (5, 4)))
    prior = np.log(np.array([0.1, 0.2, 0.3, 0.4]))
    pooled = restate(lp, list(range(5)), src=np.zeros(5, np.int32), weights=[1.0], log_prior=prior)
    plain = restate(lp, list(range(5)), log_prior=prior)
    assert (pooled["lq"] == plain["lq"]).all() and pooled["score"] == plain["score"] and pooled["cls"] == plain["cls"]
    acc = np.zeros(4)
    for r in lp:
        acc = acc + r
    assert np.abs(plain["lq"].astype(np.float64) - log_softmax(acc - 4.0 * prior)).max() <= 1e-12


def test_parse_and_resolve():
    from proben_amd import calibration as C
    names = ["thermal_only", "early_fusion"]
    assert C.parse_pool_weights("0.6,0.5", names) == [0.6, 0.5]
    assert C.parse_pool_weights("early_fusion=0.5,thermal_only=0.6", names) == [0.6, 0.5]
    assert C.parse_pool_weights("0,1", names) == [0.0, 1.0]
    assert C.resolve_pool_weights({"thermal_only": 0.25, "early_fusion": 1, "x": 3}, names, "file") == [0.25, 1.0]
    for bad, msg in (("0.6", "lists 1 values for 2"), ("0.6,early_fusion=1", "mixes"), ("a=1,a=2", "twice"), ("thermal_only=1", "no pool weight for early_fusion"),
                     ("nan,1", "not finite and >= 0"), ("-0.1,1", "not finite and >= 0"), ("inf,1", "not finite"), ("0,0", "all 0"), ("x,1", "not a number")):
        with pytest.raises(ValueError, match=msg):
            C.parse_pool_weights(bad, names)
    with pytest.raises(ValueError, match="3 pool weights for 2 detectors"):
        C.check_pool_weights([1, 1, 1], 2, "fusion")
    assert C.check_pool_weights(None, 2, "fusion") is None


def test_calibration_file_round_trip(tmp_path):
    from proben_amd import calibration as C
    p = tmp_path / "c.json"
    C.save(p, {"a": 1.5, "b": 0.7}, pool_weights={"a": 0.6, "b": 0.0})
    rec = C.load(p)
    assert rec["pool_weights"] == {"a": 0.6, "b": 0.0} and rec["detectors"] == {"a": 1.5, "b": 0.7}
    C.save(p, {"a": 1.5, "b": 0.7})
    assert "pool_weights" not in json.load(open(p)) and "pool_weights" not in C.load(p)
    for bad in ({"a": -1.0, "b": 1.0}, {"a": float("nan"), "b": 1.0}, {"a": 0.0, "b": 0.0}, [1.0, 1.0]):
        raw = json.load(open(p))
        raw["pool_weights"] = bad
        q = tmp_path / "bad.json"
        json.dump(raw, open(q, "w"))
        with pytest.raises(ValueError, match="pool"):
            C.load(q)
    with pytest.raises(ValueError, match="not finite and >= 0"):
        C.save(p, {"a": 1.0}, pool_weights={"a": -2})


def test_pool_weights_belong_to_proben_log():
    import torch
    from proben_amd import fusion as F
    z = torch.zeros((0, 4), dtype=torch.float64)
    info = {"img_name": "x", "bbox": [[0, 0, 1, 1]], "score": [0.5], "class": [0], "prob": [[0.5, 0.2, 0.1]], "vars": [[1.0]]}
    for mode in ("probEn", "avg", "max", "probEn_binary"):
        with pytest.raises(ValueError, match="pool_weights belong to score_fusion 'probEn-log'"):
            F.fuse_batch(z, z[:, 0], z[:, :3], z[:, 0], z[:, 0].int(), torch.zeros(1, dtype=torch.int32), score_fusion=mode, pool_weights=[1.0, 1.0])
        with pytest.raises(ValueError, match="pool_weights belong to score_fusion 'probEn-log'"):
            F.fusion([mode, "v-avg"], info, info, pool_weights=[1.0, 1.0])
        with pytest.raises(ValueError, match="pool_weights belong to score_fusion 'probEn-log'"):
            F.fuse_detections([], mode, pool_weights=[1.0, 1.0])
    for bad, msg in (([1.0], "1 pool weights for 2"), ([float("nan"), 1.0], "not finite"), ([-1.0, 1.0], "not finite and >= 0"), ([0.0, 0.0], "all 0")):
        with pytest.raises(ValueError, match=msg):
            F.fusion(["probEn-log", "v-avg"], info, info, pool_weights=bad)


def test_argument_checks_answer_without_a_gpu():
    """pe_proben_fuse_batch_pooled, pe_proben_pack_pooled and pe_pool_nll check their arguments before any device work and explain
    themselves through pe_last_error()."""
    import __graft_entry__ as g
    g.build()
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()  # noqa: E731
    P = 4096      # a non-null pointer that is never dereferenced

    def fuse(row_source=P, weights=P, nd=2, K=3, boxes=P, cluster=None):
        return L.pe_proben_fuse_batch_pooled(boxes, P, P, P, P, row_source, P, None, None, 1, K, 64, 0, 0.5, 640.0, 512.0, None, weights, nd,
                                             P, P, P, P, P, cluster, None)
    assert fuse(boxes=None) == -1 and "pe_proben_fuse_batch_pooled: null input pointer" in err()
    assert fuse(row_source=None) == -1 and "row_source / pool_weights" in err()
    assert fuse(weights=None) == -1 and "row_source / pool_weights" in err()
    assert fuse(nd=0) == -1 and "num_detectors 0 not in [1,8]" in err()
    assert fuse(nd=9) == -1 and "num_detectors 9 not in [1,8]" in err()
    assert fuse(K=63) == -1 and "num_classes 63 not in [1,62]" in err()
    tab = (ctypes.c_void_p * 2)(P, P)
    T = (ctypes.c_double * 2)(1.0, 1.0)

    def pack(out_source=P, logits=tab, temps=T, nd=2):
        return L.pe_proben_pack_pooled(tab, None, tab, None, logits, tab, tab, temps, None, nd, 1, 4, 3, 2, 8, P, P, P, P, P, P, P, P, P, out_source, None)
    assert pack(out_source=None) == -1 and "pe_proben_pack_pooled: null output (out_source)" in err()
    assert pack(temps=None) == -1 and "pe_proben_pack_pooled: null pointer (temperatures" in err()
    assert pack(logits=None) == -1 and "neither probabilities nor logits" in err()
    assert pack(nd=5) == -1 and "num_detectors 5" in err()
    W = (ctypes.c_double * 4)(1.0, 1.0, 0.5, 0.0)

    def nll(w=W, nc=2, nd=2, k1=4, out=P, rows=10, lp=P):
        return L.pe_pool_nll(lp, P, rows, k1, P, 20, P, P, 5, None, w, nc, nd, P, out, P, None)
    assert nll(nc=0) == -1 and "num_candidates 0 not in [1,64]" in err()
    assert nll(nc=65) == -1 and "num_candidates 65" in err()
    assert nll(nd=9) == -1 and "num_detectors 9 not in [1,8]" in err()
    assert nll(w=None) == -1 and "null pointer (weights)" in err()
    assert nll(w=(ctypes.c_double * 4)(1.0, -1.0, 1.0, 1.0)) == -1 and "candidate 0, detector 1) is not finite and >= 0" in err()
    assert nll(w=(ctypes.c_double * 4)(1.0, 1.0, float("nan"), 1.0)) == -1 and "candidate 1, detector 0" in err()
    assert nll(k1=1) == -1 and "num_columns 1" in err()
    assert nll(k1=65) == -1 and "num_columns 65" in err()
    assert nll(out=None) == -1 and "workspace / out / out_flags" in err()
    assert nll(lp=None) == -1 and "log_probs / row_source" in err()
    assert nll(rows=-1) == -1 and "num_rows -1" in err()
