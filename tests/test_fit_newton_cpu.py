"""calibration._projected_newton behind fit_pool_weights and fit_presence: its iterates are those of the two loops it replaced
(tests/frozen_newton.py), bit for bit.  No GPU: calibration.pool_nll and calibration.bias_nll are replaced by the NumPy restatements of
tests/test_pool_cpu.py and tests/test_presence_cpu.py, the same evaluator drives the frozen loop and the new code in one process, and
every candidate matrix the evaluator receives and every entry of the returned record must agree by tobytes() - so neither libm's exp
nor LAPACK's solve can make the comparison depend on the machine.

The cases are small (at most 300 clusters, D <= 4, K + 1 <= 4) and together reach every branch of the loop; the frozen loops count
the branches, and a case that no longer reaches the branch it is named for fails."""
import collections

import numpy as np
import pytest
import torch

import frozen_newton
from fuse_ref import log_softmax
from test_pool_cpu import cluster_tables, nll_grad
from test_presence_cpu import np_bias_nll


def key(x):
    x = np.ascontiguousarray(np.asarray(x, np.float64))
    return x.shape, x.tobytes()


def canon(x):
    """A result record with every float replaced by its bits, so that == compares bit for bit (and NaN with NaN)."""
    if isinstance(x, dict):
        return {k: canon(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [canon(v) for v in x]
    return ("f64", np.float64(x).tobytes()) if isinstance(x, float) else (type(x).__name__, x)


def same_record(a, b):
    assert canon(a) == canon(b), (a, b)


# ---- pooling weights ------------------------------------------------------------------------------------------------------------------

def pool_case(C, k1, sources, w_true, seed, offset=0.0):
    """C clusters of len(sources) rows; row t of a cluster belongs to detector abs(sources[t]) and a negative entry makes it a COPY of the
    cluster's first row (two identical detectors).  Labels are drawn from the pooled posterior at w_true.  `offset` is added to every
    entry of the tables G: the posterior does not see a shift common to a row's columns, the rounding of the gradient's terms does."""
    rng = np.random.default_rng(seed)
    m, D = len(sources), max(abs(s) for s in sources) + 1
    z = rng.normal(0.0, 2.0, (C, m, k1)).astype(np.float32)
    for t, s in enumerate(sources):
        if s < 0:
            z[:, t] = z[:, 0]
    lp = log_softmax(z.reshape(C * m, k1))
    src = np.tile(np.abs(sources), C).astype(np.int32)
    offs = (np.arange(C + 1) * m).astype(np.int32)
    G, _, _ = cluster_tables(lp, src, np.arange(C * m), offs, D)
    a = np.einsum("d,cdj->cj", np.asarray(w_true, np.float64), G)
    p = np.exp(a - a.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    labels = (rng.random(C)[:, None] > np.cumsum(p, 1)).sum(1).clip(0, k1 - 1).astype(np.int32)
    return G + offset, labels, D


def pool_evaluator(G, labels, seen):
    def pool_nll(*args):
        W = np.asarray(args[-1 if len(args) == 1 else 5], np.float64)
        seen.append(key(W))
        out = [nll_grad(G, labels, w) for w in W]
        return np.asarray([n.sum() for n, _ in out]), np.asarray([g.sum(0) for _, g in out]), 0, -1
    return pool_nll


# Two identical detectors make the Hessian singular, but on their own they do not reach the fallback direction: the ridge
# 1e-10 * trace exceeds the forward differences' rounding (about 1e-11 here), the ridged system is positive definite and its solution
# descends (checked with the frozen loop alone: 0 fallbacks over the seeds 0 to 2).  With the tables shifted by 2^30 the rounding of
# the gradient's terms (2^30 * 2^-53 / h per cluster) exceeds the ridge, the singular direction's eigenvalue comes out with either sign
# and the fallback is taken in 5 of the 7 rounds.
#          name: (clusters, K + 1, sources, w_true, seed, offset, hi, gtol, max_rounds), the branch the case is there for
POOL = {"interior": ((300, 4, (0, 1, 0), (0.7, 0.4), 0, 0.0, 64.0, 1e-7, 60), "converged"),
        "lower_bound": ((200, 3, (0, 1), (0.9, 0.0), 2, 0.0, 64.0, 1e-7, 60), "held"),
        "upper_bound": ((200, 3, (0, 1), (1.6, 0.8), 2, 0.0, 1.25, 1e-7, 60), "held"),
        "identical_detectors": ((200, 4, (0, -1), (0.5, 0.5), 2, 2.0 ** 30, 64.0, 1e-7, 60), "fallback"),
        "no_step_lowers": ((150, 3, (0, 1, 2, 3), (0.8, 0.5, 0.3, 0.6), 4, 0.0, 64.0, 0.0, 60), "no_step"),
        "cut_by_max_rounds": ((150, 4, (0, 1), (2.5, 0.2), 5, 0.0, 64.0, 1e-7, 2), "max_rounds")}


@pytest.mark.parametrize("name", POOL)
def test_fit_pool_weights_takes_the_frozen_loops_steps(monkeypatch, name):
    from proben_amd import calibration
    (C, k1, sources, w_true, seed, offset, hi, gtol, max_rounds), branch = POOL[name]
    G, labels, D = pool_case(C, k1, sources, w_true, seed, offset)
    want_seen, got_seen, hits = [], [], collections.Counter()
    want = frozen_newton.fit_pool_weights(pool_evaluator(G, labels, want_seen), C, D, hi, gtol, max_rounds, hits)
    assert hits[branch] > 0, (name, dict(hits), want)
    if name.endswith("_bound"):
        assert want["at_bound"].count({"lower_bound": "lo", "upper_bound": "hi"}[name]) == 1, want
    monkeypatch.setattr(calibration, "pool_nll", pool_evaluator(G, labels, got_seen))
    got = calibration.fit_pool_weights(None, None, None, None, torch.from_numpy(labels), D, None, hi, gtol, max_rounds)
    assert got_seen == want_seen, (len(got_seen), len(want_seen))
    same_record(got, want)


# ---- presence rows --------------------------------------------------------------------------------------------------------------------

def bias_case(C, k1, seed, shift, absent=None):
    """Fused log-posteriors of C clusters, labels drawn from softmax(base + shift); `absent`: a label that never occurs (its entry of the
    row has its minimum at minus infinity)."""
    rng = np.random.default_rng(seed)
    base = log_softmax(rng.normal(0.0, 1.5, (C, k1)))
    p = np.exp(log_softmax(base + np.asarray(shift)[None, :]))
    if absent is not None:
        p[:, absent] = 0.0
        p /= p.sum(1, keepdims=True)
    labels = (rng.random(C)[:, None] > np.cumsum(p, 1)).sum(1).clip(0, k1 - 1).astype(np.int32)
    return base, labels


def bias_evaluator(seen):
    def bias_nll(base, labels, candidates):
        base, labels = np.asarray(base), np.asarray(labels)
        B = np.asarray(candidates, np.float64)
        seen.append(key(B))
        if len(labels) == 0:
            return np.zeros(len(B)), np.zeros(B.shape), 0, -1
        out = [np_bias_nll(base, labels, b) for b in B]
        return np.asarray([f for f, _, _ in out]), np.asarray([g for _, g, _ in out]), 0, -1
    return bias_nll


#          name: (clusters, K + 1, seed, shift, absent label, hi, gtol, max_rounds), the branch the case is there for
BIAS = {"interior": ((300, 4, 0, (0.8, -0.5, 0.3, 0.0), None, 16.0, 1e-7, 60), "converged"),
        "lower_bound": ((200, 3, 1, (0.2, 0.0, 0.0), 0, 2.0, 1e-7, 60), "held"),
        "upper_bound": ((200, 3, 2, (3.0, 0.0, 0.0), None, 0.5, 1e-7, 60), "held"),
        "no_step_lowers": ((150, 4, 3, (0.4, 0.1, -0.2, 0.0), None, 16.0, 0.0, 60), "no_step"),
        "cut_by_max_rounds": ((150, 2, 4, (4.0, 0.0), None, 16.0, 1e-7, 2), "max_rounds")}


@pytest.mark.parametrize("name", BIAS)
def test_fit_presence_takes_the_frozen_loops_steps(monkeypatch, name):
    """Two detectors, every cluster of pattern 1 or 3 and none of pattern 2: row 2 stays zero, rows 1 and 3 are fitted."""
    from proben_amd import calibration
    (C, k1, seed, shift, absent, hi, gtol, max_rounds), branch = BIAS[name]
    base, labels = bias_case(C, k1, seed, shift, absent)
    patterns = np.where(np.arange(C) % 3 == 0, 3, 1).astype(np.int32)
    want_seen, got_seen, hits = [], [], collections.Counter()
    frozen = bias_evaluator(want_seen)
    want = {"table": np.zeros((4, k1)), "patterns": {}}
    for P in (1, 2, 3):
        sel = patterns == P
        row, want["patterns"][P] = frozen_newton.fit_bias(lambda cand: frozen(base[sel], labels[sel], cand), int(sel.sum()), k1, hi, gtol,
                                                          max_rounds, hits)
        want["table"][P] = row
    assert hits[branch] > 0 and hits["zero_row"] == 1, (name, dict(hits), want)
    if name.endswith("_bound"):
        assert any({"lower_bound": "lo", "upper_bound": "hi"}[name] in r["at_bound"] for r in want["patterns"].values()), want
    monkeypatch.setattr(calibration, "bias_nll", bias_evaluator(got_seen))
    monkeypatch.setattr(calibration._lib, "require_cuda", lambda *tensors: None)
    got = calibration.fit_presence(torch.from_numpy(base), torch.from_numpy(patterns), torch.from_numpy(labels), 2, hi, gtol, max_rounds)
    assert got_seen == want_seen, (len(got_seen), len(want_seen))
    assert got["hi"] == hi and got["unassigned"] == 0 and key(got["table"]) == key(want["table"])
    assert not np.any(want["table"][2]) and want["patterns"][2]["rounds"] == 0 and want["patterns"][2]["converged"]
    same_record(got["patterns"], want["patterns"])
