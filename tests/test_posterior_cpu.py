"""The fused detection as a full prediction (pe_proben_fuse_batch_posterior, fuse_batch(with_posterior=True), late_fusion.fused_to_j1,
demo_probEn --write_fused, calibration_report --fused-posterior): what can be checked without a GPU, and the np.longdouble restatement
the GPU tests (tests/test_posterior_gpu.py) compare the kernel against.  The comparator is never the code under test.  u = 2^-53."""
import numpy as np
import pytest
import torch

U = 2.0 ** -53
LD = np.longdouble
BOX = ["v-avg", "s-avg", "avg", "argmax"]


def seq_sum(rows):
    acc = np.zeros_like(rows[0])
    for r in rows:
        acc = acc + r
    return acc


def restate(lp, boxes, scores, var, members, box, log_prior=None, weights=None):
    """include/proben_hip.h's formulas for ONE cluster in np.longdouble.  lp f64 [n, K+1], boxes f64 [n, 4], scores / var f64 [n],
    members = the cluster's rows in cluster order (matches in sorted order, pivot last), weights = each ROW's pool weight or None.
    Returns (lq [K+1], fused box [4], fused variance, lq bound [K+1] in units of u, absolute); a cluster of one copies its row.

    The lq bound, first order in u (the derivation of tests/test_proben_logp_gpu.py::_restate carried to lq).
    Column j: x_t = w_t lp_tj rounds once per product when pooled (S_j u, S_j = sum_t |x_t|); the sequential sum is m - 1 additions of
    partial sums <= S_j ((m - 1) S_j u); with a prior the factor c = W - 1 (pooled: W's m - 1 additions, (m - 1) W u, and the
    subtraction, |c| u; unpooled: exact) times log_prior_j rounds once (|c lprior_j| u) and the subtraction once more (|a_j| u):
      A_j = [S_j] + (m - 1) S_j + [((m - 1) W + |c|) |lprior_j|] + [|c lprior_j| + |a_j|].
    top is one of the a_j; d_j = a_j - top rounds once: D_j = A_j + A_best + |d_j| absolute.  e_j = exp(d_j) within 1 ulp (<= 2 u
    relative) of the exp of a d_j that is D_j u off: E_j = D_j + 2 relative.  tot adds K roundings of partial sums <= tot to the
    weighted sum_j s_j E_j: T = sum_j s_j E_j + K relative, which is T u ABSOLUTE on log(tot), plus log's own ulp (2 |log tot| u).
    The final subtraction rounds once (|lq_j| u):   |lq_j - exact| <= (D_j + T + 2 |log tot| + |lq_j|) u."""
    m = len(members)
    if m == 1:
        r = members[0]
        return lp[r].astype(LD), boxes[r].astype(LD), LD(var[r]), np.zeros(lp.shape[1])
    x = lp[members].astype(LD)
    pooled = weights is not None
    W = LD(m)
    if pooled:
        w = weights[members].astype(LD)
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
    top = a.max()
    jb = int(np.argmax(a))
    d = a - top
    e = np.exp(d)
    tot = seq_sum(list(e))
    lq = d - np.log(tot)
    D = A + A[jb] + np.abs(d.astype(np.float64))
    s = (e / tot).astype(np.float64)
    T = float((s * (D + 2.0)).sum()) + len(a) - 1
    bound = D + T + 2.0 * abs(float(np.log(tot))) + np.abs(lq.astype(np.float64))
    b, v, sc = boxes[members].astype(LD), var[members].astype(LD), scores[members].astype(LD)
    if box == "argmax":
        t = int(np.argmax(scores[members]))          # first maximum in cluster order
        return lq, b[t], v[t], bound
    lam = {"v-avg": (1 / v) / (1 / v).sum(), "s-avg": sc / sc.sum(), "avg": np.full(m, LD(1) / m)}[box]
    fused_var = 1 / (1 / v).sum() if box == "v-avg" else (lam * lam * v).sum()
    return lq, (lam[:, None] * b).sum(0), fused_var, bound


def var_bound(box, m):
    """Relative bound on the kernel's fused variance in units of u.  v-avg: m reciprocals (u each), m - 1 additions of positive terms
    ((m - 1) u), one reciprocal: (m + 1) u <= (m + 3) u.  s-avg: lambda = s / wsum carries wsum's (m - 1) u and its own division
    (m u); squared 2 m u + u; times var u: (2 m + 2) u per positive term, m - 1 additions: (3 m + 1) u <= (3 m + 4) u.  avg: lambda =
    1 / m rounds once, so (m + 3) u <= (3 m + 4) u.  argmax and single rows: a copy."""
    return {"v-avg": m + 3, "s-avg": 3 * m + 4, "avg": 3 * m + 4, "argmax": 0}[box] if m > 1 else 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_flags_and_keywords_are_refused_outside_proben_log():
    from proben_amd import fusion as F
    from proben_amd.cli import calibration_report
    from proben_amd.late_fusion import late_fusion
    from proben_amd.opt import config_parser
    from proben_amd.pipeline import FramePairPipeline
    for mode in ("probEn", "avg", "max"):
        with pytest.raises(SystemExit):
            config_parser(["--write_fused", "fused.json", "--score_fusion", mode])
    with pytest.raises(SystemExit):
        config_parser(["--write_fused", "fused.json"])                  # the default score fusion is probEn
    assert config_parser(["--write_fused", "fused.json", "--score_fusion", "probEn-log"]).write_fused == "fused.json"
    assert config_parser([]).write_fused is None
    z = torch.zeros((0, 4), dtype=torch.float64)
    msg = "with_posterior belongs to score_fusion 'probEn-log'"
    for mode in ("probEn", "avg", "max", "probEn_binary"):
        with pytest.raises(ValueError, match=msg):
            F.fuse_batch(z, z[:, 0], z[:, :3], z[:, 0], z[:, 0].int(), torch.zeros(1, dtype=torch.int32), score_fusion=mode, with_posterior=True)
        with pytest.raises(ValueError, match=msg):
            F.fuse_detections([], mode, with_posterior=True)
        with pytest.raises(ValueError, match=msg):
            late_fusion([], [mode, "v-avg"], with_posterior=True)
        with pytest.raises(ValueError, match=msg):
            FramePairPipeline([], mode, with_posterior=True)
    rep = ["--predictions", "a.json", "b.json", "--dataset_path", "d", "--calibration", "c.json", "--fused-posterior"]
    with pytest.raises(SystemExit):
        calibration_report.parse(rep)                                   # --score_fusion defaults to probEn
    assert calibration_report.parse(rep + ["--score_fusion", "probEn-log"]).fused_posterior
    assert not calibration_report.parse(rep[:-1]).fused_posterior


def test_argument_checks_answer_without_a_gpu():
    """pe_proben_fuse_batch_posterior checks its arguments before any device work and explains itself through pe_last_error()."""
    import __graft_entry__ as g
    g.build()
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()  # noqa: E731
    P = 4096      # a non-null pointer that is never dereferenced
    who = "pe_proben_fuse_batch_posterior"

    def fuse(row_source=P, weights=P, nd=2, K=3, boxes=P, lq=P, var=P, mem=P, box_mode=0, rows=64, counts=P):
        return L.pe_proben_fuse_batch_posterior(boxes, P, P, P, P, row_source, P, None, None, 1, K, rows, box_mode, 0.5, 640.0, 512.0, None,
                                                weights, nd, P, P, P, P, counts, None, lq, var, mem, None)
    assert fuse(boxes=None) == -1 and f"{who}: null input pointer" in err()
    assert fuse(counts=None) == -1 and f"{who}: null output pointer" in err()
    assert fuse(row_source=None) == -1 and "row_source and pool_weights go together" in err()
    assert fuse(weights=None) == -1 and "row_source and pool_weights go together" in err()
    for kw in ({"lq": None}, {"var": None}, {"mem": None}):
        assert fuse(**kw) == -1 and "out_log_posterior / out_vars / out_members" in err()
    assert fuse(nd=0) == -1 and "num_detectors 0 not in [1,8]" in err()
    assert fuse(nd=9) == -1 and "num_detectors 9 not in [1,8]" in err()
    assert fuse(K=63) == -1 and "num_classes 63 not in [1,62]" in err()
    assert fuse(K=63, row_source=None, weights=None, nd=0) == -1 and "num_classes 63 not in [1,62]" in err()
    assert fuse(box_mode=4) == -1 and "bad box_mode 4" in err()
    assert fuse(rows=0) == -1 and "max_rows_per_image 0 not in [1,2048]" in err()
    assert fuse(rows=2000) == -2 and "LDS" in err()
    assert L.pe_proben_fuse_batch_posterior(None, None, None, None, None, None, None, None, None, 0, 3, 64, 0, 0.5, 640.0, 512.0, None, None, 0,
                                            None, None, None, None, None, None, None, None, None, None) == 0         # no image: nothing to do


# ---- fused_to_j1 ------------------------------------------------------------------------------------------------------------------

def test_fused_to_j1_on_hand_made_rows():
    from proben_amd.late_fusion import J1_KEYS, fused_to_j1
    dets = [{"image": ["a0", "a1", "a2"], "image_id": [10, 11, 12]}, {"image": ["b0", "b1", "b2"], "image_id": [20, 21, 22]}]
    lq0 = np.log(np.array([[0.7, 0.1, 0.1, 0.1], [0.05, 0.05, 0.1, 0.8], [0.2, 0.5, 0.2, 0.1]]))
    img0 = (np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [9.5, 10.5, 11.5, 12.5]]), torch.tensor([0.7, 0.8, 0.5]), torch.tensor([0.0, 3.0, 1.0]),
            lq0, np.array([0.25, 1.5, 2.0]), np.array([2, 3, 1], np.int32))
    img2 = (np.zeros((0, 4)), torch.zeros(0), torch.zeros(0), np.zeros((0, 4)), np.zeros(0), np.zeros(0, np.int32))
    j1, dropped = fused_to_j1(dets, [img0, None, img2])
    assert dropped == 1                                                  # img0's second row is background (class K = 3)
    assert list(j1) == J1_KEYS
    assert j1["image"] == ["b0", "b1", "b2"] and j1["image_id"] == [20, 21, 22]          # dets[1]'s, as the driver pairs them
    assert j1["boxes"] == [[[1.0, 2.0, 3.0, 4.0], [9.5, 10.5, 11.5, 12.5]], [], []]
    assert j1["scores"] == [[float(np.float32(0.7)), 0.5], [], []]
    assert j1["classes"] == [[0, 1], [], []] and all(isinstance(c, int) for c in j1["classes"][0])
    assert j1["class_logits"] == [[lq0[0].tolist(), lq0[2].tolist()], [], []]
    assert j1["probs"] == [[np.exp(lq0[0, :3]).tolist(), np.exp(lq0[2, :3]).tolist()], [], []]
    assert j1["vars"] == [[[0.25], [2.0]], [], []]
    # the file is a valid probEn-log input at T = 1: softmax(class_logits / 1) is the posterior it carries
    lg = np.asarray(j1["class_logits"][0])
    sm = np.exp(lg - lg.max(1, keepdims=True))
    np.testing.assert_allclose(sm / sm.sum(1, keepdims=True), np.exp(lq0[[0, 2]]), rtol=1e-15)
    import json
    assert json.loads(json.dumps(j1)) == j1
    with pytest.raises(ValueError, match="carry no posterior"):
        fused_to_j1(dets, [img0[:3], None, None])


# ---- the restatement's own associativity ------------------------------------------------------------------------------------------

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
        sc = np.exp(lp.max(1))
        lq3, b3, v3, _ = restate(lp, boxes, sc, var, [0, 1, 2], "v-avg", prior)
        lq1, b1, v1, _ = restate(lp, boxes, sc, var, [0, 1], "v-avg", prior)
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
