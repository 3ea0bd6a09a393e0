"""Correlated box fusion, box_fusion "c-avg" (csrc/boxcorr.hip, calibration.fit_box_correlation): what can be
checked without a GPU, and the references the GPU tests (tests/test_boxcorr_gpu.py) compare the kernels against - `restate`, the dense
generalised-least-squares mean in np.longdouble, and the NumPy restatement of the fit's statistics.  The comparator is never the code
under test.  u = 2^-53."""
import ctypes
import math

import numpy as np
import pytest

U = 2.0 ** -53
LD = np.longdouble
MAX_D = 4
# The constant of |y - y_ref| <= C_GLS * cond_2(R) * u * |y_ref|, |.| the largest entry (entry by entry there is no such bound: under
# a strong correlation a weight can pass through zero, and the error of a solve is relative to the solution's size, not to each entry's).
# Four times the largest ratio test_woodbury_transcription_against_the_dense_solve observes between the float64 transcription of the
# kernel's Woodbury elimination and the dense longdouble solve: 15.71 over its 2 000 clusters (the test prints it and asserts that the
# constant covers 4 x what it sees).  The factor four is for what the device's sqrt and division may differ from the host's by.  Not taken
# from the code under test.
C_GLS = 64.0
BBOX_REG_WEIGHTS = (10.0, 10.0, 5.0, 5.0)


# ---- the references -------------------------------------------------------------------------------------------------------------

def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in np.longdouble (numpy.linalg has no longdouble solver)."""
    A, b = A.astype(LD).copy(), b.astype(LD).copy()
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]], b[[k, p]] = A[[p, k]], b[[p, k]]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]
            b[i] -= f * b[k]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def cluster_correlation(src, P):
    """R = diag(1 - P[d][d]) + G P G': P[a][b] between two different rows, 1 on the diagonal."""
    src = np.asarray(src)
    R = np.asarray(P, dtype=np.float64)[np.ix_(src, src)].copy()
    np.fill_diagonal(R, 1.0)
    return R


def restate(coords, var, src, P):
    """The dense GLS mean of ONE cluster in np.longdouble: C_tu = R_tu s_t s_u, y = C^-1 1, Y = sum y, lambda = y / Y, box = sum_t
    coord_t lambda_t, out_var = 1 / Y.  coords f64 [m, 4], var f64 [m] (after the variance scales), src int [m] (each row's detector), P
    [D][D]; the rows in ascending input-row order.  Returns {"y", "lam", "box", "var" (longdouble), "cond" (cond_2(R), float64)}."""
    R = cluster_correlation(src, P)
    s = np.sqrt(np.asarray(var, dtype=np.float64).astype(LD))
    C = R.astype(LD) * s[:, None] * s[None, :]
    y = _solve_ld(C, np.ones(len(s), dtype=LD))
    Y = y.sum()
    lam = y / Y
    return {"y": y, "lam": lam, "box": (np.asarray(coords, dtype=np.float64).astype(LD) * lam[:, None]).sum(0), "var": LD(1) / Y,
            "cond": float(np.linalg.cond(R))}


def woodbury_weights(var, src, P):
    """The kernel's arithmetic for y, float64, operation by operation (csrc/boxcorr.hip: walk 1, solve4, weight): Python floats are IEEE
    float64 and nothing is contracted."""
    D = len(P)
    Pp = [[float(P[i][j]) if i < D and j < D else 0.0 for j in range(MAX_D)] for i in range(MAX_D)]
    ad = [1.0 - Pp[i][i] for i in range(MAX_D)]
    n, us = [0.0] * MAX_D, [0.0] * MAX_D
    for v, d in zip(var, src):
        u = 1.0 / math.sqrt(float(v))
        n[d] += 1.0
        us[d] += u
    nn = [n[d] / ad[d] for d in range(MAX_D)]
    g = [us[d] / ad[d] for d in range(MAX_D)]
    A = [[(1.0 if i == j else 0.0) + Pp[i][j] * nn[j] for j in range(MAX_D)] for i in range(MAX_D)]
    b = []
    for i in range(MAX_D):
        acc = 0.0
        for j in range(MAX_D):
            acc += Pp[i][j] * g[j]
        b.append(acc)
    for k in range(MAX_D - 1):
        for i in range(k + 1, MAX_D):
            f = A[i][k] / A[k][k]
            for j in range(k + 1, MAX_D):
                A[i][j] -= f * A[k][j]
            b[i] -= f * b[k]
    w = [0.0] * MAX_D
    for i in range(MAX_D - 1, -1, -1):
        acc = b[i]
        for j in range(i + 1, MAX_D):
            acc -= A[i][j] * w[j]
        w[i] = acc / A[i][i]
    out = []
    for v, d in zip(var, src):
        v = float(v)
        s = math.sqrt(v)
        out.append((1.0 / v) / ad[d] - w[d] / (ad[d] * s))
    return np.array(out)


def random_correlation(rng, D, diag_hi=0.9, off_hi=0.95):
    """A P that is itself positive semidefinite, so that every composition of rows has a positive definite R: diagonal uniform in
    [0, diag_hi], off-diagonals uniform in [-off_hi / 2, off_hi], shrunk towards the diagonal until it is (a reference-side search,
    coarser than the code's)."""
    P = np.zeros((D, D))
    for a in range(D):
        P[a, a] = rng.uniform(0.0, diag_hi)
        for b in range(a + 1, D):
            P[a, b] = P[b, a] = rng.uniform(-off_hi / 2, off_hi)
    diag = np.diag(np.diag(P))
    f = 1.0
    while np.linalg.eigvalsh(diag + f * (P - diag))[0] < 1e-9:
        f *= 0.9
    return diag + f * (P - diag)


def positive_definite(src, P):
    return float(np.linalg.eigvalsh(cluster_correlation(src, P))[0]) > 0.0


def get_deltas(det, gt, w=BBOX_REG_WEIGHTS):
    """Box2BoxTransform.get_deltas(detection, ground truth) over [n, 4] arrays, the expressions of pe_variance_stats."""
    sw, sh = det[:, 2] - det[:, 0], det[:, 3] - det[:, 1]
    tw, th = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    scx, scy = det[:, 0] + 0.5 * sw, det[:, 1] + 0.5 * sh
    tcx, tcy = gt[:, 0] + 0.5 * tw, gt[:, 1] + 0.5 * th
    return np.stack([w[0] * (tcx - scx) / sw, w[1] * (tcy - scy) / sh, w[2] * np.log(tw / sw), w[3] * np.log(th / sh)], 1)


def detection_with_residual(gt, r, w=BBOX_REG_WEIGHTS):
    """The box whose get_deltas(box, gt) is r: w_det = w_gt / exp(r_w / ww), cx_det = cx_gt - r_x * w_det / wx."""
    tw, th = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    tcx, tcy = gt[:, 0] + 0.5 * tw, gt[:, 1] + 0.5 * th
    sw, sh = tw / np.exp(r[:, 2] / w[2]), th / np.exp(r[:, 3] / w[3])
    scx, scy = tcx - r[:, 0] * sw / w[0], tcy - r[:, 1] * sh / w[1]
    return np.stack([scx - 0.5 * sw, scy - 0.5 * sh, scx + 0.5 * sw, scy + 0.5 * sh], 1)


def simulate_pairs(rng, n, rho):
    """n two-detector clusters (rows 2c and 2c + 1 of detectors 0 and 1).  The ground truth first, z correlated at rho through a Cholesky
    factor, variances log-uniform over two decades, each detection the box whose residual is exactly z * sqrt(var).
    Returns (det f64 [2n, 4], var f64 [2n], src i32 [2n], gt f64 [n, 4])."""
    x1, y1 = rng.uniform(0, 400, n), rng.uniform(0, 300, n)
    gt = np.stack([x1, y1, x1 + rng.uniform(20, 200, n), y1 + rng.uniform(20, 200, n)], 1)
    L = np.linalg.cholesky(np.array([[1.0, rho], [rho, 1.0]]))
    z = np.einsum("ab,nbc->nac", L, rng.standard_normal((n, 2, 4)))
    var = 10.0 ** rng.uniform(-3.0, -1.0, (n, 2))
    r = z * np.sqrt(var)[:, :, None]
    det = np.stack([detection_with_residual(gt, r[:, 0]), detection_with_residual(gt, r[:, 1])], 1).reshape(2 * n, 4)
    return det, var.reshape(-1), np.tile(np.array([0, 1], dtype=np.int32), n), gt


def pair_stats_numpy(det, var, src, member_rows, cluster_offsets, match, gt, D, w=BBOX_REG_WEIGHTS):
    """pe_box_pair_stats restated: the terms in float64 NumPy, the sums with math.fsum.  Returns (pairs int [D, D], rows [D], S [D, D], Q [D],
    excluded, S_abs [D, D], Q_abs [D], last): S_abs / Q_abs the sums of the terms' magnitudes (what the GPU test's bound multiplies),
    last the index of the last excluded member or -1."""
    pairs, rows = np.zeros((D, D), dtype=np.int64), [0] * D
    s_terms = {(a, b): [] for a in range(D) for b in range(a, D)}
    q_terms = {d: [] for d in range(D)}
    excluded, last = 0, -1
    for c in range(len(match)):
        g = int(match[c])
        if g < 0:
            continue
        mem = []
        for t in range(int(cluster_offsets[c]), int(cluster_offsets[c + 1])):
            row = int(member_rows[t])
            v, d, b = float(var[row]), int(src[row]), det[row]
            ok = v > 0 and math.isfinite(v) and 0 <= d < D and b[2] - b[0] > 0 and b[3] - b[1] > 0 \
                and gt[g, 2] - gt[g, 0] > 0 and gt[g, 3] - gt[g, 1] > 0
            if not ok:
                excluded, last = excluded + 1, t
                continue
            r = get_deltas(b[None], gt[g][None], w)[0]
            mem.append((d, r, math.sqrt(v), v))
        for i, (d, r, s, v) in enumerate(mem):
            rows[d] += 1
            q_terms[d].append(float(((r[0] * r[0] / v + r[1] * r[1] / v) + r[2] * r[2] / v) + r[3] * r[3] / v))
            for d2, r2, s2, _ in mem[i + 1:]:
                den = s * s2
                a, b = min(d, d2), max(d, d2)
                pairs[a, b] += 1
                s_terms[(a, b)].append(float(((r[0] * r2[0] / den + r[1] * r2[1] / den) + r[2] * r2[2] / den) + r[3] * r2[3] / den))
    S, S_abs, Q, Q_abs = np.zeros((D, D)), np.zeros((D, D)), [0.0] * D, [0.0] * D
    for (a, b), ts in s_terms.items():
        S[a, b] = S[b, a] = math.fsum(ts)
        S_abs[a, b] = S_abs[b, a] = math.fsum(abs(t) for t in ts)
        pairs[b, a] = pairs[a, b]
    for d, ts in q_terms.items():
        Q[d], Q_abs[d] = math.fsum(ts), math.fsum(abs(t) for t in ts)
    return pairs, rows, S, Q, excluded, S_abs, Q_abs, last


def estimate_numpy(pairs, rows, S, Q):
    """rho_ab = (S_ab / (4 N_ab)) / sqrt((Q_a / (4 M_a)) * (Q_b / (4 M_b))), 0 without pairs."""
    D = len(rows)
    rho = np.zeros((D, D))
    for a in range(D):
        for b in range(D):
            if pairs[a, b] and rows[a] and rows[b]:
                rho[a, b] = (S[a, b] / (4 * pairs[a, b])) / math.sqrt((Q[a] / (4 * rows[a])) * (Q[b] / (4 * rows[b])))
    return rho


def fuse_pairs_in_error_space(r, var, rho):
    """Two-row clusters in error space (the residuals themselves): the GLS error sum_t lambda_t r_t and its variance 1 / Y under the
    correlation rho, closed form of the 2 x 2 inverse.  r [n, 2, 4], var [n, 2]."""
    s = np.sqrt(var)
    cross = rho * s[:, 0] * s[:, 1]
    det = var[:, 0] * var[:, 1] - cross * cross
    y = np.stack([(var[:, 1] - cross) / det, (var[:, 0] - cross) / det], 1)
    Y = y.sum(1)
    lam = y / Y[:, None]
    return (r * lam[:, :, None]).sum(1), 1.0 / Y, lam


# ---- the tests ------------------------------------------------------------------------------------------------------------------

def test_woodbury_transcription_against_the_dense_solve(capsys):
    """The float64 transcription of the kernel's elimination against `restate`: 2 000 random clusters, m in [2, 12], D in {2, 3, 4},
    several rows per detector, P[d][d] up to 0.9, off-diagonals up to 0.95.  Fixes C_GLS: four times the largest
    max_t |y_t - y_ref_t| / (cond_2(R) u max_t |y_ref_t|) seen here must not exceed it."""
    rng = np.random.default_rng(20240519)
    worst = 0.0
    for _ in range(2000):
        D = int(rng.integers(2, 5))
        m = int(rng.integers(2, 13))
        P = random_correlation(rng, D)
        src = rng.integers(0, D, m)
        var = 10.0 ** rng.uniform(-3.0, -1.0, m)
        ref = restate(np.zeros((m, 4)), var, src, P)
        y = woodbury_weights(var, src, P)
        worst = max(worst, float(np.abs(y.astype(LD) - ref["y"]).max() / (ref["cond"] * U * np.abs(ref["y"]).max())))
    with capsys.disabled():
        print(f"\n[boxcorr] Woodbury transcription vs dense longdouble solve: largest max|dy| / (cond(R) u max|y|) = {worst:.3f}; "
              f"C_GLS = {C_GLS} (4 x {C_GLS / 4})")
    assert 4.0 * worst <= C_GLS


def test_zero_matrix_gives_the_v_avg_weights_exactly():
    rng = np.random.default_rng(7)
    for D in (1, 2, 3, 4):
        for _ in range(50):
            m = int(rng.integers(2, 13))
            var = 10.0 ** rng.uniform(-4.0, 2.0, m)
            y = woodbury_weights(var, rng.integers(0, D, m), np.zeros((D, D)))
            assert np.array_equal(y, 1.0 / var)


def test_check_box_correlation():
    from proben_amd import calibration as cal
    good = [[0.2, 0.5], [0.5, 0.2]]
    assert np.array_equal(cal.check_box_correlation(good, 2), np.array(good))
    assert cal.check_box_correlation([[0.0]]).shape == (1, 1)
    for bad, word in [([[0.0, 0.5], [0.4, 0.0]], "symmetric"), ([[0.0, float("nan")], [float("nan"), 0.0]], "finite"),
                      ([[0.0, float("inf")], [float("inf"), 0.0]], "finite"),
                      ([[0.0, 0.9, 0.9], [0.9, 0.0, -0.9], [0.9, -0.9, 0.0]], "semidefinite"), ([[1.0, 0.0], [0.0, 0.0]], "[0, 1)"),
                      ([[-0.1, 0.0], [0.0, 0.0]], "[0, 1)"), ([[0.0, 0.1, 0.2], [0.1, 0.0, 0.3]], "square"), (np.zeros((5, 5)), "square"),
                      ("no", "matrix")]:
        with pytest.raises(ValueError, match=word.replace("[", r"\[").replace(")", r"\)")):
            cal.check_box_correlation(bad)
    with pytest.raises(ValueError, match="over 2 detectors, not 3"):
        cal.check_box_correlation(good, 3)
    assert cal.BOX_CORR_MAX_DETECTORS == cal.PRESENCE_MAX_DETECTORS == MAX_D


def test_parse_and_resolve_box_correlation():
    from proben_amd import calibration as cal
    P = cal.parse_box_correlation("rgb:thermal=0.5,rgb:rgb=0.2", ["rgb", "thermal"])
    assert np.array_equal(P, np.array([[0.2, 0.5], [0.5, 0.0]]))
    assert np.array_equal(cal.parse_box_correlation("thermal:rgb=0.5", ["rgb", "thermal"]), np.array([[0.0, 0.5], [0.5, 0.0]]))
    assert np.array_equal(cal.parse_box_correlation("0.3", ["a", "b"]), np.array([[0.0, 0.3], [0.3, 0.0]]))
    assert cal.parse_box_correlation("a:c=0.25", ["a", "b", "c"])[0, 2] == 0.25
    for text, names, word in [("0.3", ["a", "b", "c"], "bare number"), ("a:x=0.3", ["a", "b"], "unknown detector"),
                              ("a:b=0.3,b:a=0.2", ["a", "b"], "twice"), ("a:b", ["a", "b"], "name:name=value"),
                              ("a=0.3", ["a", "b"], "name:name=value"), ("a:b=much", ["a", "b"], "number"), ("", ["a", "b"], "no pair"),
                              ("a:b=0.9,a:c=0.9,b:c=-0.9", ["a", "b", "c"], "semidefinite"), ("a:a=1.0", ["a", "b"], "diagonal"),
                              ("1.5", ["a", "b"], "semidefinite")]:
        with pytest.raises(ValueError, match=word):
            cal.parse_box_correlation(text, names)
    rec = {"detectors": ["thermal", "rgb"], "matrix": [[0.1, 0.4], [0.4, 0.3]]}
    assert np.array_equal(cal.resolve_box_correlation(rec, ["rgb", "thermal"], "file"), np.array([[0.3, 0.4], [0.4, 0.1]]))
    assert np.array_equal(cal.resolve_box_correlation(rec, ["thermal", "rgb"], "file"), np.array(rec["matrix"]))
    for names in (["rgb", "early"], ["rgb"], ["rgb", "thermal", "early"]):
        with pytest.raises(ValueError, match="is over thermal,rgb"):
            cal.resolve_box_correlation(rec, names, "file")
    with pytest.raises(ValueError, match="not a box-correlation record"):
        cal.resolve_box_correlation({"matrix": [[0.0]]}, ["rgb"], "file")
    with pytest.raises(ValueError, match="symmetric"):
        cal.resolve_box_correlation({"detectors": ["a", "b"], "matrix": [[0, 0.1], [0.2, 0]]}, ["a", "b"], "file")


def test_save_and_load_carry_the_box_correlation(tmp_path):
    from proben_amd import calibration as cal
    path = str(tmp_path / "cal.json")
    rec = {"detectors": ["rgb", "thermal"], "matrix": [[0.0, 0.6], [0.6, 0.0]], "raw": [[0.0, 0.6], [0.6, 0.0]], "shrink": 1.0,
           "pairs": [[0, 10], [10, 0]], "rows": [10, 10], "excluded": 0, "iou": 0.5, "box_fusion": "v-avg"}
    cal.save(path, {"rgb": 1.0, "thermal": 2.0}, box_correlation=rec)
    back = cal.load(path)
    assert back["box_correlation"] == rec
    cal.save(path, {"rgb": 1.0, "thermal": 2.0})
    assert "box_correlation" not in cal.load(path)
    with pytest.raises(ValueError, match="semidefinite"):
        cal.save(path, {"rgb": 1.0}, box_correlation={"detectors": ["a", "b"], "matrix": [[0, 1.5], [1.5, 0]]})


def unit_diagonal_min_eig(P):
    """The eigenvalue check_box_correlation looks at, restated: the smallest one of P with its diagonal set to 1."""
    M = np.array(P, dtype=np.float64)
    np.fill_diagonal(M, 1.0)
    return float(np.linalg.eigvalsh(M)[0])


def test_positive_semidefinite_shrink():
    from proben_amd import calibration as cal
    raw = np.array([[0.1, 0.9, 0.9], [0.9, 0.0, -0.9], [0.9, -0.9, 0.2]])
    fixed, f = cal.shrink_to_psd(raw)
    assert 0.0 < f < 1.0
    assert unit_diagonal_min_eig(raw) < -0.5 and unit_diagonal_min_eig(fixed) >= -1e-12
    assert np.array_equal(np.diag(fixed), np.diag(raw))
    diag = np.diag(np.diag(raw))
    assert np.array_equal(fixed, diag + f * (raw - diag))
    # the largest factor that works, found here by a finer search of its own: the smallest eigenvalue is concave in the factor
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if unit_diagonal_min_eig(diag + mid * (raw - diag)) >= -1e-12 else (lo, mid)
    assert abs(f - lo) <= 1e-6 and f <= lo + 1e-15
    cal.check_box_correlation(fixed)
    ok = np.array([[0.2, 0.5], [0.5, 0.2]])
    same, one = cal.shrink_to_psd(ok)
    assert one == 1.0 and np.array_equal(same, ok)


def test_estimator_clamps_and_reports():
    from proben_amd import calibration as cal
    pairs = np.array([[5, 40], [40, 0]])
    est = cal.box_correlation_estimate(pairs, [50, 40], np.array([[-2.0, 80.0], [80.0, 0.0]]), [200.0, 160.0])
    assert est["empty"] == [[1, 1]] and est["clamped"] == [0]
    assert est["raw"][0][0] < 0 and est["matrix"][0][0] == 0.0 and est["matrix"][1][1] == 0.0
    assert est["raw"][0][1] == pytest.approx((80.0 / 160) / 1.0)
    assert est["stderr"][0][1] == pytest.approx(math.sqrt((1 + 0.25) / 160)) and est["stderr"][1][1] is None


@pytest.fixture(scope="module")
def simulation():
    """Per rho: the estimate on 20 000 clusters, then coverage and mean squared error of both box rules on 20 000 more."""
    from proben_amd import calibration as cal
    out = {}
    for k, rho in enumerate((0.0, 0.3, 0.6, 0.9)):
        rng = np.random.default_rng(1000 + k)
        n = 20000
        det, var, src, gt = simulate_pairs(rng, n, rho)
        r = get_deltas(det, np.repeat(gt, 2, 0))
        z = (r / np.sqrt(var)[:, None]).reshape(n, 2, 4)
        S01 = float((z[:, 0] * z[:, 1]).sum())
        Q = [float((z[:, 0] ** 2).sum()), float((z[:, 1] ** 2).sum())]
        est = cal.box_correlation_estimate(np.array([[0, n], [n, 0]]), [n, n], np.array([[0.0, S01], [S01, 0.0]]), Q)
        rho_hat = est["matrix"][0][1]
        det2, var2, _, gt2 = simulate_pairs(rng, n, rho)
        r2 = get_deltas(det2, np.repeat(gt2, 2, 0)).reshape(n, 2, 4)
        v2 = var2.reshape(n, 2)
        rec = {"rho_hat": rho_hat, "stderr": est["stderr"][0][1], "n": n, "est": est}
        for rule, used in (("c-avg", rho_hat), ("v-avg", 0.0)):
            e, fv, lam = fuse_pairs_in_error_space(r2, v2, used)
            rec[rule] = {"coverage": float((np.abs(e) <= np.sqrt(fv)[:, None]).mean()), "mse": float((e ** 2).mean()),
                         "negative": float((lam.min(1) < 0).mean())}
        out[rho] = rec
    return out


@pytest.mark.parametrize("rho", [0.0, 0.3, 0.6, 0.9])
def test_simulation_recovers_the_correlation_and_the_coverage(simulation, rho, capsys):
    rec = simulation[rho]
    se = math.sqrt((1 + rho * rho) / (4 * rec["n"]))
    with capsys.disabled():
        print(f"\n[boxcorr] rho {rho}: rho_hat {rec['rho_hat']:.4f} ({(rec['rho_hat'] - rho) / se:+.2f} standard errors); 1-sigma coverage "
              f"c-avg {rec['c-avg']['coverage']:.4f} v-avg {rec['v-avg']['coverage']:.4f}; mse c-avg {rec['c-avg']['mse']:.5f} v-avg "
              f"{rec['v-avg']['mse']:.5f}; clusters with a negative weight {rec['c-avg']['negative']:.3f}")
    assert abs(rec["rho_hat"] - rho) <= 4 * se
    assert rec["stderr"] == pytest.approx(math.sqrt((1 + rec["rho_hat"] ** 2) / (4 * rec["n"])))
    assert rec["est"]["shrink"] == 1.0 and rec["est"]["empty"] == [[0, 0], [1, 1]]
    assert abs(rec["c-avg"]["coverage"] - 0.6827) <= 0.0066          # four binomial standard errors over 80 000 (row, coordinate) pairs
    if rho == 0.6:
        assert rec["v-avg"]["coverage"] < 0.62
        assert rec["c-avg"]["mse"] < rec["v-avg"]["mse"]


def test_detection_built_from_a_residual_has_that_residual():
    rng = np.random.default_rng(3)
    det, var, src, gt = simulate_pairs(rng, 500, 0.6)
    r = get_deltas(det, np.repeat(gt, 2, 0))
    assert np.all(np.abs(r) / np.sqrt(var)[:, None] < 7.0)
    back = detection_with_residual(np.repeat(gt, 2, 0), r)
    assert np.allclose(back, det, rtol=0, atol=1e-9)


def test_check_mode_refusals():
    import proben_amd.fusion as F
    P = [[0.0, 0.5], [0.5, 0.0]]
    for score in ("probEn", "avg", "max"):
        with pytest.raises(ValueError, match="c-avg"):
            F._check_mode(score, None, "fuse_batch", box_fusion="c-avg", box_correlation=P)
    with pytest.raises(ValueError, match="needs a box_correlation"):
        F._check_mode("probEn-log", None, "fuse_batch", box_fusion="c-avg")
    with pytest.raises(ValueError, match="box_correlation belongs to"):
        F._check_mode("probEn-log", None, "fuse_batch", box_fusion="v-avg", box_correlation=P)
    F._check_mode("probEn-log", None, "fuse_batch", box_fusion="c-avg", box_correlation=P)
    F._check_mode("probEn", None, "fuse_batch", box_fusion="v-avg")
    assert "c-avg" not in F.BOX_MODES          # the fusion kernel never sees it
    import torch
    z = torch.zeros((0, 4), dtype=torch.float64)
    args = (z, z[:, 0], z[:, :3], z[:, 0], z[:, 0].int(), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs a box_correlation"):
        F.fuse_batch(*args, score_fusion="probEn-log", box_fusion="c-avg")
    with pytest.raises(ValueError, match="box_correlation belongs to"):
        F.fuse_batch(*args, score_fusion="probEn-log", box_fusion="v-avg", box_correlation=P)
    with pytest.raises(ValueError, match="c-avg"):
        F.fuse_batch(*args, score_fusion="probEn", box_fusion="c-avg", box_correlation=P)


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.LIB_PATH


def test_argument_checks_answer_before_any_device_work(built_lib):
    """Both entry points refuse bad arguments through pe_last_error() without touching a device (this machine has none)."""
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()
    p = 4096          # a non-null pointer that is never dereferenced: every call below fails its checks first
    gls = lambda **kw: L.pe_box_gls_batch(*[kw.get(k, d) for k, d in
                                           [("boxes", p), ("vars", p), ("src", p), ("cluster", p), ("offsets", p), ("row_counts", None),
                                            ("counts", p), ("B", 1), ("max_rows", 64), ("corr", p), ("D", 2), ("out_boxes", p),
                                            ("out_vars", None), ("stream", None)]])
    assert gls(B=0) == 0                                            # no image: nothing to do
    assert gls(B=-1) != 0 and "num_images" in err()
    for D in (0, 5, -1):
        assert gls(D=D) != 0 and "num_detectors" in err() and "[1,4]" in err()
    for R in (0, 2049, -3):
        assert gls(max_rows=R) != 0 and "max_rows_per_image" in err() and "[1,2048]" in err()
    for k in ("boxes", "vars", "src", "cluster", "offsets", "counts"):
        assert gls(**{k: None}) != 0 and "null input pointer" in err()
    assert gls(corr=None) != 0 and "correlation" in err()
    assert gls(out_boxes=None) != 0 and "null output pointer" in err()
    w = (ctypes.c_float * 4)(10, 10, 5, 5)
    pair = lambda **kw: L.pe_box_pair_stats(*[kw.get(k, d) for k, d in
                                             [("boxes", p), ("vars", p), ("src", p), ("N", 8), ("members", p), ("M", 8), ("offsets", p),
                                              ("match", p), ("C", 4), ("gt", p), ("G", 4), ("D", 2), ("w", w), ("work", p), ("out", p),
                                              ("flags", p), ("stream", None)]])
    for D in (0, 5):
        assert pair(D=D) != 0 and "num_detectors" in err()
    for k in ("C", "N", "M", "G"):
        assert pair(**{k: -1}) != 0 and "num_clusters" in err()
    for k in ("work", "out", "flags"):
        assert pair(**{k: None}) != 0 and "workspace / out / out_flags" in err()
    for k in ("members", "offsets", "match"):
        assert pair(**{k: None}) != 0 and "member_rows" in err()
    for k in ("boxes", "vars", "src", "gt"):
        assert pair(**{k: None}) != 0 and "row_source" in err()
    assert pair(w=(ctypes.c_float * 4)(10, 10, 0, 5)) != 0 and "bbox_reg_weights[2]" in err()
    assert pair(w=(ctypes.c_float * 4)(10, float("nan"), 5, 5)) != 0 and "bbox_reg_weights[1]" in err()
