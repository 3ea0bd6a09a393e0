"""Presence evidence for probEn-log (pe_proben_fuse_batch_presence, pe_bias_nll, fuse_batch(presence=...), calibration.fit_presence,
demo_probEn --presence): what can be checked without a GPU, the np.longdouble restatement of the fit's terms and the NumPy float64 fit
that the GPU tests (tests/test_presence_gpu.py) compare the kernels against, and the CPU simulation DESIGN.md section 18 quotes.  The
comparator is never the code under test; the rule itself is restated in tests/fuse_ref.py.  u = 2^-53."""
import json

import numpy as np
import pytest
import torch

from fuse_ref import LD, seq_sum


# ---- the fit, restated ------------------------------------------------------------------------------------------------------------

def bias_terms(base, labels, b):
    """Per cluster, in np.longdouble: (nll term [C], gradient term [C, K+1], nll bound [C], gradient bound [C, K+1], bounds absolute in
    units of u).  a_j = base_j + b_j rounds once (|a_j| u); d_j = a_j - top once more and carries both ends: D_j = |a_j| + |a_top| + |d_j|;
    e_j = exp(d_j): E_j = D_j + 2 relative; tot: T = sum_j s_j E_j + K relative; log(tot): T + 2 |log tot| absolute; the term
    log(tot) - d_y rounds once: T + 2 |log tot| + D_y + |term|.  s_j = e_j / tot: E_j + T + 1 relative; s_j - [y = j] rounds once:
    s_j (E_j + T + 1) + |s_j - [y = j]|."""
    a = base.astype(LD) + np.asarray(b, np.float64).astype(LD)[None, :]
    C, k1 = a.shape
    top = a.max(1, keepdims=True)
    d = a - top
    e = np.exp(d)
    tot = seq_sum(list(e.T))
    s = e / tot[:, None]
    rows = np.arange(C)
    term = np.log(tot) - d[rows, labels]
    ind = np.zeros((C, k1))
    ind[rows, labels] = 1.0
    g = s - ind
    af, df, sf = np.abs(a.astype(np.float64)), np.abs(d.astype(np.float64)), s.astype(np.float64)
    Dj = af + np.abs(top.astype(np.float64)) + df
    E = Dj + 2.0
    T = (sf * E).sum(1) + k1 - 1
    lt = np.abs(np.log(tot).astype(np.float64))
    nb = T + 2.0 * lt + Dj[rows, labels] + np.abs(term.astype(np.float64))
    gb = sf * (E + T[:, None] + 1.0) + np.abs(g.astype(np.float64))
    return term, g, nb, gb


def np_bias_nll(base, labels, b):
    """(nll, gradient [K+1], Hessian [K+1, K+1]) in float64: the restatement the NumPy fit runs on."""
    a = base + np.asarray(b, np.float64)[None, :]
    a = a - a.max(1, keepdims=True)
    e = np.exp(a)
    s = e / e.sum(1, keepdims=True)
    rows = np.arange(len(labels))
    nll = float(-(np.log(s[rows, labels])).sum())
    g = s.sum(0) - np.bincount(labels, minlength=base.shape[1])
    H = np.diag(s.sum(0)) - s.T @ s
    return nll, g, H


def np_fit_bias(base, labels, hi=16.0, gtol=1e-7, max_rounds=100):
    """One table row: b[:K] in [-hi, hi]^K, b_K = 0, minimising np_bias_nll by a projected Newton iteration with the exact Hessian and
    step halving.  Returns (b, rounds, converged by max |projected gradient| <= gtol * clusters)."""
    C, k1 = base.shape
    K = k1 - 1
    b = np.zeros(k1)
    if C == 0:
        return b, 0, True
    for rounds in range(1, max_rounds + 1):
        f, g, H = np_bias_nll(base, labels, b)
        g, H, x = g[:K], H[:K, :K], b[:K]
        held = ((x <= -hi) & (g > 0)) | ((x >= hi) & (g < 0))
        pg = np.where(held, 0.0, g)
        if np.max(np.abs(pg)) <= gtol * C:
            return b, rounds, True
        free = ~held
        p = np.zeros(K)
        p[free] = -np.linalg.solve(H[np.ix_(free, free)] + 1e-12 * np.eye(int(free.sum())), g[free])
        t = 1.0
        while t > 1e-12:
            trial = b.copy()
            trial[:K] = np.clip(x + t * p, -hi, hi)
            if np_bias_nll(base, labels, trial)[0] < f:
                break
            t *= 0.5
        else:
            return b, rounds, False
        b = trial
    return b, max_rounds, False


# ---- the simulation ---------------------------------------------------------------------------------------------------------------

PRIOR = np.array([0.12, 0.10, 0.08, 0.70])                      # three classes and background: most candidate places hold nothing
MU = np.array([[[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, 0.0]],
               [[1.5, 0.3, 0.0], [0.0, 1.8, 0.2], [0.3, 0.0, 1.6], [0.0, 0.0, 0.0]]])         # [detector][class] -> mean feature
FIRE = np.array([[0.85, 0.60, 0.75, 0.25], [0.55, 0.90, 0.70, 0.30]])                       # [detector][class] firing probability
RHO = 0.6                                                        # the detectors share a frame: their firing is correlated


def simulate(seed, n):
    """n clusters of two detectors over K + 1 = 4 columns.  A place has class y ~ PRIOR; detector d fires when its Gaussian latent
    (correlation RHO between the detectors, given the class: a Gaussian copula) falls under the class's firing quantile, and a place
    where nobody fires is no cluster (drawn again).  A detector that fires reports the posterior that is EXACT given its own feature
    and the fact that it fired: p_d(j | z_d, fired_d) ~ PRIOR_j FIRE_dj N(z_d; MU_dj, I).  The fused base is ProbEn's product of the
    rows present (uniform prior term).  Returns (base f64 [n, 4] normalised, pattern i32 [n], label i32 [n])."""
    from statistics import NormalDist
    rng = np.random.default_rng(seed)
    q = np.vectorize(NormalDist().inv_cdf)(FIRE)
    base, pat, lab = np.zeros((n, 4)), np.zeros(n, np.int32), np.zeros(n, np.int32)
    got = 0
    while got < n:
        N = 2 * (n - got) + 64
        y = rng.choice(4, N, p=PRIOR)
        shared = rng.normal(size=N)
        fired = np.stack([RHO * shared + np.sqrt(1 - RHO * RHO) * rng.normal(size=N) < q[d, y] for d in range(2)], 1)
        a = np.zeros((N, 4))
        for d in range(2):
            z = MU[d, y] + rng.normal(size=(N, 3))
            ll = -0.5 * ((z[:, None, :] - MU[d][None, :, :]) ** 2).sum(2) + np.log(PRIOR * FIRE[d])[None, :]
            ll = ll - ll.max(1, keepdims=True)
            ll = ll - np.log(np.exp(ll).sum(1, keepdims=True))
            a += np.where(fired[:, d, None], ll, 0.0)
        keep = np.nonzero(fired.any(1))[0][:n - got]
        a = a[keep] - a[keep].max(1, keepdims=True)
        base[got:got + len(keep)] = a - np.log(np.exp(a).sum(1, keepdims=True))
        pat[got:got + len(keep)] = fired[keep, 0] + 2 * fired[keep, 1]
        lab[got:got + len(keep)] = y[keep]
        got += len(keep)
    return base, pat, lab


def top_label_ece(lq, labels, bins=15):
    conf, hit = np.exp(lq.max(1)), lq.argmax(1) == labels
    idx = np.minimum((conf * bins).astype(int), bins - 1)
    return float(sum(abs(hit[idx == b].mean() - conf[idx == b].mean()) * (idx == b).mean() for b in range(bins) if (idx == b).any()))


def nll_of(base, labels, pattern, table):
    a = base + table[pattern]
    a = a - a.max(1, keepdims=True)
    lq = a - np.log(np.exp(a).sum(1, keepdims=True))
    return -lq[np.arange(len(labels)), labels], lq


def test_simulation_held_out_nll_falls_in_every_pattern():
    """The simulation of DESIGN.md section 18: 20 000 clusters fitted and 20 000 held out on seeds 0, 1 and 2, through the NumPy
    restatement alone.  Prints the fitted rows and the held-out NLL per cluster / top-label ECE before and after.  Asserted: every
    pattern's fit converges by the gradient criterion, held-out NLL falls overall and in every pattern."""
    for seed in (0, 1, 2):
        base, pat, lab = simulate(seed, 40000)
        fit, held = slice(0, 20000), slice(20000, 40000)
        table = np.zeros((4, 4))
        for P in (1, 2, 3):
            sel = pat[fit] == P
            b, rounds, conv = np_fit_bias(base[fit][sel], lab[fit][sel])
            assert conv and rounds <= 12, (seed, P, rounds)
            table[P] = b
        before, lq0 = nll_of(base[held], lab[held], pat[held], np.zeros((4, 4)))
        after, lq1 = nll_of(base[held], lab[held], pat[held], table)
        print(f"seed {seed}: rows " + " ".join(f"P={P}:({', '.join(f'{v:+.2f}' for v in table[P])})" for P in (1, 2, 3)))
        print(f"seed {seed}: held-out NLL per cluster {before.mean():.4f} -> {after.mean():.4f}; top-label ECE (15 bins) "
              f"{top_label_ece(lq0, lab[held]):.4f} -> {top_label_ece(lq1, lab[held]):.4f}; per pattern " +
              ", ".join(f"P={P}: {before[pat[held] == P].mean():.4f} -> {after[pat[held] == P].mean():.4f} ({int((pat[held] == P).sum())})"
                        for P in (1, 2, 3)))
        assert after.mean() < before.mean()
        for P in (1, 2, 3):
            assert after[pat[held] == P].mean() < before[pat[held] == P].mean(), (seed, P)


# ---- argument checks --------------------------------------------------------------------------------------------------------------

def test_argument_checks_answer_without_a_gpu():
    """Both entry points check their arguments before any device work and explain themselves through pe_last_error()."""
    import ctypes
    import __graft_entry__ as g
    g.build()
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()  # noqa: E731
    P = 4096      # a non-null pointer that is never dereferenced
    who = "pe_proben_fuse_batch_presence"

    def fuse(row_source=P, weights=None, table=P, nd=2, K=3, boxes=P, lq=P, var=P, mem=P, pat=P, box_mode=0, rows=64, counts=P):
        return L.pe_proben_fuse_batch_presence(boxes, P, P, P, P, row_source, P, None, None, 1, K, rows, box_mode, 0.5, 640.0, 512.0, None,
                                               weights, table, nd, P, P, P, P, counts, None, lq, var, mem, pat, None)
    assert fuse(boxes=None) == -1 and f"{who}: null input pointer" in err()
    assert fuse(counts=None) == -1 and f"{who}: null output pointer" in err()
    assert fuse(row_source=None) == -1 and "row_source / presence" in err()
    assert fuse(table=None) == -1 and "row_source / presence" in err()
    assert fuse(row_source=None, weights=P) == -1 and "row_source" in err()
    for nd in (0, 5):
        assert fuse(nd=nd) == -1 and f"num_detectors {nd} not in [1,4]" in err()
        assert fuse(nd=nd, weights=P) == -1 and f"num_detectors {nd} not in [1,4]" in err()
    for kw in ({"lq": None}, {"var": None}, {"mem": None}, {"lq": None, "var": None}, {"var": None, "mem": None}, {"lq": None, "mem": None}):
        assert fuse(**kw) == -1 and "out_log_posterior / out_vars / out_members go together" in err()
    assert fuse(K=63) == -1 and "num_classes 63 not in [1,62]" in err()
    assert fuse(box_mode=4) == -1 and "bad box_mode 4" in err()
    assert fuse(rows=0) == -1 and "max_rows_per_image 0 not in [1,2048]" in err()
    assert fuse(rows=2000) == -2 and "LDS" in err()
    assert L.pe_proben_fuse_batch_presence(None, None, None, None, None, None, None, None, None, 0, 3, 64, 0, 0.5, 640.0, 512.0, None, None,
                                           None, 0, None, None, None, None, None, None, None, None, None, None, None) == 0      # no image

    cand = (ctypes.c_double * (65 * 17))()

    def nll(base=P, labels=P, C=8, k1=4, c=cand, n_c=3, work=P, out=P, flags=P):
        return L.pe_bias_nll(base, labels, C, k1, c, n_c, work, out, flags, None)
    who = "pe_bias_nll"
    for n_c in (0, 65):
        assert nll(n_c=n_c) == -1 and f"{who}: num_candidates {n_c} not in [1,64]" in err()
    assert nll(k1=17) == -2 and "num_columns 17 (K + 1) above 16" in err()
    assert nll(k1=1) == -1 and "num_columns 1 (K + 1) < 2" in err()
    assert nll(c=None) == -1 and "null pointer (candidates)" in err()
    assert nll(C=-1) == -1 and "num_clusters -1 < 0" in err()
    for kw in ({"work": None}, {"out": None}, {"flags": None}):
        assert nll(**kw) == -1 and "null pointer (workspace / out / out_flags)" in err()
    for kw in ({"base": None}, {"labels": None}):
        assert nll(**kw) == -1 and "null pointer (base / labels)" in err()
    cand[5] = float("nan")
    assert nll() == -1 and "candidate entry nan (candidate 1, column 1) is not finite" in err()
    cand[5] = float("inf")
    assert nll() == -1 and "is not finite" in err()


# ---- the host side ----------------------------------------------------------------------------------------------------------------

NAMES = ["thermal_only", "early_fusion"]
TEXT = "thermal_only=-0.1:-0.9:0:0,early_fusion=-1.3:0:0.3:0,thermal_only+early_fusion=1.6:1.5:1.1:0"


def test_parse_presence():
    from proben_amd.calibration import parse_presence
    t = parse_presence(TEXT, NAMES)
    assert t.dtype == np.float64 and t.tolist() == [[0, 0, 0, 0], [-0.1, -0.9, 0, 0], [-1.3, 0, 0.3, 0], [1.6, 1.5, 1.1, 0]]
    assert parse_presence(TEXT, NAMES[::-1]).tolist() == t[[0, 2, 1, 3]].tolist()                 # a detector's bit is its position
    assert parse_presence("early_fusion+thermal_only=1:2:3:0", NAMES).tolist() == [[0] * 4, [0] * 4, [0] * 4, [1, 2, 3, 0]]
    three = parse_presence("a+c=1:0", ["a", "b", "c"])
    assert three.shape == (8, 2) and three[5].tolist() == [1, 0] and not three[[0, 1, 2, 3, 4, 6, 7]].any()
    with pytest.raises(ValueError, match="unknown detector 'middle_fusion'"):
        parse_presence("middle_fusion=0:0:0:0", NAMES)
    with pytest.raises(ValueError, match="lists pattern thermal_only\\+early_fusion twice"):
        parse_presence("thermal_only+early_fusion=0:0:0:0,early_fusion+thermal_only=1:1:1:0", NAMES)
    with pytest.raises(ValueError, match="names thermal_only twice"):
        parse_presence("thermal_only+thermal_only=0:0:0:0", NAMES)
    with pytest.raises(ValueError, match="lists 3 entries for K \\+ 1 = 4 columns"):
        parse_presence("thermal_only=0:0:0:0,early_fusion=1:1:0", NAMES)
    with pytest.raises(ValueError, match="lists 4 entries for K \\+ 1 = 2 columns"):
        parse_presence(TEXT, NAMES, num_columns=2)
    for bad in ("nan", "inf", "-inf"):
        with pytest.raises(ValueError, match="not finite"):
            parse_presence(f"thermal_only=0:{bad}:0:0", NAMES)
    with pytest.raises(ValueError, match="not a ':' separated list of numbers"):
        parse_presence("thermal_only=0:x:0:0", NAMES)
    with pytest.raises(ValueError, match="not pattern=v:v"):
        parse_presence("0:0:0:0", NAMES)


def test_check_presence_and_table_shapes():
    from proben_amd.calibration import check_presence
    assert check_presence(np.zeros((4, 4)), 2, 4).shape == (4, 4)
    row0 = np.zeros((4, 2))
    row0[0] = [7.0, -7.0]                         # row 0 is present and ignored: any finite numbers
    assert check_presence(row0, 2, 2)[0].tolist() == [7.0, -7.0]
    for bad, msg in ((np.zeros((3, 4)), "has 3 rows"), (np.zeros((32, 4)), "has 32 rows"), (np.zeros((4, 1)), "K \\+ 1 >= 2"),
                     (np.zeros(4), "K \\+ 1 >= 2"), ([[0.0, float("nan")]] * 2, "not finite"), ("abc", "not a table of numbers")):
        with pytest.raises(ValueError, match=msg):
            check_presence(bad)
    with pytest.raises(ValueError, match="has 4 rows for 3 detectors"):
        check_presence(np.zeros((4, 4)), 3)
    with pytest.raises(ValueError, match="has 4 columns for K \\+ 1 = 2"):
        check_presence(np.zeros((4, 4)), 2, 2)


def test_save_load_round_trip(tmp_path):
    from proben_amd import calibration as C
    table = C.parse_presence(TEXT, NAMES)
    rec = {"detectors": NAMES, "columns": 4, "table": table.tolist(), "hi": 16.0}
    with_key, without = tmp_path / "a.json", tmp_path / "b.json"
    C.save(str(with_key), {"thermal_only": 1.4, "early_fusion": 0.9}, presence=rec)
    C.save(str(without), {"thermal_only": 1.4, "early_fusion": 0.9})
    got = C.load(str(with_key))
    assert got["presence"] == rec and "presence" not in C.load(str(without)) and "presence" not in json.load(open(without))
    assert C.resolve_presence(got["presence"], NAMES, "a.json").tolist() == table.tolist()
    assert C.resolve_presence(got["presence"], NAMES[::-1], "a.json").tolist() == table[[0, 2, 1, 3]].tolist()
    with pytest.raises(ValueError, match="is over thermal_only,early_fusion, not thermal_only,middle_fusion"):
        C.resolve_presence(got["presence"], ["thermal_only", "middle_fusion"], "a.json")
    bad = json.load(open(with_key))
    bad["presence"]["table"][1][0] = float("nan")
    json.dump(bad, open(with_key, "w"))
    with pytest.raises(ValueError, match="not finite"):
        C.load(str(with_key))
    with pytest.raises(ValueError, match="has 4 rows for 3 detectors"):
        C.save(str(with_key), {"a": 1.0}, presence={"detectors": ["a", "b", "c"], "columns": 4, "table": table.tolist()})


def test_keyword_and_flag_are_refused_outside_proben_log():
    from proben_amd import fusion as F
    from proben_amd.cli import demo_probEn
    from proben_amd.late_fusion import late_fusion
    from proben_amd.opt import config_parser
    from proben_amd.pipeline import FramePairPipeline
    z = torch.zeros((0, 4), dtype=torch.float64)
    table = np.zeros((4, 4))
    msg = "presence belongs to score_fusion 'probEn-log' \\(got '{}'\\): the other score fusions have no log-evidence to add it to"
    for mode in ("probEn", "avg", "max", "probEn_binary"):
        with pytest.raises(ValueError, match="fuse_batch: " + msg.format(mode)):
            F.fuse_batch(z, z[:, 0], z[:, :3], z[:, 0], z[:, 0].int(), torch.zeros(1, dtype=torch.int32), score_fusion=mode, presence=table)
        with pytest.raises(ValueError, match="fuse_detections: " + msg.format(mode)):
            F.fuse_detections([], mode, presence=table)
        with pytest.raises(ValueError, match="late_fusion: " + msg.format(mode)):
            late_fusion([], [mode, "v-avg"], presence=table)
        with pytest.raises(ValueError, match="FramePairPipeline: " + msg.format(mode)):
            FramePairPipeline([], mode, presence=table)
    with pytest.raises(ValueError, match="presence needs row_source"):
        F.fuse_batch(z, z[:, 0], None, z[:, 0], z[:, 0].int(), torch.zeros(1, dtype=torch.int32), score_fusion="probEn-log", log_probs=z,
                     presence=table)
    with pytest.raises(ValueError, match="has 4 rows for 3 detectors"):
        FramePairPipeline([None, None, None], "probEn-log", presence=table)
    for mode in ("probEn", "avg", "max"):
        with pytest.raises(SystemExit):
            config_parser(["--presence", TEXT, "--score_fusion", mode])
    with pytest.raises(SystemExit):
        demo_probEn.main(["--presence", TEXT, "--score_fusion", "probEn", "--dataset_path", "d", "--prediction_path", "p"])
    assert config_parser(["--presence", TEXT, "--score_fusion", "probEn-log"]).presence == TEXT
    assert config_parser([]).presence is None
