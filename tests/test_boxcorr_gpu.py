"""Correlated box fusion on the GPU: pe_box_gls_batch against the dense longdouble solve, pe_box_pair_stats against its NumPy
restatement, the fit end to end and the drivers.  References and the constant C_GLS live in tests/test_boxcorr_cpu.py; the bounds are
derived in DESIGN.md section 19.  u = 2^-53."""
import json
import math
import os

import numpy as np
import pytest
import torch

from fuse_inputs import GRID, batch, grid_image, to_dev, weights, write_flir
from fuse_ref import clusters
from test_boxcorr_cpu import (C_GLS, LD, U, cluster_correlation, estimate_numpy, pair_stats_numpy, restate, simulate_pairs,
                              detection_with_residual)

pytestmark = pytest.mark.gpu

SEQ = 1000         # a row bound at which the bit matrices do not fit the LDS: the sequential clustering


def _matrix(D, off, diag):
    P = np.full((D, D), off)
    np.fill_diagonal(P, diag)
    return P


def _matrices(D):
    """The issue's two - moderate (0.5 beside a diagonal of 0.2) and near-singular (0.95 beside 0.9) - and one that is itself positive
    semidefinite (0.5 beside 0.6), under which every composition of rows has a positive definite R."""
    return {"moderate": _matrix(D, 0.5, 0.2), "near-singular": _matrix(D, 0.95, 0.9), "psd": _matrix(D, 0.5, 0.6)}


def _images(rng, k1, D):
    """8 images of 2 to 64 rows with clusters of 2 to 12 members (sources cycle, so a cluster larger than D holds several rows of one
    detector) and single rows; variances log-uniform over two decades."""
    plans = [([2], 0), ([2, 3], 2), ([4, 5, 6], 1), ([7, 8, 9, 2], 3), ([10, 11, 12, 2, 2], 4), ([12, 3, 2, 2, 4], 0), ([2, 2, 2, 3, 3], 5),
             ([12, 12, 11, 9, 8, 6, 2], 4)]
    images = []
    for sizes, single in plans:
        im = grid_image(rng, sizes, k1, D, n_single=single)
        im["vars"] = 10.0 ** rng.uniform(-1.0, 1.0, len(im["scores"]))
        assert 2 <= len(im["scores"]) <= 64
        images.append(im)
    return images


def _members(im):
    """[(fused row k, the cluster's rows in ascending input-row order)], from the restated greedy clustering."""
    return [(k, sorted(mem)) for k, (_, mem) in enumerate(clusters(im["boxes"], im["scores"], im["classes"].astype(np.float64)))]


def _check_cluster(ref, m, got_box, got_var, frac):
    """One fused row against `restate`: boxes within C_GLS cond(R) u X plus the (2 m + 1) X u of the weighted sum, X = sum_t |coord_t
    lambda_t|; the variance within C_GLS cond(R) u relative (when the run wrote one).  frac collects the largest fractions."""
    X = np.abs(ref["coords"].astype(LD) * ref["lam"][:, None]).sum(0).astype(np.float64)
    tol = (C_GLS * ref["cond"] + 2 * m + 1) * U * X
    err = np.abs(got_box.astype(LD) - ref["box"]).astype(np.float64)
    frac["box"] = max(frac["box"], float((err / tol).max()))
    assert np.all(err <= tol), (m, ref["cond"], err, tol)
    if got_var is not None:
        rel = float(abs(LD(got_var) - ref["var"]) / abs(ref["var"]))
        tolv = C_GLS * ref["cond"] * U
        frac["var"] = max(frac["var"], rel / tolv)
        assert rel <= tolv, (m, ref["cond"], rel, tolv)


def _same(x, y):
    """Equal bytes (the NaN the wrapper prefills compares equal to itself)."""
    return x.shape == y.shape and x.dtype == y.dtype and x.contiguous().cpu().numpy().tobytes() == y.contiguous().cpu().numpy().tobytes()


SAME = ("scores", "classes", "keep", "counts", "cluster", "log_posterior", "members", "pattern")
LIVE_ONLY = ("scores", "classes", "keep")


@pytest.mark.parametrize("D,k1", [(2, 2), (3, 4), (4, 4), (4, 2)])
def test_fusion_against_the_dense_solve(D, k1):
    from proben_amd import fusion as F
    rng = np.random.default_rng(190 + 10 * D + k1)
    images = _images(rng, k1, D)
    (b, s, v, c, offs_d, src, lp), offs = batch(images)
    members = [_members(im) for im in images]
    weights = rng.uniform(0.3, 1.5, D).tolist()
    table = rng.normal(0, 1, (2 ** D, k1))
    frac = {"box": 0.0, "var": 0.0}
    seen, checked, not_pd, undecided = set(), 0, 0, 0
    live = np.zeros(offs[-1], bool)
    for i in range(len(images)):
        live[offs[i]:offs[i] + len(members[i])] = True
    live = to_dev(live)
    for name, P in _matrices(D).items():
        refs = {}
        for i, im in enumerate(images):
            for k, mem in members[i]:
                if len(mem) >= 2:
                    refs[(i, k)] = dict(restate(im["boxes"][mem], im["vars"][mem], im["src"][mem], P), coords=im["boxes"][mem],
                                        low=float(np.linalg.eigvalsh(cluster_correlation(im["src"][mem], P))[0]))
        for pool in (None, weights):
            for pres in (None, table):
                for post in (False, True):
                    for bound in (None, SEQ):
                        kw = dict(max_rows=bound, log_probs=lp, pool_weights=pool, presence=pres, with_posterior=post, row_source=src)
                        if pool is None and pres is None:
                            base = F.fuse_batch(b, s, None, v, c, offs_d, "probEn-log", "v-avg", **dict(kw, row_source=None))
                        else:
                            base = F.fuse_batch(b, s, None, v, c, offs_d, "probEn-log", "v-avg", **kw)
                        got = F.fuse_batch(b, s, None, v, c, offs_d, "probEn-log", "c-avg", box_correlation=P, **kw)
                        for key in SAME:
                            if key in base:      # scores / classes / keep are uninitialised beyond counts[b]: the fused rows only
                                x, y = (base[key], got[key]) if key not in LIVE_ONLY else (base[key][live], got[key][live])
                                assert _same(x, y), (name, key, pool is not None, pres is not None, post, bound)
                        gb = got["boxes"].cpu().numpy()
                        gv = got["vars"].cpu().numpy() if post else None
                        bb = base["boxes"].cpu().numpy()
                        bv = base["vars"].cpu().numpy() if post else None
                        for i, im in enumerate(images):
                            assert int(got["counts"][i]) == len(members[i])
                            for k, mem in members[i]:
                                o = offs[i] + k
                                if len(mem) == 1:      # a cluster of one never reads the matrix: the v-avg run's bytes
                                    assert gb[o].tobytes() == bb[o].tobytes() and (gv is None or gv[o].tobytes() == bv[o].tobytes())
                                    continue
                                ref = refs[(i, k)]
                                seen.add(len(mem))
                                if ref["low"] < -1e-9:       # R is not positive definite: no such distribution, NaN
                                    assert np.isnan(gb[o]).all() and (gv is None or np.isnan(gv[o])), (name, i, k, ref["low"])
                                    not_pd += 1
                                elif ref["low"] <= 1e-9:     # singular to rounding: either answer, nothing to compare with
                                    undecided += 1
                                else:
                                    _check_cluster(ref, len(mem), gb[o], None if gv is None else gv[o], frac)
                                    checked += 1
    print(f"[boxcorr] D={D} K+1={k1}: {checked} cluster checks (sizes {sorted(seen)}), {not_pd} with R not positive definite (NaN), "
          f"{undecided} singular to rounding; largest fraction of the bound: boxes {frac['box']:.4f}, vars {frac['var']:.4f}")
    assert set(range(2, 13)) <= seen and checked >= 1000 and frac["box"] > 0


def test_zero_matrix_is_v_avg():
    from proben_amd import fusion as F
    D, k1 = 3, 4
    rng = np.random.default_rng(77)
    images = _images(rng, k1, D)
    (b, s, v, c, offs_d, src, lp), offs = batch(images)
    passthrough = np.zeros(len(images), np.int32)
    passthrough[1] = 1
    kw = dict(log_probs=lp, with_posterior=True, row_source=src, pool_weights=[1.0] * D, row_counts=to_dev(np.diff(offs).astype(np.int32)),
              passthrough=to_dev(passthrough), max_rows=64)
    base = F.fuse_batch(b, s, None, v, c, offs_d[:-1], "probEn-log", "v-avg", **kw)
    zero = F.fuse_batch(b, s, None, v, c, offs_d[:-1], "probEn-log", "c-avg", box_correlation=np.zeros((D, D)), **kw)
    other = F.fuse_batch(b, s, None, v, c, offs_d[:-1], "probEn-log", "c-avg", box_correlation=_matrix(D, 0.5, 0.6), **kw)
    bb, bv, mem_n = base["boxes"].cpu().numpy(), base["vars"].cpu().numpy(), base["members"].cpu().numpy()
    two = larger = ones = 0
    worst = {"box": 0.0, "var": 0.0}
    for i, im in enumerate(images):
        cnt = int(base["counts"][i])
        assert cnt == int(zero["counts"][i]) == int(other["counts"][i])
        if passthrough[i]:
            assert cnt == len(im["scores"])
        clusters = dict(_members(im)) if not passthrough[i] else {}
        for k in range(cnt):
            o = offs[i] + k
            zb, zv = zero["boxes"][o].cpu().numpy(), zero["vars"][o].cpu().numpy()
            if mem_n[o] == 1:                    # clusters of one and passthrough rows: equal bytes under every matrix
                for run in (zero, other):
                    assert run["boxes"][o].cpu().numpy().tobytes() == bb[o].tobytes() and run["vars"][o].cpu().numpy().tobytes() == bv[o].tobytes()
                ones += 1
            elif mem_n[o] == 2:                  # a sum of two is commutative and y_t = 1 / var_t is exact: the v-avg bytes
                assert zb.tobytes() == bb[o].tobytes() and zv.tobytes() == bv[o].tobytes(), (i, k)
                two += 1
            else:                                # the order of the sums differs: within v-avg's own bound (section 17) of the exact value
                mem = clusters[k]
                m = len(mem)
                ref = restate(im["boxes"][mem], im["vars"][mem], im["src"][mem], np.zeros((D, D)))
                X = np.abs(im["boxes"][mem].astype(LD) * ref["lam"][:, None]).sum(0).astype(np.float64)
                err = np.abs(zb.astype(LD) - ref["box"]).astype(np.float64)
                rel = float(abs(LD(float(zv)) - ref["var"]) / ref["var"])
                worst["box"] = max(worst["box"], float((err / ((2 * m + 1) * U * X)).max()))
                worst["var"] = max(worst["var"], rel / ((m + 3) * U))
                assert np.all(err <= (2 * m + 1) * U * X) and rel <= (m + 3) * U, (i, k, m)
                larger += 1
    print(f"[boxcorr] zero matrix: {two} clusters of two with the v-avg bytes, {larger} larger ones at {worst['box']:.3f} (boxes) and "
          f"{worst['var']:.3f} (vars) of v-avg's bound, {ones} single rows unchanged")
    assert two >= 8 and larger >= 15 and ones >= 10


def _tile_image(rng, k1, D):
    """1 060 rows, more than one LDS tile of pe_box_gls_batch (1 024): 500 clusters of two and 20 of three, a class per band so that 540
    anchors exist; the rows are permuted, so clusters straddle the tile boundary."""
    sizes = [2] * 500 + [3] * 20
    box, src, cls = [], [], []
    slots = [(a, k) for k in range(3) for a in range(len(GRID))]
    for j, m in enumerate(sizes):
        a, k = slots[j]
        x, y = GRID[a]
        for t in range(m):
            box.append(np.array([x, y, x + 20, y + 20], np.float64) + rng.integers(-1, 2, 4))
            src.append((t + j) % D)
            cls.append(k)
    n = len(box)
    perm = rng.permutation(n)
    lp = np.log(rng.dirichlet(np.ones(k1), n))
    return {"boxes": np.asarray(box)[perm], "scores": rng.uniform(0.1, 0.9, n)[perm], "lp": lp, "src": np.asarray(src, np.int32)[perm],
            "vars": 10.0 ** rng.uniform(-1.0, 1.0, n), "classes": np.asarray(cls, np.int32)[perm]}


def test_edges():
    """counts == -1, a passthrough image, an image of more than one LDS tile, an empty image, a row of an unknown detector, and the
    elements beyond counts[b]."""
    from proben_amd import _lib
    from proben_amd import fusion as F
    D, k1 = 2, 4
    rng = np.random.default_rng(11)
    P = _matrix(D, 0.5, 0.6)
    over = {"boxes": rng.uniform(0, 400, (1101, 4)), "scores": rng.uniform(0, 1, 1101), "lp": np.log(rng.dirichlet(np.ones(k1), 1101)),
            "src": np.zeros(1101, np.int32), "vars": np.ones(1101), "classes": np.zeros(1101, np.int32)}
    single = grid_image(rng, [2, 3], k1, D, n_single=2)
    tile = _tile_image(rng, k1, D)
    empty = grid_image(rng, [], k1, D)
    bad = grid_image(rng, [3, 2, 4], k1, D, n_single=2)
    images = [over, single, tile, empty, bad]
    bad_members = _members(bad)
    victim = next(mem for _, mem in bad_members if len(mem) == 3)[1]
    bad["src"][victim] = D                                        # outside [0, D)
    (b, s, v, c, offs_d, src, lp), offs = batch(images)
    passthrough = np.zeros(len(images), np.int32)
    passthrough[1] = 1
    kw = dict(max_rows=1100, log_probs=lp, with_posterior=True, row_source=src, row_counts=to_dev(np.diff(offs).astype(np.int32)),
              passthrough=to_dev(passthrough))
    # unit pool weights: the entry point that writes "cluster"; a row of an unknown detector then has a NaN score in BOTH runs (POOL)
    base = F.fuse_batch(b, s, None, v, c, offs_d[:-1], "probEn-log", "v-avg", pool_weights=[1.0] * D, **kw)
    got = F.fuse_batch(b, s, None, v, c, offs_d[:-1], "probEn-log", "c-avg", box_correlation=P, pool_weights=[1.0] * D, **kw)
    torch.cuda.synchronize()
    for key in ("counts", "cluster", "members", "log_posterior"):
        assert _same(base[key], got[key]), key
    cnt = got["counts"].cpu().numpy()
    live = np.zeros(offs[-1], bool)
    for i in range(len(images)):
        live[offs[i]:offs[i] + max(cnt[i], 0)] = True
    for key in ("keep", "classes", "scores"):      # uninitialised beyond counts[b]; a NaN score (the unknown detector) compares by bytes
        assert base[key].cpu().numpy()[live].tobytes() == got[key].cpu().numpy()[live].tobytes(), key
    assert cnt[0] == -1 and cnt[1] == len(single["scores"]) and cnt[2] == 520 and cnt[3] == 0
    gb, gv, bb, bv = (x.cpu().numpy() for x in (got["boxes"], got["vars"], base["boxes"], base["vars"]))
    mem_n = got["members"].cpu().numpy()
    # counts == -1 and beyond counts[b]: the variance keeps the wrapper's NaN sentinel
    assert np.isnan(gv[offs[0]:offs[1]]).all()
    for i in range(1, len(images)):
        assert np.isnan(gv[offs[i] + cnt[i]:offs[i + 1]]).all()
    # the passthrough image: the v-avg run's bytes (its own rows)
    sl = slice(offs[1], offs[2])
    assert gb[sl].tobytes() == bb[sl].tobytes() == single["boxes"].tobytes() and gv[sl].tobytes() == bv[sl].tobytes()
    # more than one tile: every cluster against the dense solve
    frac = {"box": 0.0, "var": 0.0}
    crossing = 0
    for k, mem in _members(tile):
        assert len(mem) in (2, 3)
        crossing += int(mem[0] < 1024 <= mem[-1])
        ref = dict(restate(tile["boxes"][mem], tile["vars"][mem], tile["src"][mem], P), coords=tile["boxes"][mem])
        _check_cluster(ref, len(mem), gb[offs[2] + k], gv[offs[2] + k], frac)
    assert crossing >= 10
    # the unknown detector: its cluster NaN, every other cluster of the image as without it
    for k, mem in bad_members:
        o = offs[4] + k
        if victim in mem:
            assert np.isnan(gb[o]).all() and np.isnan(gv[o]) and not np.isnan(bb[o]).any()
        elif len(mem) == 1:
            assert gb[o].tobytes() == bb[o].tobytes()
        else:
            ref = dict(restate(bad["boxes"][mem], bad["vars"][mem], bad["src"][mem], P), coords=bad["boxes"][mem])
            _check_cluster(ref, len(mem), gb[o], gv[o], frac)
    # the entry point itself on sentinel-filled outputs: only fused rows of two or more members are written
    ob = torch.full_like(got["boxes"], 12345.0)
    ov = torch.full_like(got["vars"], 54321.0)
    st = _lib.lib().pe_box_gls_batch(_lib.ptr(b), _lib.ptr(v), _lib.ptr(src), _lib.ptr(got["cluster"]), _lib.ptr(offs_d[:-1].contiguous()),
                                     _lib.ptr(kw["row_counts"]), _lib.ptr(got["counts"]), len(images), 1100,
                                     _lib.ptr(to_dev(P)), D, _lib.ptr(ob), _lib.ptr(ov), _lib.stream())
    assert st == 0
    ob, ov = ob.cpu().numpy(), ov.cpu().numpy()
    written = np.zeros(len(ov), bool)
    for i in (2, 4):
        written[offs[i]:offs[i] + cnt[i]] = mem_n[offs[i]:offs[i] + cnt[i]] >= 2
    assert (ob[~written] == 12345.0).all() and (ov[~written] == 54321.0).all()
    keep = written & ~np.isnan(gv)
    assert ob[keep].tobytes() == gb[keep].tobytes() and ov[keep].tobytes() == gv[keep].tobytes()
    assert np.isnan(ob[written & np.isnan(gv)]).all()
    # without an out_vars only the boxes are written
    ob2 = torch.full_like(got["boxes"], 12345.0)
    st = _lib.lib().pe_box_gls_batch(_lib.ptr(b), _lib.ptr(v), _lib.ptr(src), _lib.ptr(got["cluster"]), _lib.ptr(offs_d[:-1].contiguous()),
                                     _lib.ptr(kw["row_counts"]), _lib.ptr(got["counts"]), len(images), 1100,
                                     _lib.ptr(to_dev(P)), D, _lib.ptr(ob2), None, _lib.stream())
    assert st == 0 and ob2.cpu().numpy().tobytes() == ob.tobytes()
    print(f"[boxcorr] edges: {crossing} clusters straddle the tile boundary; largest fraction of the bound: boxes {frac['box']:.4f}, "
          f"vars {frac['var']:.4f}")


def _pair_case(rng, C, D):
    """C clusters of 1 to 6 members over shuffled rows, residuals drawn like the simulation's; about one cluster in eight without a
    ground-truth box; members with a degenerate box, a zero / NaN / infinite variance and a source outside [0, D)."""
    sizes = rng.integers(1, 7, C)
    M = int(sizes.sum())
    cluster_offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    G = C + 3
    x1, y1 = rng.uniform(0, 400, G), rng.uniform(0, 300, G)
    gt = np.stack([x1, y1, x1 + rng.uniform(20, 200, G), y1 + rng.uniform(20, 200, G)], 1)
    match = rng.permutation(G)[:C].astype(np.int32)
    match[rng.uniform(size=C) < 0.125] = -1
    N = M + 5                                            # a few rows no cluster uses
    member_rows = rng.permutation(N)[:M].astype(np.int32)
    var = 10.0 ** rng.uniform(-3.0, -1.0, N)
    src = rng.integers(0, D, N).astype(np.int32)
    det = rng.uniform(0, 300, (N, 4))
    det[:, 2:] += det[:, :2] + 5
    for c in range(C):
        rows = member_rows[cluster_offsets[c]:cluster_offsets[c + 1]]
        g = max(int(match[c]), 0)
        shared = rng.standard_normal(4)
        z = 0.7 * shared[None] + 0.7 * rng.standard_normal((len(rows), 4))
        det[rows] = detection_with_residual(np.repeat(gt[g][None], len(rows), 0), z * np.sqrt(var[rows])[:, None])
    if C > 1:
        gt[int(match[match >= 0][0])] = [5.0, 5.0, 5.0, 50.0]            # a degenerate ground-truth box: its members are excluded
    for j, row in enumerate(member_rows[::7][:40]):
        kind = j % 6
        if kind == 0:
            det[row, 2] = det[row, 0] - 1.0
        elif kind == 1:
            var[row] = 0.0
        elif kind == 2:
            var[row] = np.nan
        elif kind == 3:
            var[row] = np.inf
        elif kind == 4:
            src[row] = D
        else:
            src[row] = -1
    return det, var, src, member_rows, cluster_offsets, match, gt


@pytest.mark.parametrize("C", [1, 257, 5000])
def test_pair_stats_against_the_restatement(C):
    """Counts and flags exact; S and Q within the chain bound of the stated summation order: a term within 22 u (section 12's q-type
    term; DESIGN.md section 19 writes the product's out), one u per addition along the longest chain a term takes part in, one for fsum
    and a ceiling - (24 + chain) u sum |terms|."""
    from proben_amd import calibration as cal
    D = 3
    rng = np.random.default_rng(C)
    det, var, src, member_rows, cluster_offsets, match, gt = _pair_case(rng, C, D)
    pairs, rows, S, Q, excluded, S_abs, Q_abs, last = pair_stats_numpy(det, var, src, member_rows, cluster_offsets, match, gt, D)
    args = [to_dev(x) for x in (det, var, src, member_rows, cluster_offsets, match, gt)]
    got = cal.box_pair_stats(*args, D)
    again = cal.box_pair_stats(*args, D)
    assert got["pairs"].tolist() == pairs.tolist() and list(got["rows"]) == rows
    assert got["excluded"] == excluded and got["last_excluded"] == last
    assert got["S"].tobytes() == again["S"].tobytes() and np.array(got["Q"]).tobytes() == np.array(again["Q"]).tobytes()
    blocks = min((C + 255) // 256, 1024)
    per_thread = (C + blocks * 256 - 1) // (blocks * 256)              # clusters a thread adds
    chain_s = 15 * per_thread + 8 + (blocks + 15) // 16 + 16          # 6 members: 15 pairs of one slot at most; the tree; the finish
    chain_q = 6 * per_thread + 8 + (blocks + 15) // 16 + 16
    worst = 0.0
    for a in range(D):
        tol = (24 + chain_q) * U * Q_abs[a]
        err = abs(got["Q"][a] - Q[a])
        worst = max(worst, err / tol if tol else 0.0)
        assert err <= tol, ("Q", a, err, tol)
        for b2 in range(a, D):
            tol = (24 + chain_s) * U * S_abs[a, b2]
            err = abs(got["S"][a, b2] - S[a, b2])
            worst = max(worst, err / tol if tol else 0.0)
            assert err <= tol, ("S", a, b2, err, tol)
            assert got["S"][a, b2] == got["S"][b2, a]
    print(f"[boxcorr] pair stats, {C} clusters: {int(np.triu(pairs).sum())} pairs, {sum(rows)} rows, {excluded} excluded; largest error "
          f"{worst:.4f} of the chain bound")
    if C > 1:
        assert excluded >= 10 and int(np.triu(pairs).sum()) > C


def test_pair_stats_of_nothing():
    from proben_amd import calibration as cal
    z4, z1 = torch.zeros((0, 4), dtype=torch.float64, device="cuda"), torch.zeros((0,), dtype=torch.float64, device="cuda")
    i0 = torch.zeros((0,), dtype=torch.int32, device="cuda")
    got = cal.box_pair_stats(z4, z1, i0, i0, torch.zeros((1,), dtype=torch.int32, device="cuda"), i0, z4, 2)
    assert got["pairs"].tolist() == [[0, 0], [0, 0]] and list(got["rows"]) == [0, 0] and got["excluded"] == 0
    est = cal.box_correlation_estimate(got["pairs"], got["rows"], got["S"], got["Q"])
    assert est["matrix"] == [[0.0, 0.0], [0.0, 0.0]] and est["empty"] == [[0, 0], [0, 1], [1, 1]]


def test_fit_box_correlation_end_to_end():
    from proben_amd import calibration as cal
    rng = np.random.default_rng(1002)
    n = 20000
    det, var, src, gt = simulate_pairs(rng, n, 0.6)
    member_rows = np.arange(2 * n, dtype=np.int32)
    cluster_offsets = np.arange(0, 2 * n + 1, 2, dtype=np.int32)
    match = np.arange(n, dtype=np.int32)
    fit = cal.fit_box_correlation(*[to_dev(x) for x in (det, var, src, member_rows, cluster_offsets, match, gt)], 2)
    pairs, rows, S, Q, excluded, _, _, _ = pair_stats_numpy(det, var, src, member_rows, cluster_offsets, match, gt, 2)
    want = estimate_numpy(pairs, rows, S, Q)
    assert fit["pairs"] == [[0, n], [n, 0]] and fit["rows"] == [n, n] and fit["excluded"] == excluded == 0
    assert abs(fit["matrix"][0][1] - want[0, 1]) <= 1e-12 and fit["matrix"][0][1] == fit["matrix"][1][0] == fit["raw"][0][1]
    assert fit["matrix"][0][0] == fit["matrix"][1][1] == 0.0 and fit["shrink"] == 1.0 and fit["empty"] == [[0, 0], [1, 1]]
    se = math.sqrt((1 + 0.36) / (4 * n))
    assert abs(fit["matrix"][0][1] - 0.6) <= 4 * se
    assert fit["stderr"][0][1] == pytest.approx(math.sqrt((1 + fit["matrix"][0][1] ** 2) / (4 * n)))
    print(f"[boxcorr] fit end to end: rho_hat {fit['matrix'][0][1]:.5f} ({(fit['matrix'][0][1] - 0.6) / se:+.2f} standard errors), "
          f"NumPy estimator differs by {abs(fit['matrix'][0][1] - want[0, 1]):.2e}")


def test_drivers(tmp_path, capsys):
    """save_predictions x 2 -> fit_temperature --with-variance --with-box-correlation -> demo_probEn --box_fusion c-avg --calibration (the
    two-stage route and --one-pass write the same fused file, with the c-avg variance) -> calibration_report --fused-posterior (both box
    rules side by side); a file without the key, and a run without the flag, leave everything as it is."""
    from proben_amd import calibration as Cal
    from proben_amd.cli import calibration_report, demo_probEn, fit_temperature, save_predictions
    from proben_amd.late_fusion import late_fusion, read_j1
    root = tmp_path / "val"
    write_flir(root, 6, 96, 120, (150, 180))
    names = ["thermal_only", "early_fusion"]
    paths = [weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
    pdir = tmp_path / "pred"
    for m, p in zip(names, paths):
        save_predictions.main(["--dataset_path", str(root), "--fusion_method", m, "--model_path", p, "--prediction_path", str(pdir), "--batch", "4"])
    files = [str(pdir / f"val_{m}_predictions.json") for m in names]
    # annotations rewritten from the detections so that rows match (the recipe of tests/test_posterior_gpu.py)
    preds = [json.load(open(f)) for f in files]
    val = root / "FLIR_thermal_RGBT_pairs_val.json"
    ds = json.load(open(val))
    anns = []
    for i, iid in enumerate(preds[0]["image_id"]):
        for k, p in enumerate(preds):
            if p["boxes"][i]:
                x1, y1, x2, y2 = p["boxes"][i][0]
                anns.append({"id": len(anns) + 1, "image_id": iid, "category_id": 1 + int(p["classes"][i][0]) % 3,
                             "bbox": [x1 + 0.03 * (1 + k) * (x2 - x1), y1 - 0.02 * (y2 - y1), (x2 - x1) * 1.05, (y2 - y1) * 0.97],
                             "area": (x2 - x1) * (y2 - y1), "iscrowd": 0})
    assert anns
    ds["annotations"] = anns
    json.dump(ds, open(val, "w"))
    cal, plain_cal = tmp_path / "cal.json", tmp_path / "cal_plain.json"
    fit_args = ["--predictions", *files, "--dataset_path", str(root), "--holdout", "0.5", "--with-variance"]
    fit_temperature.main(fit_args + ["--out", str(plain_cal)])
    capsys.readouterr()
    fit_temperature.main(fit_args + ["--out", str(cal), "--with-box-correlation"])
    printed = capsys.readouterr().out
    with capsys.disabled():
        print(printed)
    rec = Cal.load(cal)
    bc = rec["box_correlation"]
    assert "box correlation (" in printed and "standard error" in printed and f"{names[0]}:{names[1]} = " in printed
    assert bc["detectors"] == names and bc["box_fusion"] == "v-avg" and bc["iou"] == 0.5
    assert {"matrix", "raw", "shrink", "pairs", "rows", "excluded", "stderr"} <= set(bc)
    Cal.check_box_correlation(bc["matrix"], 2)
    stripped = {k: v for k, v in json.load(open(cal)).items() if k != "box_correlation"}
    assert stripped == json.load(open(plain_cal))                     # the flag adds its key and changes nothing else
    with pytest.raises(SystemExit):
        fit_temperature.main(["--predictions", files[0], "--dataset_path", str(root), "--out", str(cal), "--with-box-correlation"])

    def demo(tag, extra, one_pass=False):
        out = tmp_path / f"out_{tag}"
        head = ["--one-pass", "--model_paths", ",".join(paths), "--workers", "2", "--batch", "4"] if one_pass else ["--prediction_path", str(pdir)]
        res = demo_probEn.main(head + ["--dataset_path", str(root), "--detectors", ",".join(names), "--outfolder", str(out), "--dataset_name",
                                       f"flir_boxcorr_{tag}", "--score_fusion", "probEn-log", "--write_fused", str(out / "fused.json")] + extra)
        return out, res

    # the fitted key is picked up, on both routes, and the routes write the same fused rows
    o2, r2 = demo("cal2", ["--box_fusion", "c-avg", "--calibration", str(cal)])
    o1, r1 = demo("cal1", ["--box_fusion", "c-avg", "--calibration", str(cal)], one_pass=True)
    assert r2["box_correlation"] == r1["box_correlation"] == {"detectors": names, "matrix": bc["matrix"]}
    assert read_j1(o2 / "fused.json") == read_j1(o1 / "fused.json") and (o2 / "fused.json").read_bytes() == (o1 / "fused.json").read_bytes()
    assert (o2 / "FLIR_probEn_eval.json").read_bytes() == (o1 / "FLIR_probEn_eval.json").read_bytes()
    # a matrix given on the command line: the fused file carries the c-avg variance, what late_fusion returns
    flag = ["--box_fusion", "c-avg", "--box_correlation", "0.6", "--calibration", str(cal)]
    of2, _ = demo("flag2", flag)
    of1, _ = demo("flag1", flag, one_pass=True)
    assert (of2 / "fused.json").read_bytes() == (of1 / "fused.json").read_bytes()
    ov, rv = demo("vavg", ["--calibration", str(cal)])
    assert "box_correlation" not in rv
    fc, fv = read_j1(of2 / "fused.json"), read_j1(ov / "fused.json")
    for key in ("image", "image_id", "scores", "classes", "class_logits", "probs"):
        assert fc[key] == fv[key], key
    temps = [rec["detectors"][m] for m in names]
    scales = [rec["variance_scales"][m] for m in names]
    direct = late_fusion([read_j1(f) for f in files], ["probEn-log", "c-avg"], temperatures=temps, names=files, variance_scales=scales,
                         with_posterior=True, box_correlation=[[0.0, 0.6], [0.6, 0.0]])
    moved = same = 0
    for i, r in enumerate(direct):
        if r is None:
            assert fc["vars"][i] == []
            continue
        keep = np.nonzero(np.asarray(r[2]) != 3)[0]                  # rows fused to the background column are not written
        assert [v[0] for v in fc["vars"][i]] == r[4][keep].tolist() and fc["boxes"][i] == r[0][keep].tolist()
        for (vc,), (vv,), m in zip(fc["vars"][i], fv["vars"][i], r[5][keep]):
            if m >= 2:                      # (two rows of ONE detector keep the v-avg value: their entry of the matrix is 0)
                moved += int(vc != vv)
            else:
                assert vc == vv
                same += 1
    assert moved > 0 and same > 0
    # a file without the key, and a run without the flag: the v-avg run's bytes
    op, rp = demo("plain", ["--calibration", str(plain_cal)])
    assert (op / "fused.json").read_bytes() == (ov / "fused.json").read_bytes()
    assert json.dumps(rp, sort_keys=True) == json.dumps(rv, sort_keys=True)          # (an AP without ground truth is NaN)
    assert (op / "FLIR_probEn_eval.json").read_bytes() == (ov / "FLIR_probEn_eval.json").read_bytes()
    assert (op / "coco_instances_results.json").read_bytes() == (ov / "coco_instances_results.json").read_bytes()
    with pytest.raises(ValueError, match="needs --box_correlation"):
        demo("none", ["--box_fusion", "c-avg", "--calibration", str(plain_cal)])
    with pytest.raises(SystemExit):
        demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names), "--box_fusion", "c-avg",
                          "--box_correlation", "0.6"])
    with pytest.raises(SystemExit):
        demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names), "--score_fusion",
                          "probEn-log", "--box_correlation", "0.6"])
    # the report: both box rules side by side under --fused-posterior; nothing new without the flag or without the key
    base = ["--dataset_path", str(root), "--predictions", *files, "--score_fusion", "probEn-log", "--on", "all"]
    capsys.readouterr()
    rep = calibration_report.main(base + ["--calibration", str(cal), "--fused-posterior"])
    printed = capsys.readouterr().out
    with capsys.disabled():
        print(printed)
    assert "v-avg: Gaussian NLL per matched fused row" in printed and "c-avg: Gaussian NLL per matched fused row" in printed
    both = rep["box_correlation"]
    assert both["matrix"] == bc["matrix"] and both["v-avg"] == rep["fused"]["after"]["variance"]
    assert both["c-avg"]["rows"] == both["v-avg"]["rows"] > 0 and all(0.0 <= c <= 1.0 for c in both["c-avg"]["coverage"])
    no_flag = calibration_report.main(base + ["--calibration", str(cal), "--out", str(tmp_path / "rep_key.json")])
    assert "box_correlation" not in no_flag and "c-avg: Gaussian" not in capsys.readouterr().out
    calibration_report.main(base + ["--calibration", str(plain_cal), "--out", str(tmp_path / "rep_plain.json")])
    assert (tmp_path / "rep_key.json").read_bytes() == (tmp_path / "rep_plain.json").read_bytes()
    no_key = calibration_report.main(base + ["--calibration", str(plain_cal), "--fused-posterior"])
    assert "box_correlation" not in no_key and "c-avg: Gaussian" not in capsys.readouterr().out
    with pytest.raises(SystemExit):
        calibration_report.main(base + ["--calibration", str(cal), "--box_fusion", "c-avg"])
