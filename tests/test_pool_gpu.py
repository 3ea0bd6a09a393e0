"""Pooling weights of score_fusion "probEn-log" on the GPU: pe_proben_fuse_batch_pooled (weights, out_cluster), pe_proben_pack_pooled
(out_source), pe_pool_nll and calibration.fit_pool_weights, against the NumPy restatement of tests/test_pool_cpu.py.  u = 2^-53."""
import json
import math
import os

import numpy as np
import pytest
import torch

from test_pool_cpu import LD, U, cluster_tables, dependence_case, log_softmax64, nll_grad, pooled_posterior, recovery_case, standard_errors

pytestmark = pytest.mark.gpu

BOX = ["v-avg", "s-avg", "avg", "argmax"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rows(out, offs, i):
    cnt = int(out["counts"][i])
    sl = slice(offs[i], offs[i] + max(cnt, 0))
    return tuple(out[k][sl].cpu().numpy() for k in ("keep", "boxes", "scores", "classes"))


# ---- fusion: weights of 1.0 are probEn-log, byte for byte -----------------------------------------------------------------------------

def _flat(infos_per_image, lps):
    from proben_amd import fusion as F
    b, s, p, v, c, offs, src = F.pack_infos(infos_per_image, with_sources=True)
    lp = _dev(np.concatenate(lps).reshape(-1, lps[0].shape[1]))
    return b, s, v, c, offs, src, lp


@pytest.mark.parametrize("rows", ["saturated", "golden"])
def test_weights_of_one_move_no_bit(golden_dir, rows):
    from test_proben_logp_gpu import _calibrated_infos, _load_case, _log_full
    from oracle import proben as O
    from proben_amd import fusion as F
    if rows == "saturated":
        cal = _calibrated_infos()
        infos, lps = [i for i, _ in cal], [lp for _, lp in cal]
    else:
        z = np.load(os.path.join(golden_dir, "proben_cases.npz"))
        infos = [_load_case(z, ci) for ci in range(int(z["num_cases"]))]
        lps = [_log_full(O.concat_infos(i)[3]) for i in infos]
    b, s, v, c, offs, src, lp = _flat(infos, lps)
    k1 = lp.shape[1]
    prior = (np.arange(k1) + 1.0).tolist()
    fused = 0
    for box in BOX:
        for pr in (None, prior):
            for bound in (None, 1100):
                ref = F.fuse_batch(b, s, None, v, c, offs, "probEn-log", box, max_rows=bound, log_probs=lp, class_prior=pr)
                got = F.fuse_batch(b, s, None, v, c, offs, "probEn-log", box, max_rows=bound, log_probs=lp, class_prior=pr,
                                   pool_weights=[1.0, 1.0, 1.0], row_source=src)
                assert torch.equal(ref["counts"], got["counts"])
                live = (torch.arange(b.shape[0], device="cuda")[None] >= offs[:-1, None]) & \
                       (torch.arange(b.shape[0], device="cuda")[None] < (offs[:-1] + ref["counts"])[:, None])
                live = live.any(0)
                fused += int(live.sum())
                for k in ("boxes", "scores", "classes", "keep"):
                    assert ref[k][live].contiguous().cpu().numpy().tobytes() == got[k][live].contiguous().cpu().numpy().tobytes(), (box, pr, bound, k)
    assert fused > 1000


# ---- fusion: non-trivial weights against the restatement ------------------------------------------------------------------------------

GRID = [(10 + 40 * ix, 10 + 40 * iy) for iy in range(12) for ix in range(15)]      # 180 far-apart 20 x 20 anchors inside 640 x 512


def _image(rng, sizes, k1, D, n_single=0, nan_row=False):
    """One image: a cluster of each size in `sizes` (+ n_single single rows) at distinct anchors, class 0, sources cycling from a random
    start, log-posteriors of random float32 logits, score = the row's own p[0] - plus, optionally, a low-score row with NaN coordinates."""
    sizes = list(sizes) + [1] * n_single
    anchors = rng.permutation(len(GRID))[:len(sizes)]
    box, src = [], []
    for a, m in zip(anchors, sizes):
        x, y = GRID[a]
        for t in range(m):
            box.append(np.array([x, y, x + 20, y + 20], np.float64) + rng.integers(-1, 2, 4))
            src.append((t + a) % D)
    n = len(box)
    box = np.asarray(box, np.float64).reshape(-1, 4)
    lp = log_softmax64(rng.normal(0, 3, (n, k1)).astype(np.float32))
    score = np.exp(lp[:, 0])
    if nan_row:
        box = np.concatenate([box, [[np.nan] * 4]])
        lp = np.concatenate([lp, log_softmax64(rng.normal(0, 3, (1, k1)))])
        score = np.append(score, score.min() * 0.5)
        src.append(0)
    perm = rng.permutation(len(score))
    return {"boxes": box[perm], "scores": score[perm], "lp": lp[perm], "src": np.asarray(src, np.int32)[perm],
            "vars": rng.uniform(0.5, 3.0, len(score)), "classes": np.zeros(len(score), np.int32)}


def _batch(images):
    cat = lambda k: np.concatenate([im[k] for im in images])  # noqa: E731
    offs = np.concatenate([[0], np.cumsum([len(im["scores"]) for im in images])]).astype(np.int32)
    return (_dev(cat("boxes").reshape(-1, 4)), _dev(cat("scores")), _dev(cat("vars")), _dev(cat("classes")), _dev(offs), _dev(cat("src")),
            _dev(cat("lp").reshape(-1, images[0]["lp"].shape[1]))), offs


def _ulp32(x):
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


def _pooled_bound(lp, w_rows, log_prior, s, a):
    """First-order bound, in units of u, of the device's float64 score against the longdouble restatement: DESIGN.md section 11's bound
    extended by the weight products.  Column j: m products w_t lp_tj (each rounds: |w_t lp_tj| u) and m - 1 additions of partial sums
    <= S_j = sum_t |w_t lp_tj|: m S_j; with a prior, W carries (m - 1) W u, W - 1 rounds (|W - 1| u), the product rounds
    (|(W - 1) lp_j| u) and the subtraction rounds (|a_j| u): [(m - 1) W + 2 |W - 1|] |lp_j| + |a_j|.  Then as section 11:
    E_j = A_j + A_best + |a_j - M| + 2, the normaliser's K additions and the division: sum_j s_j E_j + K + 1."""
    m = len(w_rows)
    w = np.asarray(w_rows, np.float64)
    A = m * (np.abs(lp) * w[:, None]).sum(0)
    if log_prior is not None:
        W = w.sum()
        A = A + ((m - 1) * W + 2 * abs(W - 1)) * np.abs(log_prior) + np.abs(a)
    j = int(np.argmax(s))
    E = A + A[j] + np.abs(a - a.max()) + 2.0
    E[j] = 0.0
    return float((s * E).sum()) + len(a) - 1 + 1


@pytest.mark.parametrize("D,k1,weights", [(2, 4, [0.7, 0.4]), (2, 2, [0.0, 1.3]), (3, 4, [0.5, 0.0, 0.25]), (3, 63, [1.5, 0.3, 0.6]), (2, 63, [0.2, 0.9])])
def test_weights_against_the_restatement(D, k1, weights):
    from test_proben_logp_gpu import _clusters
    from proben_amd import fusion as F
    rng = np.random.default_rng(100 * D + k1)
    images = [_image(rng, [1, 2, 3, 9, 2, 5], k1, D, n_single=3) for _ in range(6)]
    (b, s, v, c, offs_d, src, lp), offs = _batch(images)
    worst = checked = 0
    for prior in (None, rng.dirichlet(np.ones(k1) * 3)):
        lprior = None if prior is None else np.log(prior / prior.sum())
        # the second bound selects the sequential clustering: 1100 rows where they fit the LDS; at K + 1 = 63 a row takes 617 bytes
        # (capacity 264 rows), and 260 rows fit sequentially (160 436 bytes) but not with the bit matrices (+ 20 800)
        for box, bound in (("v-avg", None), ("s-avg", 1100 if k1 <= 4 else 260)):
            ref = F.fuse_batch(b, s, None, v, c, offs_d, "probEn-log", box, max_rows=bound, log_probs=lp,
                               class_prior=None if prior is None else prior.tolist())
            got = F.fuse_batch(b, s, None, v, c, offs_d, "probEn-log", box, max_rows=bound, log_probs=lp,
                               class_prior=None if prior is None else prior.tolist(), pool_weights=weights, row_source=src)
            assert torch.equal(ref["counts"], got["counts"])
            for i, im in enumerate(images):
                rk, rb, rs, rc = _rows(ref, offs, i)
                gk, gb, gs, gc = _rows(got, offs, i)
                cl = _clusters(im["boxes"], im["scores"], im["classes"].astype(np.float64))
                assert gk.tolist() == [p for p, _ in cl] and gk.tobytes() == rk.tobytes() and gb.tobytes() == rb.tobytes()
                for r, (piv, mem) in enumerate(cl):
                    if len(mem) == 1:
                        assert gs[r] == np.float32(im["scores"][piv]) and gc[r] == 0.0
                        continue
                    w_rows = [weights[k] for k in im["src"][mem]]
                    sp, a = pooled_posterior(im["lp"][mem], w_rows, lprior)
                    j = int(np.argmax(sp))
                    want = sp[j]
                    bnd = _pooled_bound(im["lp"][mem], w_rows, lprior, sp.astype(np.float64), a.astype(np.float64))
                    tol = 0.5 * _ulp32(float(want)) * (1 + 2.0 ** -20) + bnd * U * float(want)
                    err = abs(LD(gs[r]) - want)
                    worst = max(worst, float(err / tol))
                    assert err <= tol, (i, r, len(mem), gs[r], float(want), float(err), tol)
                    assert gc[r] == j
                    checked += 1
    print(f"D={D} K+1={k1} w={weights}: {checked} clusters, largest error {worst:.3f} of its bound")
    assert checked >= 100


# ---- out_cluster -----------------------------------------------------------------------------------------------------------------------

def test_out_cluster():
    from test_proben_logp_gpu import _clusters
    from proben_amd import fusion as F
    rng = np.random.default_rng(5)
    k1, D = 4, 2
    images = []
    for n in (0, 1, 2, 63, 64, 65, 129):          # the bit matrices' word boundaries
        pick = [9, 3, 2, 3] if n >= 17 else [2] if n == 2 else []
        images.append(_image(rng, pick, k1, D, n_single=n - sum(pick)))
        assert len(images[-1]["scores"]) == n
    images.append(_image(rng, [9, 3, 2, 1], k1, D, n_single=4, nan_row=True))
    single = _image(rng, [2, 3], k1, D, n_single=2)        # a passthrough image
    images.append(single)
    over = {"boxes": rng.uniform(0, 400, (1101, 4)), "scores": rng.uniform(0, 1, 1101), "lp": log_softmax64(rng.normal(0, 1, (1101, k1))),
            "src": np.zeros(1101, np.int32), "vars": np.ones(1101), "classes": np.zeros(1101, np.int32)}
    images.insert(4, over)
    (b, s, v, c, offs_d, src, lp), offs = _batch(images)
    B = len(images)
    counts = _dev(np.diff(offs).astype(np.int32))
    passthrough = np.zeros(B, np.int32)
    passthrough[B - 1] = 1
    call = lambda bound, sl=slice(None), o=offs_d[:-1], cn=counts, pt=_dev(passthrough), args=(b, s, v, c, src, lp): F.fuse_batch(  # noqa: E731
        args[0], args[1], None, args[2], args[3], o, "probEn-log", "v-avg", max_rows=bound, log_probs=args[5], row_counts=cn, passthrough=pt,
        pool_weights=[0.7, 0.4], row_source=args[4])
    tight, wide = call(129), call(1100)
    torch.cuda.synchronize()
    assert tight["cluster"].cpu().numpy().tobytes() == wide["cluster"].cpu().numpy().tobytes()
    assert torch.equal(tight["counts"], wide["counts"])
    got = tight["cluster"].cpu().numpy()
    seen = set()
    for i, im in enumerate(images):
        n = len(im["scores"])
        g = got[offs[i]:offs[i] + n]
        if i == 4:
            assert int(tight["counts"][i]) == -1 and (g == -2).all()
            continue
        if passthrough[i]:
            assert g.tolist() == list(range(n)) and int(tight["counts"][i]) == n
            continue
        want = np.full(n, -1, np.int32)
        cl = _clusters(im["boxes"], im["scores"], im["classes"].astype(np.float64))
        for k, (_, mem) in enumerate(cl):
            want[mem] = k
            seen.add(len(mem))
        assert g.tolist() == want.tolist(), i
        assert int(tight["counts"][i]) == len(cl)
        if np.isnan(im["boxes"]).any():
            assert (want == -1).sum() == 1 and want[np.isnan(im["boxes"][:, 0])][0] == -1
        if n == 0:
            continue
        # alone in its launch: the same bytes
        one = F.fuse_batch(_dev(im["boxes"].reshape(-1, 4)), _dev(im["scores"]), None, _dev(im["vars"]), _dev(im["classes"]),
                           _dev(np.array([0, n], np.int32)), "probEn-log", "v-avg", max_rows=max(n, 1), log_probs=_dev(im["lp"].reshape(-1, k1)),
                           pool_weights=[0.7, 0.4], row_source=_dev(im["src"]))
        assert one["cluster"].cpu().numpy().tobytes() == g.tobytes(), i
    assert {1, 2, 3, 9} <= seen


# ---- out_source ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nd", [2, 3])
def test_out_source(nd):
    """Counts 0 / 1 / 64 / 65 / 66 / above D per detector, classes above max_class dropped on both sides of the 64-row chunk boundary, an
    image with a single source: out_source is the detector index of every written row; every other output is pe_proben_pack_calibrated's."""
    from proben_amd import fusion as F
    rng = np.random.default_rng(nd)
    D, K = 66, 3
    pat = [[0, 0, 0], [1, 0, 0], [0, 5, 0], [64, 65, 66], [66, 64, 1], [65, 70, 64], [70, 70, 70], [1, 1, 1]]
    B = len(pat)
    dets = []
    for d in range(nd):
        cls = rng.integers(0, 5, (B, D)).astype(np.int32)
        cls[:, 62:66] = rng.integers(2, 4, (B, 4))         # drops across the chunk boundary
        cls[:, 0] = 0
        dets.append({"boxes": _dev(rng.uniform(0, 300, (B, D, 4)).astype(np.float32)), "scores": _dev(rng.uniform(0, 1, (B, D)).astype(np.float32)),
                     "classes": _dev(cls), "prob_score": _dev(rng.dirichlet(np.ones(K + 1), (B, D))[:, :, :K].astype(np.float32)),
                     "class_logits": _dev(rng.normal(0, 3, (B, D, K + 1)).astype(np.float32)), "vars": _dev(rng.uniform(0.5, 2, (B, D)).astype(np.float32)),
                     "counts": _dev(np.array([p[d] for p in pat], np.int32))})
    w = [1.0] * nd
    for temps, logp, vs in ((None, False, None), ((1.5, 0.8, 1.1)[:nd], False, (0.5, 2.0, 1.5)[:nd]), ((1.5, 0.8, 1.1)[:nd], True, (0.5, 2.0, 1.5)[:nd])):
        ref = F.pack_rows(dets, 2, temps, log_posteriors=logp, variance_scales=vs or [1.0] * nd)
        got = F.pack_rows(dets, 2, temps, log_posteriors=logp, variance_scales=vs or [1.0] * nd, pool_weights=w)
        bare = F.pack_rows(dets, 2, temps, log_posteriors=logp, variance_scales=None, pool_weights=w) if vs is None else None
        torch.cuda.synchronize()
        assert len(got) == len(ref) + 1
        cnt = ref[6].cpu().numpy()
        S = nd * D
        live = _dev((np.arange(S)[None] < cnt[:, None]).reshape(-1))
        for i in (5, 6, 7):
            assert torch.equal(ref[i], got[i])
        for i in [0, 1, 2, 3, 4] + ([8] if logp else []):
            assert ref[i][live].contiguous().cpu().numpy().tobytes() == got[i][live].contiguous().cpu().numpy().tobytes(), i
            if bare is not None:
                assert ref[i][live].contiguous().cpu().numpy().tobytes() == bare[i][live].contiguous().cpu().numpy().tobytes(), i
        src = got[-1].cpu().numpy().reshape(B, S)
        for b in range(B):
            want = []
            for d in range(nd):
                c = min(pat[b][d], D)
                want += [d] * int((dets[d]["classes"][b, :c].cpu().numpy() <= 2).sum())
            assert cnt[b] == len(want) and src[b, :cnt[b]].tolist() == want, b
        assert int(ref[7][1]) == 1 and int(ref[7][3]) == 0


# ---- routes ----------------------------------------------------------------------------------------------------------------------------

def test_fuse_detections_is_pack_plus_fuse_and_equals_the_file_route():
    from test_calibration_gpu import detector_rows
    from proben_amd import fusion as F
    from proben_amd.late_fusion import late_fusion
    dets = detector_rows(3)
    temps, prior, w = (1.5, 0.8), [0.1, 0.3, 0.2, 0.4], [0.6, 0.35]
    B, D = dets[0]["scores"].shape
    S = 2 * D
    dev = F.fuse_detections(dets, "probEn-log", "s-avg", temperatures=temps, class_prior=prior, pool_weights=w)
    plain = F.fuse_detections(dets, "probEn-log", "s-avg", temperatures=temps, class_prior=prior)
    ob, os_, op, ov, oc, ooff, ocnt, osingle, olp, osrc = F.pack_rows(dets, 2, temps, log_posteriors=True, pool_weights=w)
    two = F.fuse_batch(ob, os_, op, ov, oc, ooff, "probEn-log", "s-avg", max_rows=S, row_counts=ocnt, passthrough=osingle, log_probs=olp,
                       class_prior=prior, pool_weights=w, row_source=osrc)
    torch.cuda.synchronize()
    cnt = dev["counts"].cpu().numpy()
    assert cnt.sum() > 0 and torch.equal(dev["counts"], two["counts"]) and torch.equal(dev["counts"], plain["counts"])
    live = _dev((np.arange(S)[None] < cnt[:, None]).reshape(-1))
    for k in ("boxes", "scores", "classes", "keep"):
        assert dev[k][live].contiguous().cpu().numpy().tobytes() == two[k][live].contiguous().cpu().numpy().tobytes(), k
    assert not torch.equal(dev["scores"][live], plain["scores"][live]), "the weights changed no score"
    j1 = []
    for d in dets:
        c = d["counts"].cpu().numpy()
        rec = {k: [] for k in ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")}
        for b in range(B):
            keep = [j for j in range(c[b]) if int(d["classes"][b, j]) <= 2]
            rec["image"].append(f"f{b}.jpeg")
            rec["image_id"].append(b)
            for key, src in (("boxes", "boxes"), ("scores", "scores"), ("classes", "classes"), ("class_logits", "class_logits"), ("probs", "prob_score")):
                rec[key].append([d[src][b, j].tolist() for j in keep])
            rec["vars"].append([[float(d["vars"][b, j])] for j in keep])
        j1.append(json.loads(json.dumps(rec)))
    via = late_fusion(j1, ["probEn-log", "s-avg"], temperatures=temps, class_prior=prior, pool_weights=w)
    for b in range(B):
        if via[b] is None:
            assert cnt[b] == 0
            continue
        sl = slice(b * S, b * S + cnt[b])
        fb, fs, fc = via[b]
        assert len(fs) == cnt[b], b
        assert np.asarray(fb, np.float64).tobytes() == dev["boxes"][sl].cpu().numpy().tobytes(), b
        assert fs.numpy().tobytes() == dev["scores"][sl].cpu().numpy().tobytes(), b
        assert fc.numpy().tobytes() == dev["classes"][sl].cpu().numpy().tobytes(), b


# ---- pe_pool_nll -----------------------------------------------------------------------------------------------------------------------

def _nll_case(rng, C, D, k1, bad=True):
    size = rng.integers(2, 10, C)
    labels = rng.integers(0, k1, C).astype(np.int32)
    excluded = []
    if bad and C >= 63:
        size[[3, C - 1]] = [1, 0]
        labels[7] = k1
        labels[11] = -1
        excluded = [3, 7, 11, C - 1]
    offs = np.concatenate([[0], np.cumsum(size)]).astype(np.int32)
    M = int(offs[-1])
    N = M + 5
    members = rng.permutation(N)[:M].astype(np.int32)            # the clusters' rows are scattered
    src = rng.integers(0, D, N).astype(np.int32)
    if bad and C >= 63:
        src[members[offs[20]]] = D                                # a bad source in cluster 20
        excluded.append(20)
    lp = log_softmax64(rng.normal(0, 3, (N, k1)).astype(np.float32))
    return lp, src, members, offs, labels, sorted(excluded)


def _nll_bounds(lp, src, members, offs, labels, w, lprior, ok, C):
    """Restatement in longdouble and the first-order bounds (in u) of DESIGN.md section 15 for the NLL and every gradient entry."""
    D = len(w)
    k1 = lp.shape[1]
    src_ok = np.where(src < D, src, 0)
    G, n, size = cluster_tables(lp, src_ok, members, offs, D, lprior, LD)
    Gabs, _, _ = cluster_tables(np.abs(lp), src_ok, members, offs, D, None, np.float64)
    G, n, Gabs, y = G[ok], n[ok], Gabs[ok], labels[ok]
    nll, grad = nll_grad(G, y, np.asarray(w, LD), lprior)
    G64 = G.astype(np.float64)
    gam = np.maximum(n - 1, 0)[:, :, None] * Gabs                  # the table: n_d - 1 additions of partial sums <= Gabs
    if lprior is not None:
        gam = gam + np.abs(n[:, :, None] * lprior[None, None, :]) + np.abs(G64)
    wv = np.asarray(w, np.float64)
    Aabs = np.einsum("d,cdj->cj", wv, np.abs(G64))
    a = np.einsum("d,cdj->cj", wv, G64) + (0 if lprior is None else lprior[None, :])
    alpha = np.einsum("d,cdj->cj", wv, gam) + D * Aabs + (np.abs(a) if lprior is not None else 0)
    top = a.max(1, keepdims=True)
    e = np.exp(a - top)
    tot = e.sum(1, keepdims=True)
    s = e / tot
    idx = np.arange(len(y))
    eps = alpha + np.abs(a - top) + 2
    tau = (s * eps).sum(1) + k1 - 1                                 # + K
    b_nll = tau + 2 * np.abs(np.log(tot[:, 0])) + alpha[idx, y] + np.abs(a[idx, y] - top[:, 0]) + np.abs(nll.astype(np.float64))
    K = k1 - 1
    b_grad = np.einsum("cj,cdj->cd", s * (eps + tau[:, None] + K + 2), np.abs(G64)) + np.einsum("cj,cdj->cd", s, gam) + gam[idx, :, y] \
        + np.abs(grad.astype(np.float64))
    # the accumulation: per lane ceil(C / (4 blocks)) clusters in turn, 4 waves, ceil(blocks / 16) blocks, 16 segments
    blocks = max(1, min((C + 3) // 4, 1024))
    depth = -(-C // (4 * blocks)) + 3 + -(-blocks // 16) + 15
    tol_nll = (b_nll.sum() + depth * np.abs(nll.astype(np.float64)).sum()) * U * 1.01
    tol_grad = (b_grad.sum(0) + depth * np.abs(grad.astype(np.float64)).sum(0)) * U * 1.01
    return nll.sum(), grad.sum(0), tol_nll, tol_grad


@pytest.mark.parametrize("C,D,k1,nc,prior", [(1, 2, 4, 1, False), (63, 3, 2, 64, True), (64, 2, 63, 64, False), (65, 3, 4, 1, True),
                                             (4097, 2, 4, 64, True), (4500, 3, 63, 64, False)])
def test_pool_nll_against_the_restatement(C, D, k1, nc, prior):
    from proben_amd import calibration as Cal
    rng = np.random.default_rng(C + 10 * D + k1)
    lp, src, members, offs, labels, excluded = _nll_case(rng, C, D, k1)
    lprior = np.log(rng.dirichlet(np.ones(k1) * 3)) if prior else None
    W = rng.uniform(0, 1.5, (nc, D))
    W[0] = 1.0
    if nc > 2:
        W[1, 0] = 0.0
    args = (_dev(lp), _dev(src), _dev(members), _dev(offs), _dev(labels))
    lpd = None if lprior is None else _dev(lprior)
    nll, grad, bad, last = Cal.pool_nll(*args, W, lpd)
    again = Cal.pool_nll(*args, W, lpd)
    assert nll.tobytes() == again[0].tobytes() and grad.tobytes() == again[1].tobytes()
    assert bad == len(excluded) and last == (excluded[-1] if excluded else -1)
    ok = np.ones(C, bool)
    ok[excluded] = False
    worst = 0.0
    for ci in sorted({0, 1, nc // 2, nc - 1} & set(range(nc))):
        want, wgrad, tol, tolg = _nll_bounds(lp, src, members, offs, labels, W[ci], lprior, ok, C)
        en, eg = abs(LD(nll[ci]) - want), np.abs(grad[ci].astype(LD) - wgrad)
        worst = max(worst, float(en / tol), float((eg / tolg).max()))
        assert en <= tol, (ci, float(nll[ci]), float(want), float(en), tol)
        assert (eg <= tolg).all(), (ci, grad[ci], wgrad, eg, tolg)
    print(f"C={C} D={D} K+1={k1} candidates={nc} prior={prior}: {bad} excluded, largest error {worst:.4f} of its bound")


def test_pool_nll_gradient_against_central_differences():
    """Central difference of the kernel's own NLL with step h = 2^-13: truncation h^2 / 6 * |third derivative| <= h^2 / 6 * sum_c R_cd^3
    (R_cd = the range of G_d over the columns: a third cumulant of a variable of range R is at most R^3), rounding 2 eps_f / (2 h) with
    eps_f the kernel's own NLL error bound (section 15) at this size."""
    from proben_amd import calibration as Cal
    rng = np.random.default_rng(77)
    C, D, k1 = 300, 3, 4
    lp, src, members, offs, labels, _ = _nll_case(rng, C, D, k1, bad=False)
    w0 = np.array([0.7, 0.4, 1.1])
    h = 2.0 ** -13
    cand = np.vstack([w0] + [w0 + sgn * h * np.eye(D)[d] for d in range(D) for sgn in (1, -1)])
    nll, grad, bad, _ = Cal.pool_nll(_dev(lp), _dev(src), _dev(members), _dev(offs), _dev(labels), cand)
    assert bad == 0
    ok = np.ones(C, bool)
    _, _, eps_f, _ = _nll_bounds(lp, src, members, offs, labels, w0, None, ok, C)
    G, _, _ = cluster_tables(lp, src, members, offs, D)
    R3 = ((G.max(2) - G.min(2)) ** 3).sum(0)
    for d in range(D):
        fd = (nll[1 + 2 * d] - nll[2 + 2 * d]) / (2 * h)
        tol = h * h / 6 * R3[d] + 2 * eps_f / (2 * h) + abs(fd) * 4 * U
        print(f"d={d}: gradient {grad[0, d]:.9f}, central difference {fd:.9f}, tolerance {tol:.3g} (NLL {nll[0]:.3f})")
        assert abs(fd - grad[0, d]) <= tol


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------

def _case_dev(case):
    return tuple(_dev(case[k]) for k in ("log_probs", "row_source", "member_rows", "cluster_offsets", "labels"))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fit_recovers_the_weights(seed):
    from proben_amd import calibration as Cal
    case = recovery_case(seed)
    fit = Cal.fit_pool_weights(*_case_dev(case), 2)
    se = standard_errors(case["G"], case["labels"], case["w_true"])
    z = (np.asarray(fit["weights"]) - case["w_true"]) / se
    print(f"seed {seed}: {fit['weights']} after {fit['rounds']} rounds, z {z}, grad {fit['grad']}, converged {fit['converged']}")
    assert (np.abs(z) <= 4).all()
    assert fit["converged"] and fit["at_bound"] == [None, None] and fit["clusters"] == 20000 and fit["excluded"] == 0
    assert fit["nll"] < fit["nll_at_1"]


def _fused_scores(case, weights):
    """Every cluster as an image of identical boxes through pe_proben_fuse_batch_pooled: (conf f64, correct i32) per cluster."""
    from proben_amd import fusion as F
    lp, offs = case["log_probs"], case["cluster_offsets"]
    N = len(lp)
    boxes = np.tile([[10.0, 10.0, 60.0, 70.0]], (N, 1))
    out = F.fuse_batch(_dev(boxes), _dev(np.exp(lp.max(1))), None, _dev(np.ones(N)), _dev(np.zeros(N, np.int32)), _dev(offs), "probEn-log", "avg",
                       max_rows=3, log_probs=_dev(lp), pool_weights=weights, row_source=_dev(case["row_source"]))
    assert int((out["counts"] != 1).sum()) == 0
    first = _dev(offs[:-1].astype(np.int64))
    return out["scores"][first].double(), (out["classes"][first].int() == _dev(case["labels"])).int()


def test_fit_on_dependent_detectors_lowers_nll_and_ece():
    from proben_amd import calibration as Cal
    fit_case, held = dependence_case(0), dependence_case(1)
    fit = Cal.fit_pool_weights(*_case_dev(fit_case), 2)
    w = fit["weights"]
    nll, _, bad, _ = Cal.pool_nll(*_case_dev(held), [[1.0, 1.0], w])
    C = len(held["labels"])
    ece = [Cal.reliability_scores(*_fused_scores(held, ww), bins=15)["ece"] for ww in ([1.0, 1.0], w)]
    print(f"weights {w} ({fit['rounds']} rounds, converged {fit['converged']}); held-out NLL per cluster {nll[0] / C:.4f} -> {nll[1] / C:.4f}; "
          f"ECE {ece[0]:.4f} -> {ece[1]:.4f}")
    assert bad == 0 and nll[1] < nll[0] and ece[1] < ece[0]
    assert all(x < 1 for x in w)


# ---- the driver ------------------------------------------------------------------------------------------------------------------------

def test_demo_proben_pool_weights(tmp_path):
    """demo_probEn --score_fusion probEn-log with pool weights from --calibration: the two-stage and the --one-pass route give identical
    AP tables and rows, which differ from the run without weights; --pool_weights 1,1 reproduces the run without weights byte for byte."""
    from test_stream_gpu import _weights, _write_flir
    from proben_amd import calibration as C
    from proben_amd.cli import demo_probEn, save_predictions
    root = tmp_path / "val"
    _write_flir(root, 6, 96, 120, (150, 180))
    names = ["thermal_only", "early_fusion"]
    paths = [_weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
    pdir = tmp_path / "pred"
    for m, p in zip(names, paths):
        save_predictions.main(["--dataset_path", str(root), "--fusion_method", m, "--model_path", p, "--prediction_path", str(pdir), "--batch", "4"])
    cal = tmp_path / "calibration.json"
    C.save(cal, {"thermal_only": 1.0, "early_fusion": 1.0}, pool_weights={"thermal_only": 0.6, "early_fusion": 0.3})
    log = ["--score_fusion", "probEn-log"]

    def two_stage(tag, extra):
        out = tmp_path / f"out2_{tag}"
        res = demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names),
                                "--outfolder", str(out), "--dataset_name", f"flir_pool2_{tag}"] + log + extra)
        return out, res

    def one_pass(tag, extra):
        out = tmp_path / f"out1_{tag}"
        res = demo_probEn.main(["--one-pass", "--dataset_path", str(root), "--detectors", ",".join(names), "--model_paths", ",".join(paths),
                                "--workers", "2", "--batch", "4", "--outfolder", str(out), "--dataset_name", f"flir_pool1_{tag}"] + log + extra)
        return out, res

    def rows(o):
        return json.load(open(o / "coco_instances_results.json"))

    plain, res0 = two_stage("plain", [])
    ones, res1 = two_stage("ones", ["--pool_weights", "1,1"])
    assert "pool_weights" not in res0 and res1["pool_weights"] == dict(zip(names, [1.0, 1.0]))
    assert (plain / "coco_instances_results.json").read_bytes() == (ones / "coco_instances_results.json").read_bytes()
    assert (plain / "FLIR_probEn_eval.json").read_bytes() == (ones / "FLIR_probEn_eval.json").read_bytes()
    o2, r2 = two_stage("cal", ["--calibration", str(cal)])
    o1, r1 = one_pass("cal", ["--calibration", str(cal)])
    assert r2["pool_weights"] == r1["pool_weights"] == {"thermal_only": 0.6, "early_fusion": 0.3}
    assert (o1 / "FLIR_probEn_eval.json").read_bytes() == (o2 / "FLIR_probEn_eval.json").read_bytes()
    a, b = rows(o1), rows(o2)
    assert len(a) == len(b) > 0
    assert [(r["image_id"], r["category_id"], r["score"]) for r in a] == [(r["image_id"], r["category_id"], r["score"]) for r in b]
    assert [r["score"] for r in b] != [r["score"] for r in rows(plain)]
    with pytest.raises(SystemExit):
        demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names), "--pool_weights", "1,1"])


def _dependent_files(tmp_path, n_img=16):
    """A FLIR val folder of n_img images and two prediction files over it, written by hand: per image 4 objects on a grid of disjoint
    30 x 35 boxes; detector 0 sees logits z0 ~ N(0, 2^2) per object, detector 1 a noisy copy z0 + N(0, 1) with detector 0's class (rows
    cluster within a class only), both with boxes within a pixel of the object's; the object's class is drawn from softmax(z0) and an
    object drawn as background gets no annotation.  Detector 0 adds one detection per image that nothing overlaps: a cluster of one.
    Returns (root, files, per image: the objects' labels in [0, 3])."""
    from test_stream_gpu import _write_flir
    root = tmp_path / "val"
    _write_flir(root, n_img, 96, 120, (96, 120))
    val = root / "FLIR_thermal_RGBT_pairs_val.json"
    ds = json.load(open(val))
    rng = np.random.default_rng(5)
    grid = [(5.0, 5.0), (45.0, 5.0), (5.0, 55.0), (45.0, 55.0)]
    preds = [{k: [] for k in ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")} for _ in range(2)]
    anns, labels = [], []
    for im in ds["images"]:
        z0 = rng.normal(0, 2, (4, 4)).astype(np.float32)
        p0 = np.exp(log_softmax64(z0))
        lab = [int(rng.choice(4, p=p / p.sum())) for p in p0]
        labels.append(lab)
        for (x, y), l in zip(grid, lab):
            if l < 3:
                anns.append({"id": len(anns) + 1, "image_id": im["id"], "category_id": l + 1, "bbox": [x, y, 30.0, 35.0], "area": 1050.0, "iscrowd": 0})
        cls = z0[:, :3].argmax(1)
        for d, p in enumerate(preds):
            z = z0 if d == 0 else (z0 + rng.normal(0, 1, z0.shape)).astype(np.float32)
            bx = [[x + e[0], y + e[1], x + 30 + e[2], y + 35 + e[3]] for (x, y), e in zip(grid, rng.uniform(-1, 1, (4, 4)))]
            c = cls.tolist()
            if d == 0:
                z = np.concatenate([z, rng.normal(0, 2, (1, 4)).astype(np.float32)])
                bx.append([85.0, 5.0, 115.0, 40.0])
                c.append(int(z[4, :3].argmax()))
            pr = np.exp(log_softmax64(z))
            p["image"].append(os.path.basename(im["file_name"]))
            p["image_id"].append(im["id"])
            p["boxes"].append(bx)
            p["classes"].append(c)
            p["class_logits"].append(z.tolist())
            p["probs"].append(pr[:, :3].tolist())
            p["scores"].append([float(pr[i, k]) for i, k in enumerate(c)])
            p["vars"].append([[0.01]] * len(bx))
    ds["annotations"] = anns
    json.dump(ds, open(val, "w"))
    pdir = tmp_path / "pred"
    pdir.mkdir()
    files = []
    for m, p in zip(("thermal_only", "early_fusion"), preds):
        files.append(str(pdir / f"val_{m}_predictions.json"))
        json.dump(p, open(files[-1], "w"))
    return root, files, preds, labels


def _own_nll(preds, labels, images, temps, prior, weights):
    """pool_nll per cluster over the 2-row clusters of `images`, from the test's own bookkeeping: object j of an image is rows (j of
    detector 0, j of detector 1) and its label the drawn one.  The clusters are summed in another order than the driver's (object
    order against fused-score order): the two sums of C terms agree to C u relative to the sum of the terms' magnitudes."""
    from proben_amd import calibration as Cal
    lp, src, mem, lab = [], [], [], []
    n = 0
    for i in images:
        for d in range(2):
            z = torch.tensor(preds[d]["class_logits"][i], dtype=torch.float32).cuda()
            lp.append(Cal.log_posteriors(z, temps[d]).cpu().numpy())
            src += [d] * len(z)
        mem += [(n + j, n + 5 + j) for j in range(4)]
        lab += labels[i]
        n += 9
    C = len(lab)
    nll, _, bad, _ = Cal.pool_nll(_dev(np.concatenate(lp)), _dev(np.array(src, np.int32)), _dev(np.array(mem, np.int32).reshape(-1)),
                                  _dev(np.arange(0, 2 * C + 1, 2, dtype=np.int32)), _dev(np.array(lab, np.int32)),
                                  [[1.0, 1.0], weights], None if prior is None else _dev(np.log(np.asarray(prior, np.float64))))
    assert bad == 0
    return C, nll / C


def test_fit_temperature_and_report_drivers(tmp_path, capsys):
    """fit_temperature --with-pool-weights writes the key and what goes with it, calibration_report prints the held-out fused NLL per
    cluster with and without the weights and fuses its "after" rows with them, and demo_probEn picks the fitted key up."""
    from proben_amd import calibration as Cal
    from proben_amd.cli import calibration_report, demo_probEn, fit_temperature
    root, files, preds, labels = _dependent_files(tmp_path)
    names = ["thermal_only", "early_fusion"]
    cal = tmp_path / "cal.json"
    fit_temperature.main(["--predictions", *files, "--dataset_path", str(root), "--holdout", "0.5", "--out", str(cal), "--with-prior",
                          "--with-pool-weights"])
    printed = capsys.readouterr().out
    rec = Cal.load(cal)
    with capsys.disabled():          # shown, and kept out of what the next readouterr() returns
        print(printed)
    assert "pool weights:" in printed and list(rec["pool_weights"]) == names
    w = [rec["pool_weights"][m] for m in names]
    assert all(math.isfinite(x) and x >= 0 for x in w) and any(x > 0 for x in w)
    assert rec["pool_clusters"] == 8 * 4 and rec["pool_excluded"] == 8            # the clusters of one row are counted, not fitted
    assert set(rec["pool_at_bound"]) == set(names) and rec["pool_fit"]["box_fusion"] == "v-avg" and rec["pool_fit"]["iou"] == 0.5
    assert rec["pool_nll"]["after"] <= rec["pool_nll"]["before"]
    temps = [rec["detectors"][m] for m in names]
    C, own = _own_nll(preds, labels, range(8), temps, rec["class_prior"], w)
    with capsys.disabled():
        print("fitted images:", rec["pool_nll"], "the test's own", own.tolist())
    for tag, x in zip(("before", "after"), own):
        assert abs(rec["pool_nll"][tag] - x) <= 1e-12 * max(1.0, abs(x))

    base = ["--dataset_path", str(root), "--predictions", *files, "--score_fusion", "probEn-log"]
    report = calibration_report.main(base + ["--calibration", str(cal)])
    printed = capsys.readouterr().out
    with capsys.disabled():          # shown, and kept out of what the next readouterr() returns
        print(printed)
    assert "fused NLL per cluster" in printed and "at w = 1" in printed and "at the file's pool weights" in printed
    pool = report["pool"]
    assert pool["weights"] == rec["pool_weights"] and pool["applied"] and pool["clusters"] == 32 and pool["excluded"] == 8
    C, own = _own_nll(preds, labels, range(8, 16), temps, rec["class_prior"], w)
    for tag, x in zip(("before", "after"), own):
        assert f"{pool['nll'][tag]:.6f}" in printed
        assert abs(pool["nll"][tag] - x) <= 1e-12 * max(1.0, abs(x))
    stripped = {k: v for k, v in json.load(open(cal)).items() if not k.startswith("pool_")}
    json.dump(stripped, open(tmp_path / "cal_plain.json", "w"))
    plain = calibration_report.main(base + ["--calibration", str(tmp_path / "cal_plain.json")])
    assert "pool" not in plain and "fused NLL per cluster" not in capsys.readouterr().out
    fig = lambda r: (r["rows"], r["excluded"], r["ece"], r["mce"], r["brier"])        # (the empty bins hold NaN)
    assert fig(plain["fused"]["before"]) == fig(report["fused"]["before"])
    assert plain["fused"]["after"]["rows"] == report["fused"]["after"]["rows"]
    assert plain["fused"]["after"]["brier"] != report["fused"]["after"]["brier"]       # the "after" rows are fused with the weights
    other = calibration_report.main(base[:-1] + ["probEn", "--calibration", str(cal)])
    assert not other["pool"]["applied"] and "no pooled form" in capsys.readouterr().out

    res = demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(tmp_path / "pred"), "--detectors", ",".join(names),
                            "--outfolder", str(tmp_path / "out"), "--dataset_name", "flir_pool_fit", "--score_fusion", "probEn-log",
                            "--calibration", str(cal)])
    assert res["pool_weights"] == rec["pool_weights"]
    with pytest.raises(SystemExit):
        fit_temperature.main(["--predictions", files[0], "--dataset_path", str(root), "--out", str(cal), "--with-pool-weights"])
