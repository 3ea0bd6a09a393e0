"""Pooling weights of score_fusion "probEn-log" on the GPU: pe_proben_fuse_batch_pooled (weights, out_cluster), pe_proben_pack_pooled
(out_source), pe_pool_nll and calibration.fit_pool_weights, against the np.longdouble restatement of the rule (tests/fuse_ref.py) and
the NumPy restatement of the fit (tests/test_pool_cpu.py).  u = 2^-53."""
import json
import math
import os

import numpy as np
import pytest
import torch

import fuse_inputs
from fuse_inputs import batch, calibrated_infos, dependent_files, detector_rows, grid_image, image_rows, load_case, log_full, to_dev, write_flir
from fuse_ref import BOX, LD, U, clusters, log_softmax, restate, ulp32
from test_pool_cpu import cluster_tables, dependence_case, nll_grad, recovery_case, standard_errors

pytestmark = pytest.mark.gpu


# ---- fusion: weights of 1.0 are probEn-log, byte for byte -----------------------------------------------------------------------------

def _flat(infos_per_image, lps):
    from proben_amd import fusion as F
    b, s, p, v, c, offs, src = F.pack_infos(infos_per_image, with_sources=True)
    lp = to_dev(np.concatenate(lps).reshape(-1, lps[0].shape[1]))
    return b, s, v, c, offs, src, lp


@pytest.mark.parametrize("rows", ["saturated", "golden"])
def test_weights_of_one_move_no_bit(golden_dir, rows):
    from oracle import proben as O
    from proben_amd import fusion as F
    if rows == "saturated":
        cal = calibrated_infos()
        infos, lps = [i for i, _ in cal], [lp for _, lp in cal]
    else:
        z = np.load(os.path.join(golden_dir, "proben_cases.npz"))
        infos = [load_case(z, ci) for ci in range(int(z["num_cases"]))]
        lps = [log_full(O.concat_infos(i)[3]) for i in infos]
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

@pytest.mark.parametrize("D,k1,weights", [(2, 4, [0.7, 0.4]), (2, 2, [0.0, 1.3]), (3, 4, [0.5, 0.0, 0.25]), (3, 63, [1.5, 0.3, 0.6]), (2, 63, [0.2, 0.9])])
def test_weights_against_the_restatement(D, k1, weights):
    from proben_amd import fusion as F
    rng = np.random.default_rng(100 * D + k1)
    images = [grid_image(rng, [1, 2, 3, 9, 2, 5], k1, D, n_single=3) for _ in range(6)]
    (b, s, v, c, offs_d, src, lp), offs = batch(images)
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
                rk, rb, rs, rc = image_rows(ref, offs, i)
                gk, gb, gs, gc = image_rows(got, offs, i)
                cl = clusters(im["boxes"], im["scores"], im["classes"].astype(np.float64))
                assert gk.tolist() == [p for p, _ in cl] and gk.tobytes() == rk.tobytes() and gb.tobytes() == rb.tobytes()
                for r, (piv, mem) in enumerate(cl):
                    if len(mem) == 1:
                        assert gs[r] == np.float32(im["scores"][piv]) and gc[r] == 0.0
                        continue
                    w = restate(im["lp"], mem, src=im["src"], weights=weights, log_prior=lprior)
                    want, j = w["score"], w["cls"]
                    tol = 0.5 * ulp32(float(want)) * (1 + 2.0 ** -20) + w["score_bound"] * U * float(want)
                    err = abs(LD(gs[r]) - want)
                    worst = max(worst, float(err / tol))
                    assert err <= tol, (i, r, len(mem), gs[r], float(want), float(err), tol)
                    assert gc[r] == j
                    checked += 1
    print(f"D={D} K+1={k1} w={weights}: {checked} clusters, largest error {worst:.3f} of its bound")
    assert checked >= 100


# ---- out_cluster -----------------------------------------------------------------------------------------------------------------------

def test_out_cluster():
    from proben_amd import fusion as F
    rng = np.random.default_rng(5)
    k1, D = 4, 2
    images = []
    for n in (0, 1, 2, 63, 64, 65, 129):          # the bit matrices' word boundaries
        pick = [9, 3, 2, 3] if n >= 17 else [2] if n == 2 else []
        images.append(grid_image(rng, pick, k1, D, n_single=n - sum(pick)))
        assert len(images[-1]["scores"]) == n
    images.append(grid_image(rng, [9, 3, 2, 1], k1, D, n_single=4, nan_row=True))
    single = grid_image(rng, [2, 3], k1, D, n_single=2)        # a passthrough image
    images.append(single)
    over = {"boxes": rng.uniform(0, 400, (1101, 4)), "scores": rng.uniform(0, 1, 1101), "lp": log_softmax(rng.normal(0, 1, (1101, k1))),
            "src": np.zeros(1101, np.int32), "vars": np.ones(1101), "classes": np.zeros(1101, np.int32)}
    images.insert(4, over)
    (b, s, v, c, offs_d, src, lp), offs = batch(images)
    B = len(images)
    counts = to_dev(np.diff(offs).astype(np.int32))
    passthrough = np.zeros(B, np.int32)
    passthrough[B - 1] = 1
    call = lambda bound, sl=slice(None), o=offs_d[:-1], cn=counts, pt=to_dev(passthrough), args=(b, s, v, c, src, lp): F.fuse_batch(  # noqa: E731
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
        cl = clusters(im["boxes"], im["scores"], im["classes"].astype(np.float64))
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
        one = F.fuse_batch(to_dev(im["boxes"].reshape(-1, 4)), to_dev(im["scores"]), None, to_dev(im["vars"]), to_dev(im["classes"]),
                           to_dev(np.array([0, n], np.int32)), "probEn-log", "v-avg", max_rows=max(n, 1), log_probs=to_dev(im["lp"].reshape(-1, k1)),
                           pool_weights=[0.7, 0.4], row_source=to_dev(im["src"]))
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
        dets.append({"boxes": to_dev(rng.uniform(0, 300, (B, D, 4)).astype(np.float32)), "scores": to_dev(rng.uniform(0, 1, (B, D)).astype(np.float32)),
                     "classes": to_dev(cls), "prob_score": to_dev(rng.dirichlet(np.ones(K + 1), (B, D))[:, :, :K].astype(np.float32)),
                     "class_logits": to_dev(rng.normal(0, 3, (B, D, K + 1)).astype(np.float32)), "vars": to_dev(rng.uniform(0.5, 2, (B, D)).astype(np.float32)),
                     "counts": to_dev(np.array([p[d] for p in pat], np.int32))})
    w = [1.0] * nd
    for temps, logp, vs in ((None, False, None), ((1.5, 0.8, 1.1)[:nd], False, (0.5, 2.0, 1.5)[:nd]), ((1.5, 0.8, 1.1)[:nd], True, (0.5, 2.0, 1.5)[:nd])):
        ref = F.pack_rows(dets, 2, temps, log_posteriors=logp, variance_scales=vs or [1.0] * nd)
        got = F.pack_rows(dets, 2, temps, log_posteriors=logp, variance_scales=vs or [1.0] * nd, pool_weights=w)
        bare = F.pack_rows(dets, 2, temps, log_posteriors=logp, variance_scales=None, pool_weights=w) if vs is None else None
        torch.cuda.synchronize()
        assert len(got) == len(ref) + 1
        cnt = ref[6].cpu().numpy()
        S = nd * D
        live = to_dev((np.arange(S)[None] < cnt[:, None]).reshape(-1))
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
    live = to_dev((np.arange(S)[None] < cnt[:, None]).reshape(-1))
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
    lp = log_softmax(rng.normal(0, 3, (N, k1)).astype(np.float32))
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
    args = (to_dev(lp), to_dev(src), to_dev(members), to_dev(offs), to_dev(labels))
    lpd = None if lprior is None else to_dev(lprior)
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
    nll, grad, bad, _ = Cal.pool_nll(to_dev(lp), to_dev(src), to_dev(members), to_dev(offs), to_dev(labels), cand)
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
    return tuple(to_dev(case[k]) for k in ("log_probs", "row_source", "member_rows", "cluster_offsets", "labels"))


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
    out = F.fuse_batch(to_dev(boxes), to_dev(np.exp(lp.max(1))), None, to_dev(np.ones(N)), to_dev(np.zeros(N, np.int32)), to_dev(offs), "probEn-log", "avg",
                       max_rows=3, log_probs=to_dev(lp), pool_weights=weights, row_source=to_dev(case["row_source"]))
    assert int((out["counts"] != 1).sum()) == 0
    first = to_dev(offs[:-1].astype(np.int64))
    return out["scores"][first].double(), (out["classes"][first].int() == to_dev(case["labels"])).int()


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
    from proben_amd import calibration as C
    from proben_amd.cli import demo_probEn, save_predictions
    root = tmp_path / "val"
    write_flir(root, 6, 96, 120, (150, 180))
    names = ["thermal_only", "early_fusion"]
    paths = [fuse_inputs.weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
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
    nll, _, bad, _ = Cal.pool_nll(to_dev(np.concatenate(lp)), to_dev(np.array(src, np.int32)), to_dev(np.array(mem, np.int32).reshape(-1)),
                                  to_dev(np.arange(0, 2 * C + 1, 2, dtype=np.int32)), to_dev(np.array(lab, np.int32)),
                                  [[1.0, 1.0], weights], None if prior is None else to_dev(np.log(np.asarray(prior, np.float64))))
    assert bad == 0
    return C, nll / C


def test_fit_temperature_and_report_drivers(tmp_path, capsys):
    """fit_temperature --with-pool-weights writes the key and what goes with it, calibration_report prints the held-out fused NLL per
    cluster with and without the weights and fuses its "after" rows with them, and demo_probEn picks the fitted key up."""
    from proben_amd import calibration as Cal
    from proben_amd.cli import calibration_report, demo_probEn, fit_temperature
    root, files, preds, labels = dependent_files(tmp_path)
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
