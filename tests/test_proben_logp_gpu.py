"""Log-posterior ProbEn (score_fusion "probEn-log": pe_proben_pack_log_posteriors, pe_log_softmax, pe_proben_fuse_batch_logp) on the GPU.

The comparator is never the code under test: oracle.proben (pinned to the reference's own outputs) where `probEn` is finite, and an
the NumPy restatement of the header's formulas in np.longdouble (tests/fuse_ref.py) elsewhere.  u = 2^-53 throughout."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from fuse_inputs import (calibrated_infos, detector_rows, fuse_logp, image_rows, load_case, log_full, logit_rows, saturated_images, weights,
                         write_flir)
from fuse_ref import BOX, LD, U, clusters, restate, ulp32

pytestmark = pytest.mark.gpu


# ---- item 2: equals probEn where probEn is sound ----------------------------------------------------------------------------------

@pytest.mark.parametrize("box", BOX)
@pytest.mark.parametrize("golden", ["proben_cases.npz", "proben_saturated.npz"])
def test_equals_proben_where_proben_is_finite(golden_dir, golden, box):
    """log_probs = log([p, 1 - sum p]) (float64, formed here) through pe_proben_fuse_batch_logp against oracle.proben on ["probEn", box]:
    keep sets, counts and boxes identical on every row (the clustering and the box rules never see the fused score); where the oracle's
    score is finite the class is identical and the float32 scores are within 1 ulp32 (the float64 results differ in rounding only: exp of
    a sum of logs against exp of the same sum less its maximum).  Both clustering forms."""
    from oracle import proben as O
    z = np.load(os.path.join(golden_dir, golden))
    n = int(z["num_cases"])
    cases = [load_case(z, ci) for ci in range(n)]
    lps = [log_full(O.concat_infos(infos)[3]) for infos in cases]
    finite = worst = 0
    for bound in (None, 1100):
        out, offs = fuse_logp(cases, lps, box, max_rows=bound)
        for ci, infos in enumerate(cases):
            keep, es, eb, ec = O.nms_bayesian(*O.concat_infos(infos), 0.5, "probEn", box)
            gk, gb, gs, gc = image_rows(out, offs, ci)
            assert int(out["counts"][ci]) == len(keep), (golden, ci)
            np.testing.assert_array_equal(gk, keep, err_msg=f"{golden} case {ci}")
            np.testing.assert_array_equal(gb, eb, err_msg=f"{golden} case {ci} boxes")
            ok = np.isfinite(es)
            want = es.astype(np.float32)
            np.testing.assert_array_equal(gc[ok], ec[ok].astype(np.float32), err_msg=f"{golden} case {ci} classes")
            assert np.isfinite(gs[ok]).all()
            err = np.abs(gs[ok].astype(np.float64) - want[ok].astype(np.float64)) / ulp32(want[ok])
            finite += int(ok.sum())
            worst = max(worst, float(err.max()) if ok.any() else 0.0)
            assert (err <= 1.0).all(), (golden, ci, gs[ok], want[ok])
    print(f"{golden} {box}: {finite} finite rows, largest score difference {worst:.1f} ulp32")
    assert finite > 0


def test_binary_vectors_k1(golden_dir):
    """K = 1: the two columns [fg, bg] are the binary form (demo_probEn.py:24-30).  The new mode reports max(fg, bg) and its index where
    bayesian_fusion reports fg, so binary_out = w compares as max(w, 1 - w) / class (w < 1 - w); only where binary_out is finite."""
    from oracle import proben as O
    z = np.load(os.path.join(golden_dir, "proben_saturated.npz"))
    vecs = np.split(z["binary_in"], np.cumsum(z["binary_len"])[:-1])
    checked = 0
    for v, w in zip(vecs, z["binary_out"]):
        if not np.isfinite(w):
            continue
        rows = len(v)
        for perm in itertools.permutations(range(rows)):       # an input order whose clustering puts v in cluster order
            sc = v[list(perm)]
            od = O.order_desc(sc)
            if [perm[i] for i in od[1:]] + [perm[od[0]]] == list(range(rows)):
                break
        else:
            pytest.fail(f"no input order gives the cluster order of {v}")
        info = {"img_name": "x", "bbox": np.tile([[10.0, 10.0, 50.0, 60.0]], (rows, 1)), "score": sc, "class": np.zeros(rows, int),
                "prob": sc[:, None], "vars": np.ones((rows, 1))}
        empty = dict(info, bbox=np.zeros((0, 4)), score=np.zeros(0), prob=np.zeros((0, 1)), vars=np.zeros((0, 1)), **{"class": np.zeros(0, int)})
        out, offs = fuse_logp([[info, empty]], [log_full(sc[:, None])], "avg")
        assert int(out["counts"][0]) == 1
        got, cls = float(out["scores"][0]), float(out["classes"][0])
        want = np.float32(max(w, 1.0 - w))
        assert cls == (1.0 if 1.0 - w > w else 0.0), (v, cls, w)
        assert abs(got - float(want)) <= ulp32(want), (v, got, want)
        checked += 1
    assert checked >= 5


# ---- item 3 / 5 / 6: saturated logits ----------------------------------------------------------------------------------------------

def _check_against_restatement(cal, out, offs, log_prior=None):
    """Every fused row of `out` against fuse_ref.restate on the image's own clustering.  Returns (rows, clusters by size, largest observed error
    in units of its bound).  The float32 exit rounds once more: half an ulp32 of the expected score on top of the float64 bound."""
    rows, worst, sizes = 0, 0.0, {}
    for i, (infos, lp) in enumerate(cal):
        from oracle.proben import concat_infos
        b, s, c, _, _ = concat_infos(infos)
        cl = clusters(b, s, c)
        gk, gb, gs, gc = image_rows(out, offs, i)
        np.testing.assert_array_equal(gk, [p for p, _ in cl])
        for r, (piv, mem) in enumerate(cl):
            sizes[len(mem)] = sizes.get(len(mem), 0) + 1
            if len(mem) == 1:           # a cluster of one keeps its row's score and class, prior or not
                assert gs[r] == np.float32(s[piv]) and gc[r] == c[piv]
                continue
            w = restate(lp, mem, log_prior=log_prior)
            want, j, bound = w["score"], w["cls"], w["score_bound"]
            tol = 0.5 * ulp32(float(want)) * (1 + 2.0 ** -20) + bound * U * float(want)
            err = abs(LD(gs[r]) - want)
            worst = max(worst, float(err / tol))
            assert err <= tol, (i, r, len(mem), gs[r], float(want), float(err), tol)
            assert gc[r] == j, (i, r, gc[r], j)
            rows += 1
    return rows, sizes, worst


def test_defined_where_proben_is_not():
    """Condition, not a measurement: on saturated rows every fused score of the new route is finite and in (0, 1], while the `probEn`
    route over the same detections (the float32 prob_score of the same logits, background = 1 - sum p) gives non-finite scores.

    Scores and classes against the longdouble restatement within its score bound (tests/fuse_ref.py) - the losing columns' large sums
    enter weighted by their own posterior s_j ~ e^-30 - plus the half ulp32 of the float32 exit, which dominates: a float64 error of a
    few hundred u is 1e-14 relative, the exit's rounding 6e-8.  Measured on an MI355X: see DESIGN.md section 11."""
    from proben_amd import fusion as F
    sat = saturated_images()
    below, exact, over = sat["sum_kinds"]
    assert below > 0 and exact > 0 and over > 0, sat["sum_kinds"]          # the float32 route meets sum p < 1, == 1 and > 1
    # the probEn route on the float32 rows
    b, s, p, v, c, offs = F.pack_infos([infos for infos, _ in sat["images"]])
    old = F.fuse_batch(b, s, p, v, c, offs, "probEn", "v-avg")
    oh = offs.cpu().numpy()
    old_scores = np.concatenate([image_rows(old, oh, i)[2] for i in range(len(sat["images"]))])
    bad = int((~np.isfinite(old_scores)).sum())
    assert bad > 0, "the inputs are too easy: probEn is finite everywhere"
    # the new route on the same detections' logits
    cal = calibrated_infos()
    for box in BOX:
        out, offs2 = fuse_logp([i for i, _ in cal], [lp for _, lp in cal], box)
        new_scores = np.concatenate([image_rows(out, offs2, i)[2] for i in range(len(cal))])
        assert len(new_scores) == len(old_scores)
        assert np.isfinite(new_scores).all() and (new_scores > 0).all() and (new_scores <= 1).all(), new_scores[~np.isfinite(new_scores)]
        rows, sizes, worst = _check_against_restatement(cal, out, offs2)
        assert sizes.get(1, 0) > 0 and sizes.get(2, 0) > 0 and sum(n for m, n in sizes.items() if m >= 8) > 0, sizes
        print(f"{box}: probEn route {bad} non-finite of {len(old_scores)} fused rows; probEn-log 0 of {len(new_scores)}; {rows} clusters of "
              f"m > 1 checked (sizes {sorted(sizes.items())}), largest error {worst:.3f} of its bound; float32 sums below/exactly/above 1: {sat['sum_kinds']}")


def test_clustering_form_and_batching_move_no_bit():
    """The bit-matrix walk (bound = the longest image) and the sequential walk (max_rows = 1100) give the same bytes in the new mode, and
    an image's result does not depend on which images share its launch."""
    cal = calibrated_infos()
    infos, lps = [i for i, _ in cal], [lp for _, lp in cal]
    prior = [0.3, 0.2, 0.1, 0.4]
    tight, offs = fuse_logp(infos, lps, "s-avg", class_prior=prior)
    wide, _ = fuse_logp(infos, lps, "s-avg", max_rows=1100, class_prior=prior)
    assert torch.equal(tight["counts"], wide["counts"]) and int(tight["counts"].sum()) > 100
    rev, offs_r = fuse_logp(infos[::-1], lps[::-1], "s-avg", class_prior=prior)
    n = len(infos)
    for i in range(n):
        a, w = image_rows(tight, offs, i), image_rows(wide, offs, i)
        r = image_rows(rev, offs_r, n - 1 - i)
        for x, y, z in zip(a, w, r):
            assert x.tobytes() == y.tobytes() == z.tobytes(), i
    for i in (0, 7, 47):            # alone in its launch
        one, o1 = fuse_logp([infos[i]], [lps[i]], "s-avg", class_prior=prior)
        for x, y in zip(image_rows(tight, offs, i), image_rows(one, o1, 0)):
            assert x.tobytes() == y.tobytes(), i
    from proben_amd import _lib
    with pytest.raises(_lib.HipLibraryError, match="LDS"):
        fuse_logp(infos, lps, "s-avg", max_rows=2000)


def test_class_prior():
    """A uniform prior subtracts one constant from every column: against None the keep sets, boxes and classes are identical and the
    scores agree within the bound of fuse_ref.restate (each against the same longdouble value; not necessarily the same bytes).  A non-uniform
    prior against the restatement; clusters of one are untouched (checked row by row in _check_against_restatement)."""
    cal = calibrated_infos((1.3, 0.8, 2.0))
    infos, lps = [i for i, _ in cal], [lp for _, lp in cal]
    none, offs = fuse_logp(infos, lps, "v-avg")
    uni, _ = fuse_logp(infos, lps, "v-avg", class_prior=[1, 1, 1, 1])
    assert torch.equal(none["counts"], uni["counts"])
    for i in range(len(infos)):
        a, b = image_rows(none, offs, i), image_rows(uni, offs, i)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes()
    r0, _, w0 = _check_against_restatement(cal, none, offs)
    r1, _, w1 = _check_against_restatement(cal, uni, offs, np.log(np.full(4, 0.25)))
    # the same longdouble value either way (the uniform prior cancels in the softmax): uni is also within None's bound
    r2, _, w2 = _check_against_restatement(cal, uni, offs)
    prior = np.array([0.02, 0.5, 0.08, 0.4])
    out, _ = fuse_logp(infos, lps, "v-avg", class_prior=prior.tolist())
    r3, _, w3 = _check_against_restatement(cal, out, offs, np.log(prior / prior.sum()))
    moved = sum(int((image_rows(out, offs, i)[2] != image_rows(none, offs, i)[2]).sum()) for i in range(len(infos)))
    assert moved > 0, "the non-uniform prior changed no score"
    print(f"prior: {r0} clusters; largest error / bound: none {w0:.3f}, uniform {w1:.3f} (against the prior-free value {w2:.3f}), "
          f"non-uniform {w3:.3f}; {moved} scores moved by the non-uniform prior")
    from proben_amd import fusion as F
    with pytest.raises(ValueError, match=r"lists 3 entries for K \+ 1 = 4"):
        fuse_logp(infos, lps, "v-avg", class_prior=[0.2, 0.3, 0.5])
    # fusion() (one image, lists in) takes the same route
    one = [dict(d, class_logits=saturated_images()["images"][0][1][k:k + len(d["score"])].tolist())
           for d, k in zip(infos[0], np.cumsum([0] + [len(d["score"]) for d in infos[0]]))]
    fb, fs, fc = F.fusion(["probEn-log", "v-avg"], *one, temperatures=[1.3, 0.8, 2.0][:len(one)], class_prior=prior.tolist())
    want = image_rows(out, offs, 0)
    assert fs.numpy().tobytes() == want[2].tobytes() and fc.numpy().tobytes() == want[3].tobytes()
    assert np.asarray(fb).tobytes() == want[1].tobytes()


# ---- item 4: the pack and the flat log-softmax ----------------------------------------------------------------------------------------

def _np_log_softmax(lg32, T):
    z = lg32.astype(np.float64) / T
    d = z - z.max(1, keepdims=True)
    s = np.exp(d).sum(1, keepdims=True)
    return d - np.log(s), d, s


def _log_posterior_bound(K, d, s, lp):
    """|device - NumPy| per element, first order.  d = z - m is the same IEEE operations on both sides: identical.  Either side's sum s
    of the K + 1 exponentials is within (2 + K) u relative (exp within 1 ulp <= 2 u, K additions of partial sums <= s, in any order),
    so log(s) moves by that much ABSOLUTELY, plus its own 1 ulp (<= 2 u |log s|); the subtraction rounds once (u |lp|).  Two sides:
    2 ((K + 2) + 2 |log s| + |lp|) u - the kind of bound section 10 derives for the probabilities (2 (K + 5) u relative), absolute here
    because log p sits next to 0 on a saturated row."""
    return 2 * ((K + 2) + 2 * np.abs(np.log(s)) + np.abs(lp)) * U * (1 + 1e-3)


@pytest.mark.parametrize("Kc", [3, 1, 80])
@pytest.mark.parametrize("T", [0.25, 1.0, 1.7])
def test_log_softmax_against_numpy_float64(Kc, T):
    """pe_log_softmax on 10^5 rows spanning +-60 with exact ties and flat rows (fuse_inputs.logit_rows) against NumPy's
    float64 log_softmax, within _log_posterior_bound; exp of it is the calibrated probability to the same order; every value finite."""
    from proben_amd.calibration import calibrated_probs, log_posteriors
    rng = np.random.default_rng(7 * Kc + int(T * 100))
    lg = logit_rows(rng, 100_000, Kc)
    dl = torch.from_numpy(np.ascontiguousarray(lg)).cuda()
    got = log_posteriors(dl, T).cpu().numpy()
    want, d, s = _np_log_softmax(lg, T)
    assert got.dtype == np.float64 and got.shape == want.shape and np.isfinite(got).all() and (got <= 0).all()
    err, bound = np.abs(got - want), _log_posterior_bound(Kc, d, s, want)
    print(f"K={Kc} T={T}: largest |difference| {err.max() / U:.2f} u, largest error / bound {(err / bound).max():.3f}, most negative {want.min():.1f}")
    assert (err <= bound).all(), (err / bound).max()
    p, bg = calibrated_probs(dl, T)
    full = np.concatenate([p.cpu().numpy(), bg.cpu().numpy()[:, None]], 1)
    # exp(log p) against p: the one-sided bound on log p is a relative one on its exp, + exp's 1 ulp, + p's own (K + 5) u of section 10
    rel = ((Kc + 2) + 2 * np.abs(np.log(s)) + np.abs(want) + 2 + (Kc + 5)) * U * 1.01
    assert (np.abs(np.exp(got) - full) <= full * rel).all()
    again = log_posteriors(dl, T).cpu().numpy()
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("Kc,temps", [(3, (1.5, 0.8)), (3, (1.0, 1.0)), (1, (0.7, 2.5))])
def test_pack_log_posteriors_parity(Kc, temps):
    """On the synthetic detectors' rows every output pe_proben_pack_log_posteriors shares with pe_proben_pack_logits is byte-identical
    (boxes, scores, probabilities, variances, classes on the live rows; offsets, counts, single-source flags whole); out_log_probs is
    pe_log_softmax of the same logits byte for byte, and within _log_posterior_bound of NumPy."""
    from proben_amd import fusion as F
    from proben_amd.calibration import log_posteriors
    dets = detector_rows(Kc)
    mc = 2 if Kc == 3 else 0
    ref = F.pack_rows(dets, mc, temps)
    got = F.pack_rows(dets, mc, temps, log_posteriors=True)
    torch.cuda.synchronize()
    assert len(ref) == 8 and len(got) == 9
    cnt = ref[6].cpu().numpy()
    S = len(dets) * dets[0]["scores"].shape[1]
    live = torch.from_numpy((np.arange(S)[None] < cnt[:, None]).reshape(-1)).cuda()
    assert int(live.sum()) > 20
    for i in (5, 6, 7):
        assert torch.equal(ref[i], got[i])
    for i in (0, 1, 2, 3, 4):
        a, b = ref[i][live].contiguous().cpu().numpy(), got[i][live].contiguous().cpu().numpy()
        assert a.tobytes() == b.tobytes(), i
    want, lgs = [], []
    for b in range(len(cnt)):
        for d, T in zip(dets, temps):
            c = int(d["counts"][b])
            lg, cls = d["class_logits"][b, :c], d["classes"][b, :c]
            keep = cls <= mc
            if int(keep.sum()):
                want.append(log_posteriors(lg[keep], T))
                lgs.append((lg[keep].cpu().numpy(), T))
    lp = got[8][live].contiguous()
    assert lp.shape[1] == Kc + 1 and torch.equal(lp, torch.cat(want))
    k, lp_h = 0, lp.cpu().numpy()
    for lg, T in lgs:
        w, d, s = _np_log_softmax(lg, T)
        assert (np.abs(lp_h[k:k + len(lg)] - w) <= _log_posterior_bound(Kc, d, s, w)).all()
        k += len(lg)


# ---- item 7: the drivers -------------------------------------------------------------------------------------------------------------

def test_fuse_detections_is_pack_plus_fuse_and_equals_the_file_route():
    """fuse_detections in the new mode = pe_proben_pack_log_posteriors + pe_proben_fuse_batch_logp on the detectors' rows; and the file
    route (late_fusion over prediction dicts holding the same detections as lists, the J1 schema) gives the same rows, bit for bit."""
    from proben_amd import fusion as F
    from proben_amd.late_fusion import late_fusion
    dets = detector_rows(3)
    temps, prior = (1.5, 0.8), [0.1, 0.3, 0.2, 0.4]
    B, D = dets[0]["scores"].shape
    S = 2 * D
    for tp, pr in ((temps, prior), (None, None)):
        dev = F.fuse_detections(dets, "probEn-log", "s-avg", temperatures=tp, class_prior=pr)
        torch.cuda.synchronize()
        cnt = dev["counts"].cpu().numpy()
        assert cnt.sum() > 0
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
        via = late_fusion(j1, ["probEn-log", "s-avg"], temperatures=tp, class_prior=pr)
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


def test_demo_proben_log_two_stage_and_one_pass(tmp_path, capsys):
    """demo_probEn --score_fusion probEn-log: the two-stage route (prediction files) and --one-pass give the same AP table and the same
    evaluation rows on the synthetic FLIR set of fuse_inputs.write_flir; --calibration written by fit_temperature --with-prior supplies
    temperatures and the class prior; --class_prior overrides it; the result differs from plain probEn's."""
    from proben_amd import calibration as C
    from proben_amd.cli import demo_probEn, fit_temperature, save_predictions
    root = tmp_path / "val"
    write_flir(root, 6, 96, 120, (150, 180))
    names = ["thermal_only", "early_fusion"]
    paths = [weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
    pdir = tmp_path / "pred"
    for m, p in zip(names, paths):
        save_predictions.main(["--dataset_path", str(root), "--fusion_method", m, "--model_path", p, "--prediction_path", str(pdir), "--batch", "4"])
    files = [str(pdir / f"val_{m}_predictions.json") for m in names]

    def two_stage(tag, extra):
        out = tmp_path / f"out2_{tag}"
        res = demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names),
                                "--outfolder", str(out), "--dataset_name", f"flir_logp2_{tag}"] + extra)
        return out, res

    def one_pass(tag, extra):
        out = tmp_path / f"out1_{tag}"
        res = demo_probEn.main(["--one-pass", "--dataset_path", str(root), "--detectors", ",".join(names), "--model_paths", ",".join(paths),
                                "--workers", "2", "--batch", "4", "--outfolder", str(out), "--dataset_name", f"flir_logp1_{tag}"] + extra)
        return out, res

    def same(o1, o2):
        assert (o1 / "FLIR_probEn_eval.json").read_bytes() == (o2 / "FLIR_probEn_eval.json").read_bytes()
        r1, r2 = json.load(open(o1 / "coco_instances_results.json")), json.load(open(o2 / "coco_instances_results.json"))
        assert len(r1) == len(r2) > 0
        assert [(r["image_id"], r["category_id"], r["score"]) for r in r1] == [(r["image_id"], r["category_id"], r["score"]) for r in r2]
        np.testing.assert_allclose([r["bbox"] for r in r1], [r["bbox"] for r in r2], rtol=1e-6, atol=1e-4)
        return r1

    plain_out, _ = two_stage("plain", [])
    log = ["--score_fusion", "probEn-log"]
    o2, res2 = two_stage("log", log)
    o1, res1 = one_pass("log", log)
    assert res2["temperatures"] == res1["temperatures"] == dict(zip(names, [1.0, 1.0])) and "class_prior" not in res2
    rows = same(o1, o2)
    assert all(np.isfinite(r["score"]) and 0 < r["score"] <= 1 for r in rows)
    rp = json.load(open(plain_out / "coco_instances_results.json"))
    assert [r["score"] for r in rp] != [r["score"] for r in rows]
    # a calibration file with a prior
    cal = tmp_path / "calibration.json"
    fit_temperature.main(["--predictions", *files, "--dataset_path", str(root), "--holdout", "0.5", "--out", str(cal), "--with-prior"])
    rec = C.load(cal)
    assert len(rec["class_prior"]) == 4 and abs(sum(rec["class_prior"]) - 1) < 1e-12 and min(rec["class_prior"]) > 0
    assert sum(rec["class_prior_counts"]) == sum(rec["rows"].values())
    o2c, res2c = two_stage("cal", log + ["--calibration", str(cal)])
    o1c, res1c = one_pass("cal", log + ["--calibration", str(cal)])
    assert res2c["class_prior"] == res1c["class_prior"] == rec["class_prior"]
    assert res2c["temperatures"] == {m: rec["detectors"][m] for m in names}
    same(o1c, o2c)
    o2p, res2p = two_stage("prior", log + ["--calibration", str(cal), "--class_prior", "0.7,0.1,0.1,0.1", "--box_fusion", "argmax"])
    o1p, res1p = one_pass("prior", log + ["--calibration", str(cal), "--class_prior", "0.7,0.1,0.1,0.1", "--box_fusion", "argmax"])
    np.testing.assert_allclose(res2p["class_prior"], [0.7, 0.1, 0.1, 0.1], rtol=1e-15)
    same(o1p, o2p)
    # without --with-prior the file has no prior and the mode runs uniform
    cal0 = tmp_path / "calibration0.json"
    fit_temperature.main(["--predictions", *files, "--dataset_path", str(root), "--holdout", "0.5", "--out", str(cal0)])
    assert "class_prior" not in json.load(open(cal0)) and "class_prior_counts" not in json.load(open(cal0))
    _, res0 = two_stage("cal0", log + ["--calibration", str(cal0)])
    assert "class_prior" not in res0
    # files without logits are refused by name
    d = json.load(open(files[0]))
    d["class_logits"] = [[[] for _ in rows_] for rows_ in d["boxes"]]
    json.dump(d, open(files[0], "w"))
    with pytest.raises(ValueError, match=r"val_thermal_only_predictions\.json: no class_logits"):
        two_stage("nologits", log)


def test_default_pipeline_still_produces_the_plain_route():
    """FramePairPipeline's default construction: what it returns is pe_proben_pack_detections + pe_proben_fuse_batch (probEn, v-avg) on
    its own detections, called here through this library's C-ABI directly - the default path does not route through the new mode.
    That is all this test shows.  That pe_proben_fuse_batch itself kept its bits is the business of the unchanged golden tests
    (tests/test_proben_gpu.py, test_proben_real_rows_gpu.py), not of this one."""
    import ctypes
    import proben_amd
    from proben_amd import _lib
    from proben_amd.pipeline import FramePairPipeline
    from proben_amd.synthetic import synthetic_images
    models = []
    for seed in (1, 2):
        cfg = proben_amd.get_cfg()
        cfg.MODEL.RESNETS.DEPTH = 50
        cfg.MODEL.ROI_BOX_HEAD.OUTPUT_LOGITS = True
        cfg.MODEL.ROI_HEADS.ENABLE_GAUSSIANNLLOSS = True
        cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 3, 0.5
        cfg.MODEL.WEIGHTS = f"synthetic://{seed}"
        models.append(proben_amd.DefaultPredictor(cfg).model)
    fr = torch.from_numpy(synthetic_images(4, height=256, width=320, seed=5)).cuda()
    dets, fused = FramePairPipeline(models)([fr, fr], [(256, 320)] * 4, (800, 1000))
    torch.cuda.synchronize()
    B, D = dets[0]["scores"].shape
    S, Kc = 2 * D, dets[0]["prob_score"].shape[2]

    def arr(key):
        return (ctypes.c_void_p * 2)(*[d[key].data_ptr() for d in dets])
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    ob, os_, op, ov, oc, ooff, ocnt, osingle = f64(B * S, 4), f64(B * S), f64(B * S, Kc), f64(B * S), i32(B * S), i32(B), i32(B), i32(B)
    L, P = _lib.lib(), _lib.ptr
    _lib.check(L.pe_proben_pack_detections(arr("boxes"), arr("scores"), arr("classes"), arr("prob_score"), arr("vars"), arr("counts"), 2, B, D,
                                           Kc, 2, S, P(ob), P(os_), P(op), P(ov), P(oc), P(ooff), P(ocnt), P(osingle), _lib.stream()), "pack")
    wb, ws, wc, wk, wn = f64(B * S, 4), torch.empty(B * S, device="cuda"), torch.empty(B * S, device="cuda"), i32(B * S), i32(B)
    _lib.check(L.pe_proben_fuse_batch(P(ob), P(os_), P(op), P(ov), P(oc), P(ooff), P(ocnt), P(osingle), B, Kc, S, 0, 0, 0.5, 640.0, 512.0,
                                      P(wb), P(ws), P(wc), P(wk), P(wn), _lib.stream()), "fuse")
    torch.cuda.synchronize()
    assert torch.equal(fused["counts"], wn) and int(wn.sum()) > 0
    live = (torch.arange(S, device="cuda")[None] < wn[:, None]).reshape(-1)
    for got, want in ((fused["boxes"], wb), (fused["scores"], ws), (fused["classes"], wc), (fused["keep"], wk)):
        assert got[live].contiguous().cpu().numpy().tobytes() == want[live].contiguous().cpu().numpy().tobytes()
