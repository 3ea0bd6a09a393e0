"""tests/boxhead_cases.py and oracle/detector.py on the CPU: the restatement of csrc/boxhead.hip under the right rule is the oracle
(select_detections + postprocess) wherever the oracle has an answer, every case builder contains what it claims to contain, and
every family's expected output changes in an exactly compared field under a deliberately wrong rule - so
tests/test_boxhead_edges_gpu.py, which compares the kernels with the restatement, can tell the two apart."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import boxhead_cases as C
from oracle import detector as D

TOL_SCORE = dict(rtol=2e-6, atol=1e-7)      # tests/test_ops_gpu.py::test_boxhead_matches_oracle_quirks: scores and probs
TOL_BOX = dict(rtol=1e-5, atol=2e-4)        # boxes
TOL_VAR = dict(rtol=2e-6)                   # vars

CASE_FIX = [(name, f) for name in C.names() for f in C.get(name).fix_vars]


def oracle_image(case, n, fix_vars, keep_count):
    K, R = case.K, C.live_rows(case, n)
    h = torch.from_numpy(np.array(case.head[n, :R]))
    spec = D.DetectorSpec(num_classes=K, score_thresh=case.thr, nms_thresh=0.5 if case.keep_mode == "nms" else 2.0,   # IoU <= 1: 2.0 never suppresses
                          detections_per_image=min(keep_count, case.max_det), fix_vars=bool(fix_vars))
    hw = tuple(case.image_hw[n].tolist())
    with np.errstate(all="ignore"):
        det = D.select_detections(h[:, :K + 1], h[:, K + 1:5 * K + 1], torch.exp(h[:, 5 * K + 1:5 * K + 2]),
                                  torch.from_numpy(np.array(case.props[n, :R])), hw, spec)
    return D.postprocess(det, hw, tuple(case.out_hw[n].tolist()))


# ------------------------------------------------------------------------------------------------ the restatement is the oracle
@pytest.mark.parametrize("name,fix_vars", CASE_FIX)
def test_the_restatement_under_the_right_rule_is_the_oracle(name, fix_vars):
    """Count, classes, class_logits and roi_index (the post-filter row id) exact, floats within the project's tolerances, boxes bit
    for bit where the case has exact boxes.  Where Case.oracle says the reference has no answer, the reason is checked instead:
    the cap bites, or Q3's candidate ids leave the live rows - and then the oracle raises IndexError."""
    case = C.get(name)
    res = C.want(name, fix_vars)
    if not case.oracle[fix_vars]:
        capped = any(cand["total"] > case.cand_max for cand, _, _, _ in res)
        q3_out = any(len(keep) and int(keep.max()) >= C.live_rows(case, n) for n, (_, keep, _, _) in enumerate(res))
        assert capped or (q3_out and not fix_vars)
        if not capped:
            with pytest.raises(IndexError):
                for n, (_, _, kc, _) in enumerate(res):
                    oracle_image(case, n, fix_vars, kc)
        return
    for n, (cand, keep, kc, det) in enumerate(res):
        want = oracle_image(case, n, fix_vars, kc)
        assert det["count"] == len(want["boxes"]), (n, det["count"], len(want["boxes"]))
        np.testing.assert_array_equal(det["classes"], want["classes"].numpy())
        np.testing.assert_array_equal(det["frow"], want["roi_index"].numpy())
        np.testing.assert_array_equal(det["logits"], want["class_logits"].numpy().reshape(-1, case.K + 1))
        np.testing.assert_allclose(det["scores"], want["scores"].numpy(), **TOL_SCORE)
        np.testing.assert_allclose(det["probs"], want["prob_score"].numpy().reshape(-1, case.K), **TOL_SCORE)
        np.testing.assert_allclose(det["vars"], want["vars"].numpy().reshape(-1), **TOL_VAR)
        np.testing.assert_allclose(det["boxes"], want["boxes"].numpy().reshape(-1, 4), **TOL_BOX)
        if case.exact_boxes:
            np.testing.assert_array_equal(det["boxes"].astype(np.float32), want["boxes"].numpy().reshape(-1, 4))


# ------------------------------------------------------------------------------------------------ what every case claims
@pytest.mark.parametrize("name", C.names())
def test_case_inputs_are_what_the_module_says(name):
    """The planted rows are the only invalid live rows; finite logits lie on the 2^-12 grid; every foreground probability keeps
    its margin from the threshold (planted ties aside) and the scores of one image their gap; every variance names its row; where
    the case has exact boxes the float32 decode (oracle.detector.apply_deltas) and the float64 decode agree bit for bit."""
    case = C.get(name)
    K = case.K
    C.check_scores(case, margin=5e-5 if C.FAMILY_OF[name] == "threshold_tie" else C.MARGIN)
    for n in range(len(case.pcnt)):
        R = C.live_rows(case, n)
        cand = C.candidates(case, n)
        planted = sorted(r for (m, r) in case.claims["invalid"] if m == n and r < R)
        assert np.nonzero(~cand["valid"])[0].tolist() == planted
        lg = case.head[n, :R, :K + 1].astype(np.float64)
        fin = np.isfinite(lg)
        assert (lg[fin] * 4096 == np.round(lg[fin] * 4096)).all() and not np.isnan(lg).any() or C.FAMILY_OF[name] == "dead_memory"
        live_var = np.exp(case.head[n, :R, 5 * K + 1].astype(np.float64))
        np.testing.assert_array_equal(C.var_row(case, live_var.astype(np.float32)), np.arange(R))
        assert np.isfinite(live_var.astype(np.float32)).all()
        if case.exact_boxes and R:
            v = cand["valid"]
            d = torch.from_numpy(np.array(case.head[n, :R, K + 1:5 * K + 1][v]))
            b32 = D.apply_deltas(d, torch.from_numpy(np.array(case.props[n, :R][v])), C.REG_W).numpy().reshape(-1, K, 4)
            b64, _ = C.decode64(case.head[n, :R, K + 1:5 * K + 1][v].reshape(-1, K, 4), case.props[n, :R][v])
            np.testing.assert_array_equal(b64.astype(np.float32).astype(np.float64), b64)        # representable
            np.testing.assert_array_equal(b32, b64.astype(np.float32))                          # and what float32 computes
    assert set(case.oracle) == set(case.fix_vars) and len(case.pcnt) in (2, 3)


def test_scan_seam_family():
    kinds = set()
    for P in C.SCAN_P:
        case = C.get(f"scan_P{P}")
        assert case.head.shape[:2] == (3, P) and case.K == 3 and case.thr == 0.5
        planted = {r for _, r in case.claims["invalid"]}
        assert planted == {r for r in C.SEAM_ROWS + (P - 1,) if r < P}
        assert case.pcnt.tolist() == case.claims["counts_drawn"]
        for c in case.pcnt.tolist():
            kinds |= {k for k, v in (("P", P), ("P-1", P - 1), ("1", 1), ("0", 0), ("P+7", P + 7)) if c == v}
            assert c in (P, P - 1, 1, 0, P + 7)
        for n in range(3):
            cand = C.candidates(case, n)
            assert cand["total"] > 0 or not cand["valid"].any()
            if case.pcnt[n] == P + 7:                       # behaves as P
                full = C.candidates(case._replace(pcnt=np.full(3, P, np.int32)), n)
                assert full["total"] == cand["total"] and np.array_equal(full["orow"], cand["orow"])
    assert kinds == {"P", "P-1", "1", "0", "P+7"}, kinds
    big = C.want("scan_P1024", 0)
    assert big[0][0]["total"] > 512 and len(big[0][1]) == 100           # more than one wave of candidates, truncated by max_det
    assert any(det["count"] and (det["frow"] != det["rows"]).any() for _, _, _, det in big)


@pytest.mark.parametrize("stride", [24, 19])
def test_dead_memory_family(stride):
    case = C.get(f"dead_memory_stride{stride}")
    assert case.head.shape == (3, 65, stride) and case.pcnt.tolist() == [40, 0, 40]
    assert np.isnan(case.head[..., 17:]).all()
    for n, R in enumerate(case.pcnt.tolist()):
        assert np.isnan(case.head[n, R:]).all() and np.isnan(case.props[n, R:]).all()
        assert np.isfinite(case.head[n, :R, :17]).sum() >= R * 17 - 8 and np.isfinite(case.props[n, :R]).all()
    res = C.want(f"dead_memory_stride{stride}", 0)
    assert res[1][0]["total"] == 0 and res[1][3]["count"] == 0 and res[0][3]["count"] > 10


def test_quirk_indices_family():
    case = C.get("quirk_indices")
    assert case.head.shape[:2] == (3, 64) and case.max_det == 100 and case.fix_vars == (0, 1)
    for n, (cand, keep, _, det) in enumerate(C.want("quirk_indices", 0)):
        rows = [r for m, r in case.claims["invalid"] if m == n]
        assert len(rows) == 10 and max(rows) < 40
        assert (cand["frow"] != cand["orow"]).mean() > 0.5
        three = (det["cid"] != det["frow"]) & (det["frow"] != det["rows"])
        assert three.mean() > 0.5, three.mean()
        fixed = C.want("quirk_indices", 1)[n][3]
        assert (det["vrow"] == det["cid"]).all() and (fixed["vrow"] == fixed["rows"]).all()
        assert (det["vrow"] != fixed["vrow"]).mean() > 0.5


@pytest.mark.parametrize("K", C.TIE_K)
def test_threshold_tie_family(K):
    """The tie rows have p == 0.5 exactly in float32 - in the kernel's own sequence and in torch's softmax - and do not pass; the
    rows one and three grid steps above do."""
    name = f"threshold_tie_K{K}"
    case = C.get(name)
    assert case.thr == 0.5 and case.head.shape[:2] == (2, 8)
    for n, (cand, _, _, _) in enumerate(C.want(name, 0)):
        for r in case.claims["ties"] + case.claims["passes"]:
            l = case.head[n, r, :K + 1]
            k = 0 if r < 2 else K - 1
            with np.errstate(all="ignore"):
                e = np.exp(l - l.max(), dtype=np.float32)
                s = np.float32(0)
                for v in e:
                    s = np.float32(s + v)
                p32 = np.float32(e[k] / s)
            pt = F.softmax(torch.from_numpy(np.array(l)), dim=-1)[k].item()
            if r in case.claims["ties"]:
                assert p32 == np.float32(0.5) and pt == 0.5 and cand["probs"][r, k] == 0.5
                assert r not in cand["orow"]
            else:
                assert p32 > np.float32(0.5) and pt > 0.5
                assert ((cand["orow"] == r) & (cand["classes"] == k)).sum() == 1


def test_multi_class_family():
    for name, over in [("multi_class_thr0.05", False), ("multi_class_thr0", False), ("multi_class_over", True)]:
        case = C.get(name)
        for n, (cand, keep, _, det) in enumerate(C.want(name, case.fix_vars[0])):
            per_row = np.bincount(cand["orow"], minlength=16)
            assert per_row.max() == 3 and (per_row == 2).any() or over
            assert (np.diff(cand["orow"] * 4 + cand["classes"]) > 0).all()            # row ascending, then class ascending
            assert (cand["total"] > 16) == over and case.oracle == ({1: True} if over else {0: True, 1: True})
    a, b = C.want("multi_class_thr0.05", 0), C.want("multi_class_thr0", 0)
    assert all(y[0]["total"] == x[0]["total"] + 1 for x, y in zip(a, b))             # the small probability passes at 0 only
    assert all((y[0]["probs"][:, :3] == 0).any() for y in b)                         # and p == 0 does not pass thr = 0


def test_q3_overrange_family():
    case = C.get("q3_overrange")
    assert case.fix_vars == (0,) and case.oracle == {0: False} and case.head.shape[:2] == (2, 8) and case.pcnt.tolist() == [4, 5]
    for n, (cand, keep, _, det) in enumerate(C.want("q3_overrange", 0)):
        R = int(case.pcnt[n])
        assert cand["total"] == 3 * R and len(keep) == 3 * R and det["count"] == 3 * R
        assert (det["vrow"] == np.minimum(det["cid"], 7)).all()
        assert ((det["vrow"] >= R) & (det["vrow"] < 7)).any() and (det["cid"] > 7).any()      # dead rows, and the clamp itself
        assert np.isfinite(case.head[n, R:, 16]).all()


@pytest.mark.parametrize("cand_max", C.CAP_MAX)
def test_cap_family(cand_max):
    name = f"cap_{cand_max}"
    case = C.get(name)
    assert case.cand_max == cand_max and case.oracle == {0: False, 1: False}
    wide = case._replace(cand_max=64 * 3)
    for n, (cand, _, _, _) in enumerate(C.want(name, 0)):
        full = C.capped(C.candidates(wide, n))
        assert cand["total"] == len(full["scores"]) > max(C.CAP_MAX)
        for k, v in C.capped(cand).items():
            np.testing.assert_array_equal(v, full[k][:cand_max])
        assert np.bincount(cand["orow"]).max() >= 2


@pytest.mark.parametrize("D_", C.EMPTY_D)
def test_empty_after_clip_family(D_):
    name = f"empty_after_clip_D{D_}"
    case = C.get(name)
    assert case.head.shape[:2] == (3, 130) and case.max_det == D_ and case.keep_mode == "order"
    for n, (cand, keep, kc, det) in enumerate(C.want(name, 0)):
        assert kc == 130 and len(keep) == D_ and cand["total"] == 130
        np.testing.assert_array_equal(cand["orow"][keep], case.claims["place"][n][:D_])     # keep position j is the row of place j
        everything = C.finalize(case, n, cand, keep, 0, C.KEEP_EMPTY)
        b = everything["boxes"].astype(np.float32)
        empty = ~((b[:, 2] - b[:, 0] > 0) & (b[:, 3] - b[:, 1] > 0))
        assert np.nonzero(empty)[0].tolist() == sorted(j for j in case.claims["empties"][n] if j < D_)
        assert det["count"] == D_ - empty.sum()
        kinds = {case.claims["empties"][n][j] for j in np.nonzero(empty)[0].tolist()}
        assert kinds <= set(C.EMPTY_KINDS) and (n != 1 or kinds == set(C.EMPTY_KINDS))      # image 1: all four ways to be empty
        assert np.isfinite(cand["boxes"]).all() and cand["valid"].all()                  # dw = -inf rows stay valid
    e = [case.claims["empties"][n] for n in range(3)]
    assert {0, 63, 64, 127, 128} <= set(e[0]) and set(range(64, 128)) <= set(e[0]) and set(e[2]) == {0, 63, 64, 127, 128}
    assert C.want(name, 0)[1][3]["count"] == 0
    if D_ == 130:
        assert C.want(name, 0)[0][3]["count"] == 63                                       # 62 of round 0, none of round 1, one of round 2


def test_keep_seams_family():
    seen = set()
    for which in ("low", "high"):
        case = C.get(f"keep_seams_{which}")
        assert case.max_det == C.KEEP_D and case.keep_mode == "order"
        for n, (cand, keep, kc, det) in enumerate(C.want(f"keep_seams_{which}", 0)):
            seen.add(kc)
            assert len(keep) == min(kc, C.KEEP_D) and cand["total"] == 80
            assert len(keep) < 3 or ((np.diff(keep) < 0).any() and (np.diff(keep) > 0).any())   # non-monotonic
            assert len(set(keep.tolist())) == len(keep)
    assert seen == {0, 1, 64, 65, C.KEEP_D, C.KEEP_D + 5}


def test_decode_edges_family():
    case = C.get("decode_edges")
    rows, K = case.claims["rows"], 3
    below, at, above = case.claims["clamp_deltas"]
    c32 = np.float32(C.SCALE_CLAMP)
    assert np.float32(below / np.float32(5)) < c32 and np.float32(at / np.float32(5)) == c32 and np.float32(above / np.float32(5)) > c32
    assert np.float32(np.nextafter(below, np.float32(np.inf)) / np.float32(5)) <= c32
    for n, (cand, keep, _, det) in enumerate(C.want("decode_edges", 0)):
        ih, iw = case.image_hw[n].tolist()
        assert np.nonzero(~cand["valid"])[0].tolist() == [rows["dx_big"], rows["dx_nbig"]]
        R = 16
        box, fin = C.decode64(case.head[n, :R, K + 1:5 * K + 1].reshape(R, K, 4), case.props[n, :R])
        for name in ("dx_big", "dx_nbig"):
            r = rows[name]
            assert fin[r].sum() == 2 and fin[r, r % K] and np.isfinite(box[r]).all()      # finite in float64, and in the class that passes
            assert abs(box[r, (r + 1) % K, 0]) > 3.5e38
        by_row = {int(o): cand["boxes"][i] for i, o in enumerate(cand["orow"])}
        ext = lambda r: (by_row[r][2] - by_row[r][0], by_row[r][3] - by_row[r][1])  # noqa: E731
        raw = lambda name: box[rows[name], rows[name] % K]  # noqa: E731
        size = lambda name: raw(name)[2 + (rows[name] + n) % 2] - raw(name)[(rows[name] + n) % 2]  # noqa: E731
        assert np.isclose(size("at"), np.exp(C.SCALE_CLAMP) * [16, 32][(rows["at"] + n) % 2])
        assert np.isclose(size("above"), np.exp(C.SCALE_CLAMP) * [16, 32][(rows["above"] + n) % 2])
        assert np.isclose(size("pinf"), np.exp(C.SCALE_CLAMP) * [16, 32][(rows["pinf"] + n) % 2])
        assert size("below") < np.exp(C.SCALE_CLAMP) * [16, 32][(rows["below"] + n) % 2] * (1 - 1e-3)
        assert ext(rows["dw_ninf"])[0] == 0 and ext(rows["dh_ninf"])[1] == 0
        assert by_row[rows["on_edge"]].tolist() == [iw - 16, 0, iw, 16]
        assert ext(rows["past_edge"])[0] == 0 and by_row[rows["past_edge"]][0] == iw
        assert by_row[rows["negative"]].tolist() == [0, 0, 8, 8]
        dropped = {rows["dw_ninf"], rows["dh_ninf"], rows["past_edge"]}
        assert det["count"] == cand["total"] - 3 and not dropped & set(det["rows"].tolist())


def test_scale_edges_family():
    case = C.get("scale_edges")
    ihw, ohw = case.image_hw, case.out_hw
    assert (ohw[0] < ihw[0]).all() and (ohw[1] == ihw[1]).all() and (ohw[2] > ihw[2]).all() and ohw[0].tolist() == [492, 614]
    assert len({tuple(x) for x in ihw.tolist()}) == 3
    for d in (0, 1):                                   # image 2: the rounded scale carries the image edge past the output edge
        assert np.float32(np.float32(ohw[2, d] / ihw[2, d]) * np.float32(ihw[2, d])) > np.float32(ohw[2, d])
    for n, (cand, keep, _, det) in enumerate(C.want("scale_edges", 0)):
        assert {0, 1} <= set(det["rows"].tolist())
        b = {int(r): det["boxes"][i] for i, r in enumerate(det["rows"])}
        assert b[0][2] == ohw[n, 1] and b[1][3] == ohw[n, 0]                             # clipped to the edge, and on it after the rescale


@pytest.mark.parametrize("K", C.SWEEP_K)
def test_k_sweep_family(K):
    case = C.get(f"k_sweep_K{K}")
    assert case.K == K and case.head.shape == (2, 8, 5 * K + 2)
    assert all(det["count"] > 0 for _, _, _, det in C.want(f"k_sweep_K{K}", 0))
    assert {1, 80} <= set(C.SWEEP_K) and {1, 80} <= set(C.TIE_K)


# ------------------------------------------------------------------------------------------------ wrong rules
CAUGHT = {
    "scan_seams": {C.LOGITS_BY_OROW, C.PROBS_BY_FROW, C.VARS_IGNORE_FIX, C.VARS_BY_FROW, C.NO_CARRY, C.ROW_DROP_PER_CLASS},
    "dead_memory": {C.LOGITS_BY_OROW, C.PROBS_BY_FROW, C.VARS_IGNORE_FIX, C.VARS_BY_FROW, C.ROW_DROP_PER_CLASS},
    "quirk_indices": {C.LOGITS_BY_OROW, C.PROBS_BY_FROW, C.VARS_IGNORE_FIX, C.VARS_BY_FROW, C.ROW_DROP_PER_CLASS},
    "threshold_tie": {C.THRESH_GE, C.VARS_IGNORE_FIX, C.VARS_BY_FROW},
    "multi_class": {C.THRESH_GE, C.VARS_IGNORE_FIX, C.VARS_BY_FROW},
    "q3_overrange": {C.VARS_BY_FROW},
    "cap": {C.CAP_LAST, C.LOGITS_BY_OROW, C.PROBS_BY_FROW, C.VARS_IGNORE_FIX, C.VARS_BY_FROW, C.NO_CARRY, C.ROW_DROP_PER_CLASS},
    "empty_after_clip": {C.KEEP_EMPTY, C.NO_CARRY},
    "keep_seams": {C.KEEP_EMPTY, C.NO_CARRY},
    "decode_edges": {C.ROW_DROP_PER_CLASS, C.KEEP_EMPTY, C.LOGITS_BY_OROW, C.PROBS_BY_FROW, C.VARS_IGNORE_FIX, C.VARS_BY_FROW},
    "scale_edges": {C.CLIP_BEFORE_SCALE_ONLY, C.VARS_IGNORE_FIX, C.VARS_BY_FROW},
    "k_sweep": {C.LOGITS_BY_OROW, C.PROBS_BY_FROW, C.VARS_IGNORE_FIX, C.VARS_BY_FROW, C.ROW_DROP_PER_CLASS},
}


def differs(case, rule):
    """Some exactly compared field of some image changes under the rule, at some fix_vars setting the case runs under.  probs are
    compared with a tolerance, so PROBS_BY_FROW counts only where the two rows' probabilities are further apart than that."""
    for f in case.fix_vars:
        right, wrong = C.exact_view(case, f), C.exact_view(case, f, rule)
        if right != wrong:
            return True
        if rule == C.PROBS_BY_FROW:
            for (_, _, _, a), (_, _, _, b) in zip(C.run(case, f), C.run(case, f, rule)):
                if not np.allclose(a["probs"], b["probs"], rtol=1e-3, atol=1e-4):
                    return True
    return False


def test_every_family_tells_a_wrong_rule_from_the_right_one():
    """A condition, not a measurement: for every wrong rule some family's expected output differs from the right rule's in an
    exactly compared field (counts, classes, the three row ids, logits bits, the row a variance names, boxes where they are exact;
    for PROBS_BY_FROW, whose field has a tolerance, by 500 times that tolerance), and every family is told apart from at least
    one wrong rule.  The table (CAUGHT, asserted to be exactly this):

        family            caught
        scan_seams        LOGITS_BY_OROW PROBS_BY_FROW VARS_IGNORE_FIX VARS_BY_FROW NO_CARRY ROW_DROP_PER_CLASS
        dead_memory       LOGITS_BY_OROW PROBS_BY_FROW VARS_IGNORE_FIX VARS_BY_FROW ROW_DROP_PER_CLASS
        quirk_indices     LOGITS_BY_OROW PROBS_BY_FROW VARS_IGNORE_FIX VARS_BY_FROW ROW_DROP_PER_CLASS
        threshold_tie     THRESH_GE VARS_IGNORE_FIX VARS_BY_FROW
        multi_class       THRESH_GE VARS_IGNORE_FIX VARS_BY_FROW
        q3_overrange      VARS_BY_FROW
        cap               CAP_LAST LOGITS_BY_OROW PROBS_BY_FROW VARS_IGNORE_FIX VARS_BY_FROW NO_CARRY ROW_DROP_PER_CLASS
        empty_after_clip  KEEP_EMPTY NO_CARRY
        keep_seams        KEEP_EMPTY NO_CARRY
        decode_edges      ROW_DROP_PER_CLASS KEEP_EMPTY LOGITS_BY_OROW PROBS_BY_FROW VARS_IGNORE_FIX VARS_BY_FROW
        scale_edges       CLIP_BEFORE_SCALE_ONLY VARS_IGNORE_FIX VARS_BY_FROW
        k_sweep           LOGITS_BY_OROW PROBS_BY_FROW VARS_IGNORE_FIX VARS_BY_FROW ROW_DROP_PER_CLASS

    ROW_DROP_PER_CLASS shows wherever a NaN delta sits in a row that passes in another class; THRESH_GE only where a probability
    equals the threshold (0.5 in threshold_tie, 0.0 in multi_class); CLIP_BEFORE_SCALE_ONLY only where the rounded scale carries
    the image edge past the output edge (scale_edges, image 2).  In empty_after_clip and keep_seams every row is valid and passes
    in one class, so the three row ids coincide there: those families are about the rounds, not the ids."""
    table = {fam: {rule for rule in C.WRONG_RULES if any(differs(C.get(name), rule) for name in C.FAMILIES[fam])} for fam in C.FAMILIES}
    for fam, rules in table.items():
        assert rules, f"no wrong rule distinguishes family {fam}"
    for rule in C.WRONG_RULES:
        assert any(rule in rules for rules in table.values()), f"no family catches {rule}"
    assert table == CAUGHT, {f: sorted(r) for f, r in table.items() if r != CAUGHT[f]}


@pytest.mark.parametrize("name", C.names())
def test_every_case_is_told_apart_from_a_wrong_rule(name):
    """Not only every family: every single case."""
    case = C.get(name)
    assert any(differs(case, rule) for rule in C.WRONG_RULES), name


def test_fix_vars_key_reaches_the_detector_config():
    import proben_amd
    from proben_amd.predictor import detector_config_from_cfg
    cfg = proben_amd.get_cfg()
    assert detector_config_from_cfg(cfg).fix_vars is False
    cfg.PROBEN.FIX_VARS = True
    assert detector_config_from_cfg(cfg).fix_vars is True
    cfg.merge_from_list(["PROBEN.FIX_VARS", False])
    assert detector_config_from_cfg(cfg).fix_vars is False
