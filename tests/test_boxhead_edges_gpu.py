"""csrc/boxhead.hip against the restatement of tests/boxhead_cases.py where a random test does not look: the three row ids, the block
scan and the finalize ballot at their 64-lane seams, the candidate cap's content, drop-empty, a score exactly on the threshold,
the clamp at +-inf, fix_vars, K = 1 and K = 80, and memory that takes no part (tests/test_boxhead_edges_cpu.py shows on the CPU
that the restatement is the oracle and that every case tells a wrong rule from the right one).

Every case goes through pe_boxhead_candidates and pe_boxhead_finalize with every output pre-filled with a sentinel and GUARD spare
entries behind it.  Integers, logits and the row a variance names are compared exactly, boxes bit for bit where the case has exact
boxes; scores and probs within the project's tolerances against the float64 restatement AND bit for bit against the kernel's own
softmax output gathered through the restatement's indices (a gather changes no bit).  Nothing outside [:count] may be written."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import boxhead_cases as C

pytestmark = pytest.mark.gpu

TOL_SCORE = dict(rtol=2e-6, atol=1e-7)      # tests/test_ops_gpu.py::test_boxhead_matches_oracle_quirks
TOL_BOX = dict(rtol=1e-5, atol=2e-4)
TOL_VAR = dict(rtol=2e-6)
SENT = 0x5A5A5A5A

CASE_FIX = [(name, f) for name in C.names() for f in C.get(name).fix_vars]


@pytest.fixture(scope="module")
def lib():
    import proben_amd  # noqa: F401
    from proben_amd import _lib
    _lib.lib()
    return _lib


def cu(a):
    return torch.from_numpy(np.array(a)).cuda()


def sent(n):
    """n entries and GUARD more, all the sentinel (int32; the kernels see the pointer only)."""
    return torch.full((n + C.GUARD,), SENT, dtype=torch.int32, device="cuda")


def host(t, shape, dtype=np.int32):
    """(the [shape] part as dtype, the guard as int32)."""
    a = t.cpu().numpy()
    n = int(np.prod(shape))
    return a[:n].view(dtype).reshape(shape), a[n:]


def untouched(what, a):
    assert (np.asarray(a).view(np.int32) == SENT).all(), f"{what} was written"


def candidates_on_gpu(lib, case):
    N, P, stride = case.head.shape
    K, cmax = case.K, case.cand_max
    d = dict(head=cu(case.head.reshape(N * P, stride)), props=cu(case.props), pcnt=cu(case.pcnt), sz=cu(case.image_hw),
             osz=cu(case.out_hw), cb=sent(N * cmax * 4), cs=sent(N * cmax), cc=sent(N * cmax), cr=sent(N * cmax * 2), ccnt=sent(N),
             ctot=sent(N), probs=sent(N * P * (K + 1)))
    p = lib.ptr
    st = lib.lib().pe_boxhead_candidates(p(d["head"]), stride, N, P, K, p(d["pcnt"]), p(d["props"]), p(d["sz"]),
                                         (ctypes.c_float * 4)(*C.REG_W), C.SCALE_CLAMP, case.thr, cmax, p(d["cb"]), p(d["cs"]),
                                         p(d["cc"]), p(d["cr"]), p(d["ccnt"]), p(d["ctot"]), p(d["probs"]), lib.stream())
    lib.check(st, "pe_boxhead_candidates")
    return d


def check_candidates(name, case, d, want):
    """Counts, the list's content over [:count], nothing behind it, the softmax scratch of the live rows and nothing else."""
    N, P, _ = case.head.shape
    K, cmax = case.K, case.cand_max
    out = {}
    for key, shape, dt in [("cb", (N, cmax, 4), np.float32), ("cs", (N, cmax), np.float32), ("cc", (N, cmax), np.int32),
                           ("cr", (N, cmax, 2), np.int32), ("ccnt", (N,), np.int32), ("ctot", (N,), np.int32),
                           ("probs", (N, P, K + 1), np.float32)]:
        out[key], guard = host(d[key], shape, dt)
        untouched(f"{name}: the guard behind {key}", guard)
    for n, (cand, _, _, _) in enumerate(want):
        c = C.capped(cand)
        cnt, R = len(c["scores"]), C.live_rows(case, n)
        assert (int(out["ctot"][n]), int(out["ccnt"][n])) == (cand["total"], cnt), (name, n, out["ctot"][n], out["ccnt"][n], cand["total"], cnt)
        np.testing.assert_array_equal(out["cc"][n, :cnt], c["classes"], err_msg=f"{name} image {n}: candidate classes")
        np.testing.assert_array_equal(out["cr"][n, :cnt, 0], c["frow"], err_msg=f"{name} image {n}: candidate frow")
        np.testing.assert_array_equal(out["cr"][n, :cnt, 1], c["orow"], err_msg=f"{name} image {n}: candidate orow")
        if case.exact_boxes:
            np.testing.assert_array_equal(out["cb"][n, :cnt], c["boxes"].astype(np.float32), err_msg=f"{name} image {n}: candidate boxes")
        else:
            np.testing.assert_allclose(out["cb"][n, :cnt], c["boxes"], err_msg=f"{name} image {n}: candidate boxes", **TOL_BOX)
        np.testing.assert_allclose(out["cs"][n, :cnt], c["scores"], err_msg=f"{name} image {n}: candidate scores", **TOL_SCORE)
        np.testing.assert_array_equal(out["cs"][n, :cnt], out["probs"][n, c["orow"], c["classes"]])
        for key in ("cb", "cs", "cc", "cr"):
            untouched(f"{name} image {n}: {key} past the count", out[key][n, cnt:])
        np.testing.assert_allclose(out["probs"][n, :R], cand["probs"], err_msg=f"{name} image {n}: softmax", **TOL_SCORE)
        ties = np.isin(cand["probs"], case.claims.get("tie_values", ()))
        np.testing.assert_array_equal(out["probs"][n, :R][ties], cand["probs"][ties].astype(np.float32))     # 0.5 and 0 are exact
        untouched(f"{name} image {n}: softmax rows past prop_counts", out["probs"][n, R:])
    return out


def finalize_on_gpu(lib, case, d, keep, kcnt, fix_vars):
    """keep: int32 device tensor of N * max_det entries (+ guard), kcnt [N]."""
    N, P, stride = case.head.shape
    K, D_ = case.K, case.max_det
    o = dict(boxes=sent(N * D_ * 4), scores=sent(N * D_), classes=sent(N * D_), logits=sent(N * D_ * (K + 1)), probs=sent(N * D_ * K),
             vars=sent(N * D_), rows=sent(N * D_), counts=sent(N))
    p = lib.ptr
    st = lib.lib().pe_boxhead_finalize(p(d["head"]), stride, N, P, K, case.cand_max, D_, int(fix_vars), p(d["probs"]), p(d["cb"]),
                                       p(d["cs"]), p(d["cc"]), p(d["cr"]), p(keep), p(kcnt), p(d["sz"]), p(d["osz"]), p(o["boxes"]),
                                       p(o["scores"]), p(o["classes"]), p(o["logits"]), p(o["probs"]), p(o["vars"]), p(o["rows"]),
                                       p(o["counts"]), lib.stream())
    lib.check(st, "pe_boxhead_finalize")
    return o


def check_detections(name, case, got, want, cand_out, shapes=None):
    """got: name -> numpy [N, D, ...] (counts [N]); every field over [:count] of EVERY image."""
    K = case.K
    for n, (cand, keep, _, det) in enumerate(want):
        m = det["count"]
        where = f"{name} image {n}"
        assert int(got["counts"][n]) == m, (where, int(got["counts"][n]), m)
        np.testing.assert_array_equal(got["classes"][n, :m], det["classes"], err_msg=f"{where}: classes")
        np.testing.assert_array_equal(got["rows"][n, :m], det["rows"], err_msg=f"{where}: det_rows (original rows)")
        np.testing.assert_array_equal(got["logits"][n, :m], det["logits"], err_msg=f"{where}: logits (Q4: through frow)")
        np.testing.assert_array_equal(C.var_row(case, got["vars"][n, :m]), det["vrow"], err_msg=f"{where}: the row the variance names")
        np.testing.assert_allclose(got["vars"][n, :m], det["vars"], err_msg=f"{where}: vars", **TOL_VAR)
        np.testing.assert_allclose(got["scores"][n, :m], det["scores"], err_msg=f"{where}: scores", **TOL_SCORE)
        np.testing.assert_allclose(got["probs"][n, :m], det["probs"], err_msg=f"{where}: probs", **TOL_SCORE)
        if cand_out is not None:
            np.testing.assert_array_equal(got["scores"][n, :m], cand_out["cs"][n, det["cid"]], err_msg=f"{where}: score bits")
            np.testing.assert_array_equal(got["probs"][n, :m], cand_out["probs"][n, det["rows"], :K], err_msg=f"{where}: prob bits (through orow)")
        if case.exact_boxes:
            np.testing.assert_array_equal(got["boxes"][n, :m], det["boxes"].astype(np.float32), err_msg=f"{where}: boxes")
        else:
            np.testing.assert_allclose(got["boxes"][n, :m], det["boxes"], err_msg=f"{where}: boxes", **TOL_BOX)


@pytest.mark.parametrize("name,fix_vars", CASE_FIX)
def test_boxhead_kernels_match_the_restatement(lib, name, fix_vars):
    from proben_amd import layers as L
    case = C.get(name)
    want = C.want(name, fix_vars)
    N, P, _ = case.head.shape
    K, cmax, D_ = case.K, case.cand_max, case.max_det
    d = candidates_on_gpu(lib, case)
    cand_out = check_candidates(name, case, d, want)
    keep_want = np.zeros((N, D_), dtype=np.int32)              # unused entries and the guard: candidate id 0, a row that exists
    for n, (_, keep, _, _) in enumerate(want):
        keep_want[n, :len(keep)] = keep
    kc_want = np.asarray([kc for _, _, kc, _ in want], dtype=np.int32)
    keep = torch.zeros(N * D_ + C.GUARD, dtype=torch.int32, device="cuda")
    if case.keep_mode == "nms":
        view = lambda t, *shape: t[:int(np.prod(shape))].view(*shape)  # noqa: E731
        k, kcnt = L.nms_batched_raw(view(d["cb"], N, cmax, 4).view(torch.float32), view(d["cs"], N, cmax).view(torch.float32),
                                    view(d["cc"], N, cmax), d["ccnt"][:N], None, 0.5, 0, D_)
        np.testing.assert_array_equal(kcnt.cpu().numpy(), kc_want)
        for n in range(N):
            np.testing.assert_array_equal(k[n, :kc_want[n]].cpu().numpy(), keep_want[n, :kc_want[n]], err_msg=f"{name} image {n}: NMS keep")
        keep[:N * D_] = k.reshape(-1)
    else:
        keep[:N * D_] = cu(keep_want.reshape(-1))
        kcnt = cu(kc_want)
    o = finalize_on_gpu(lib, case, d, keep, kcnt, fix_vars)
    got = {}
    for key, shape, dt in [("boxes", (N, D_, 4), np.float32), ("scores", (N, D_), np.float32), ("classes", (N, D_), np.int32),
                           ("logits", (N, D_, K + 1), np.float32), ("probs", (N, D_, K), np.float32), ("vars", (N, D_), np.float32),
                           ("rows", (N, D_), np.int32), ("counts", (N,), np.int32)]:
        got[key], guard = host(o[key], shape, dt)
        untouched(f"{name}: the guard behind det {key}", guard)
    check_detections(name, case, got, want, cand_out)
    for n, (_, _, _, det) in enumerate(want):
        for key in ("boxes", "scores", "classes", "logits", "probs", "vars", "rows"):
            untouched(f"{name} image {n}: det {key} past the count", got[key][n, det["count"]:])
    # finalize reads its inputs only
    again = check_candidates(name, case, d, want)
    for key in cand_out:
        np.testing.assert_array_equal(again[key].view(np.int32), cand_out[key].view(np.int32))


def test_fix_vars_through_the_model(lib):
    """GeneralizedRCNN._roi_heads(head=...) on the quirk_indices inputs with DetectorConfig(fix_vars=False) and (fix_vars=True): each
    matches the restatement in every field, and the two differ in vars (and in nothing else)."""
    from proben_amd.rcnn import DetectorConfig, GeneralizedRCNN
    from proben_amd.synthetic import synthetic_state_dict
    case = C.get("quirk_indices")
    N, P, stride = case.head.shape
    K = case.K
    cfgs = {f: DetectorConfig(num_classes=K, score_thresh=case.thr, nms_thresh=0.5, post_nms_topk=P, detections_per_image=case.max_det,
                              fix_vars=bool(f)) for f in (0, 1)}
    model = GeneralizedRCNN(cfgs[0], synthetic_state_dict(50, K, 3, seed=4))
    head = np.zeros((N * P, model.w.head_stride), np.float32)
    head[:, :stride] = case.head.reshape(N * P, stride)
    results = {}
    for f in (0, 1):
        model.cfg = cfgs[f]
        assert dataclasses.asdict(model.cfg)["fix_vars"] is bool(f)
        det = model._roi_heads(None, cu(case.props), cu(case.pcnt), cu(case.image_hw), cu(case.out_hw), N, head=cu(head))
        got = {k: det[m].cpu().numpy() for k, m in [("boxes", "boxes"), ("scores", "scores"), ("classes", "classes"), ("logits", "class_logits"),
                                                   ("probs", "prob_score"), ("vars", "vars"), ("rows", "rows"), ("counts", "counts")]}
        np.testing.assert_array_equal(det["cand_total"].cpu().numpy(), [cand["total"] for cand, _, _, _ in C.want("quirk_indices", f)])
        check_detections(f"model fix_vars={f}", case, got, C.want("quirk_indices", f), None)
        results[f] = got
    np.testing.assert_array_equal(results[0]["counts"], results[1]["counts"])
    for n, m in enumerate(results[0]["counts"]):
        for key in ("boxes", "scores", "classes", "logits", "probs", "rows"):
            np.testing.assert_array_equal(results[0][key][n, :m], results[1][key][n, :m])
        assert (results[0]["vars"][n, :m] != results[1]["vars"][n, :m]).mean() > 0.5


def test_argument_contract(lib):
    """K = 81, per_image = 1025, per_image = 0 and head_stride = 5K + 1 are refused with a message and touch no output; N = 0 is
    fine and touches none either."""
    case = C.get("k_sweep_K3")
    N, P, stride = case.head.shape
    K, cmax = 3, case.cand_max
    p = lib.ptr
    hd, pr, pc, sz = cu(case.head.reshape(N * P, stride)), cu(case.props), cu(case.pcnt), cu(case.image_hw)

    def call(n=N, per_image=P, k=K, st=stride):
        o = [sent(N * cmax * 4), sent(N * cmax), sent(N * cmax), sent(N * cmax * 2), sent(N), sent(N), sent(N * P * (K + 1))]
        status = lib.lib().pe_boxhead_candidates(p(hd), st, n, per_image, k, p(pc), p(pr), p(sz), (ctypes.c_float * 4)(*C.REG_W),
                                                 C.SCALE_CLAMP, 0.5, cmax, *[p(t) for t in o], lib.stream())
        torch.cuda.synchronize()
        return status, lib.lib().pe_last_error().decode(), o

    for kw, words in [(dict(k=81), "num_classes 81"), (dict(per_image=1025), "per_image 1025"), (dict(per_image=0), "per_image 0"),
                      (dict(st=5 * K + 1), f"head_stride {5 * K + 1} < {5 * K + 2}")]:
        status, msg, o = call(**kw)
        assert status != 0 and "pe_boxhead_candidates" in msg and words in msg, (kw, status, msg)
        for t in o:
            untouched(f"{kw}: an output of a refused call", t.cpu().numpy())
    status, _, o = call(n=0)
    assert status == 0
    for t in o:
        untouched("N = 0: an output", t.cpu().numpy())
    status, _, o = call()
    assert status == 0 and (o[4].cpu().numpy()[:N] != SENT).all()                 # the same call with nothing wrong does write
    # finalize with N = 0
    D_ = case.max_det
    outs = [sent(N * D_ * 4), sent(N * D_), sent(N * D_), sent(N * D_ * (K + 1)), sent(N * D_ * K), sent(N * D_), sent(N * D_), sent(N)]
    keep, kcnt = torch.zeros(N * D_, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    status = lib.lib().pe_boxhead_finalize(p(hd), stride, 0, P, K, cmax, D_, 0, p(o[6]), p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(keep),
                                           p(kcnt), p(sz), p(sz), *[p(t) for t in outs], lib.stream())
    torch.cuda.synchronize()
    assert status == 0
    for t in outs:
        untouched("finalize with N = 0: an output", t.cpu().numpy())
