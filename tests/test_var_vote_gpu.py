"""csrc/varvote.hip (pe_boxhead_var_vote) against the float64 restatement of tests/var_vote_ref.py, through the C-ABI and through the model.

Tolerance.  Every kept coordinate must be the restatement's float32 or one of its two neighbours (np.spacing).  The kernel adds
non-negative float64 terms (boxes are clipped to >= 0), so its sums carry a relative error of order n * 2^-53, as does the kernel's
p * (1 / var) against the restatement's p / var and the device's float64 exp against libm's: all far below half a float32 ulp, so only
a value that sits on a rounding boundary can land on the neighbour.  The one float32 quantity of the rule is var = exp(log-variance),
"computed in float32 as finalize does": two float32 exp routines may differ in the last bit, and a last-bit change of a weight moves a
voted coordinate by up to an ulp of its own.  So the restatement is handed the float32 variances boxhead_finalize_kernel itself reports
for the same rows (device_variances: pe_boxhead_finalize with fix_vars = 1 over every row), and those are in turn held to NumPy's
float32 exp within the tolerance the box-head tests put on a reported variance (rtol 2e-6; the device's expf and NumPy's differ by
more than one ulp at log-variances near -9).  Everything that is not a kept coordinate is compared bit for bit."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import boxhead_cases as C
import var_vote_ref as V

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = 0x5A5A5A5A
GUARD = C.GUARD
S = 0.025
HW = (512, 640)
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "proben_hip.h")) as _f:
    TILE = int(re.search(r"#define\s+PE_VAR_VOTE_TILE\s+(\d+)", _f.read()).group(1))      # candidates per LDS tile of the kernel


@pytest.fixture(scope="module")
def lib():
    import proben_amd  # noqa: F401
    from proben_amd import _lib
    _lib.lib()
    return _lib


def cu(a):
    return torch.from_numpy(np.array(a)).cuda()          # a copy: the cases' arrays are read-only


def guarded(a):
    """The array's bits as int32 on the device with GUARD sentinel entries behind them."""
    flat = np.ascontiguousarray(a).reshape(-1).view(np.int32)
    return cu(np.concatenate([flat, np.full(GUARD, SENT, dtype=np.int32)]))


def device_variances(lib, head, K):
    """exp(head[r, 5K+1]) for every row r of head [R, stride], as boxhead_finalize_kernel computes it: one pe_boxhead_finalize call with
    fix_vars = 1 in which candidate r is row r, every candidate is kept and every box is [0, 0, 1, 1] on a 1 x 1 image."""
    R, stride = head.shape
    p = lib.ptr
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")        # noqa: E731
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")      # noqa: E731
    rows = torch.arange(R, dtype=torch.int32, device="cuda")
    cb = cu(np.tile(np.array([0, 0, 1, 1], dtype=F32), (R, 1)))
    hw, kcnt, hd = cu(np.array([[1, 1]], dtype=np.int32)), cu(np.array([R], dtype=np.int32)), cu(head)
    probs, cs, cc, cr = f32(R, K + 1), f32(R), i32(R), torch.stack([rows, rows], 1).contiguous()
    out = dict(boxes=f32(R, 4), scores=f32(R), classes=i32(R), logits=f32(R, K + 1), probs=f32(R, K), vars=f32(R), rows=i32(R), counts=i32(1))
    st = lib.lib().pe_boxhead_finalize(p(hd), stride, 1, R, K, R, R, 1, p(probs), p(cb), p(cs), p(cc), p(cr), p(rows), p(kcnt), p(hw), p(hw),
                                       p(out["boxes"]), p(out["scores"]), p(out["classes"]), p(out["logits"]), p(out["probs"]), p(out["vars"]),
                                       p(out["rows"]), p(out["counts"]), lib.stream())
    lib.check(st, "pe_boxhead_finalize")
    torch.cuda.synchronize()
    assert int(out["counts"].cpu()) == R and (out["rows"].cpu().numpy() == np.arange(R)).all()
    got = out["vars"].cpu().numpy()
    with np.errstate(all="ignore"):
        ref = np.exp(head[:, 5 * K + 1].astype(F32))
    fin = np.isfinite(ref) & (ref > 0)
    np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-6)          # the project's tolerance on a reported variance (TOL_VAR)
    assert (V.bits(got[~fin & ~np.isnan(ref)]) == V.bits(ref[~fin & ~np.isnan(ref)])).all()      # exp(-inf) = 0, exp(inf) = inf
    assert np.isnan(got[np.isnan(ref)]).all()
    return got


class Problem:
    """N images of candidate lists built by hand: head [N, P, stride], boxes / classes / rows [N, cmax, ...], counts, keep [N, D], kcnt."""

    def __init__(self, images, K, max_det, P=64, pad=0, stride_pad=0):
        self.N, self.K, self.D, self.P = len(images), K, max_det, P
        self.stride = 5 * K + 2 + stride_pad
        self.cmax = max(1, max(len(im["boxes"]) for im in images) + pad)
        N, cmax = self.N, self.cmax
        self.head = np.full((N, P, self.stride), np.nan, dtype=F32)          # the vote reads column 5K+1 only: NaN everywhere else
        self.boxes = np.full((N, cmax, 4), np.nan, dtype=F32)                # rows past the count: NaN boxes, class and rows out of range
        self.classes = np.full((N, cmax), -7, dtype=np.int32)
        self.rows = np.full((N, cmax, 2), 1 << 30, dtype=np.int32)
        self.counts = np.zeros(N, dtype=np.int32)
        self.keep = np.full((N, max_det), -1, dtype=np.int32)
        self.kcnt = np.zeros(N, dtype=np.int32)
        for n, im in enumerate(images):
            c = len(im["boxes"])
            self.head[n, :, 5 * K + 1] = im["logvar"]
            self.boxes[n, :c], self.classes[n, :c] = im["boxes"], im["classes"]
            self.rows[n, :c, 0], self.rows[n, :c, 1] = im["orow"] // 2, im["orow"]     # the filtered row id takes no part
            self.counts[n] = c
            k = np.asarray(im["keep"], dtype=np.int32)[:max_det]
            self.keep[n, :len(k)] = k
            self.kcnt[n] = im.get("kcnt", len(im["keep"]))

    def image(self, n):
        c = int(self.counts[n])
        return dict(boxes=self.boxes[n, :c], classes=self.classes[n, :c], orow=self.rows[n, :c, 1], logvar=self.head[n, :, 5 * self.K + 1],
                    keep=self.keep[n, :min(int(self.kcnt[n]), self.D)], kcnt=int(self.kcnt[n]))


def draw_image(key, count, kc, K, P=64, bad_fraction=0.05, kcnt=None):
    rng = np.random.default_rng(C.seed_of("var_vote", key))
    boxes, classes, _ = V.random_pile(rng, count, K, image_hw=HW) if count else (np.zeros((0, 4), F32), np.zeros(0, np.int32), None)
    logvar = rng.uniform(-9.0, -2.0, P).astype(F32)
    bad = np.nonzero(rng.random(P) < bad_fraction)[0]
    logvar[bad] = np.array([-np.inf, np.inf, np.nan], dtype=F32)[np.arange(len(bad)) % 3]
    keep = rng.permutation(count)[:kc] if count else np.zeros(0, np.int64)
    im = dict(boxes=boxes, classes=classes, orow=rng.integers(0, P, count).astype(np.int32), logvar=logvar, keep=keep)
    if kcnt is not None:
        im["kcnt"] = kcnt
    return im


def run(lib, pb, sigma_t=S):
    """-> (out [N, cmax, 4] float32 as int32 bits; SENT wherever the kernel wrote nothing).  Checks the guards and that the inputs are unchanged."""
    p = lib.ptr
    ins = dict(head=pb.head, boxes=pb.boxes, classes=pb.classes, rows=pb.rows, counts=pb.counts, keep=pb.keep, kcnt=pb.kcnt)
    dev = {k: guarded(a) for k, a in ins.items()}
    out = torch.full((pb.N * pb.cmax * 4 + GUARD,), SENT, dtype=torch.int32, device="cuda")
    st = lib.lib().pe_boxhead_var_vote(p(dev["head"]), pb.stride, pb.N, pb.P, pb.K, pb.cmax, pb.D, p(dev["boxes"]), p(dev["classes"]),
                                       p(dev["rows"]), p(dev["counts"]), p(dev["keep"]), p(dev["kcnt"]), sigma_t, p(out), lib.stream())
    lib.check(st, "pe_boxhead_var_vote")
    o = out.cpu().numpy()
    assert (o[pb.N * pb.cmax * 4:] == SENT).all(), "the guard behind out_boxes was written"
    for k, a in ins.items():
        back = dev[k].cpu().numpy()
        assert (back[:a.size] == a.reshape(-1).view(np.int32)).all() and (back[a.size:] == SENT).all(), f"input {k} was written"
    return o[:pb.N * pb.cmax * 4].reshape(pb.N, pb.cmax, 4)


def want_of(lib, pb, sigma_t=S):
    var = device_variances(lib, pb.head.reshape(pb.N * pb.P, pb.stride), pb.K).reshape(pb.N, pb.P)
    out = []
    for n in range(pb.N):
        im = pb.image(n)
        out.append(V.vote(im["boxes"], im["classes"], var[n][im["orow"]], im["keep"], sigma_t))
    return out


def check(name, pb, got, want):
    moved = 0
    for n in range(pb.N):
        im = pb.image(n)
        c = len(im["boxes"])
        kept = np.zeros(c, dtype=bool)
        kept[[b for b in im["keep"].tolist() if 0 <= b < c]] = True
        g = got[n, :c].view(F32)
        np.testing.assert_array_equal(got[n, :c][~kept], V.bits(im["boxes"][~kept]), err_msg=f"{name} image {n}: a box that is not kept")
        assert V.within_one_ulp(g[kept], want[n][kept]), (name, n, np.abs(g[kept].astype(np.float64) - want[n][kept]).max())
        assert (got[n, c:] == SENT).all(), f"{name} image {n}: rows past cand_counts were written"
        moved += int((V.bits(want[n][kept]) != V.bits(im["boxes"][kept])).any(1).sum())
    return moved


# (candidate count, kept count, K): the 64-lane seams, the 16-wave round seam (kept 16 / 17), the LDS tile's seams, kept = max_det
def shapes(T=TILE):
    return {"c1_k1_K1": (1, 1, 1), "c63_k0": (63, 0, 3), "c64_k1": (64, 1, 3), "c65_k63_K80": (65, 63, 80), "c200_k64": (200, 64, 3),
            "c200_k65": (200, 65, 3), "c300_kD": (300, 100, 3), f"c{T - 1}_k16": (T - 1, 16, 3), f"c{T}_k17_K1": (T, 17, 1),
            f"c{T + 1}_k33": (T + 1, 33, 3)}


@functools.lru_cache(maxsize=None)
def shape_problem(name):
    count, kc, K = shapes()[name]
    # kept = max_det: keep_counts says 5 more than the keep array holds, as pe_nms_batched may report
    return Problem([draw_image(name, count, kc, K, kcnt=kc + 5 if kc == 100 else None)], K, 100, pad=3 if count % 2 else 0, stride_pad=count % 3)


@pytest.mark.parametrize("name", list(shapes()))
def test_vote_matches_the_restatement(lib, name):
    pb = shape_problem(name)
    got = run(lib, pb)
    moved = check(name, pb, got, want_of(lib, pb))
    assert moved > 0 or pb.kcnt[0] == 0 or pb.counts[0] == 1, "no kept box had a voter but itself: the case tests nothing"
    np.testing.assert_array_equal(run(lib, pb), got, err_msg=f"{name}: two runs differ")


@functools.lru_cache(maxsize=None)
def batch_problem():
    ims = [draw_image("batch0", 130, 20, 3), draw_image("batch1", 0, 0, 3), draw_image("batch2", TILE + 1, 40, 3)]
    ims[0]["keep"] = np.concatenate([ims[0]["keep"][:10], [130, -1, 1 << 20], ims[0]["keep"][10:]])      # ids outside the list are skipped
    return ims, Problem(ims, 3, 100)


def test_batch_of_three_and_each_image_alone(lib):
    """N = 3 with one empty image and unequal counts against the restatement; then each image alone (its own cand_max, N = 1): bit-identical."""
    ims, pb = batch_problem()
    got = run(lib, pb)
    check("batch", pb, got, want_of(lib, pb))
    for n, im in enumerate(ims):
        alone = Problem([im], 3, 100)
        c = len(im["boxes"])
        np.testing.assert_array_equal(run(lib, alone)[0, :c], got[n, :c], err_msg=f"image {n} alone differs from image {n} in the batch")


def edge_problem():
    """The CPU file's edge cases as one image: kept 0 with neighbours that must not vote (other class, IoU 0, no area, variance 0 / inf /
    NaN); kept 7 with a bad variance of its own beside a good neighbour; kept 9 without area; kept 11 with an exact duplicate (12) and a
    good neighbour (13).  Rows: 0 good (0.01-ish), 1 -> var 0, 2 -> inf, 3 -> NaN."""
    k = [10, 10, 30, 30]
    boxes = np.array([k, k, [30, 10, 50, 30], [15, 15, 15, 25], [12, 10, 32, 30], [12, 10, 32, 30], [12, 10, 32, 30],
                      [100, 100, 140, 140], [104, 100, 144, 140], [200, 200, 200, 240], [198, 200, 230, 240],
                      [300, 300, 340, 360], [300, 300, 340, 360], [306, 300, 346, 360]], dtype=F32)
    classes = np.array([1, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 0, 0, 0], dtype=np.int32)
    orow = np.array([0, 0, 0, 0, 1, 2, 3, 3, 0, 0, 0, 0, 4, 5], dtype=np.int32)
    logvar = np.full(64, -4.5, dtype=F32)
    logvar[1:6] = [-np.inf, np.inf, np.nan, -6.0, -3.0]
    return dict(boxes=boxes, classes=classes, orow=orow, logvar=logvar, keep=np.array([0, 7, 9, 11]))


def test_edge_cases_on_the_device(lib):
    im = edge_problem()
    pb = Problem([im], 3, 8)
    got = run(lib, pb)
    want = want_of(lib, pb)
    check("edges", pb, got, want)
    for b in (0, 7, 9):
        np.testing.assert_array_equal(got[0, b], V.bits(im["boxes"][b]), err_msg=f"kept box {b} must keep its bits")
    assert got[0, 11].view(F32)[0] > 300 and got[0, 11].view(F32)[1] == 300            # the neighbour pulls x, not y
    # sigma_t -> 0: only b and its exact duplicate remain, and the result is the NMS box bit for bit
    tiny = run(lib, pb, 1e-30)
    np.testing.assert_array_equal(tiny[0, :len(im["boxes"])], V.bits(im["boxes"]))


def test_sigma_to_zero_gives_the_input_bits_on_a_pile(lib):
    pb = shape_problem("c200_k65")
    got = run(lib, pb, 1e-30)
    np.testing.assert_array_equal(got[0, :200], V.bits(pb.boxes[0, :200]))


# ------------------------------------------------------------------------------------------------ through the model
FIELDS = [("boxes", "boxes"), ("scores", "scores"), ("classes", "classes"), ("logits", "class_logits"), ("probs", "prob_score"),
          ("vars", "vars"), ("rows", "rows"), ("counts", "counts")]
MODEL_CASE = "quirk_indices"          # P = 64 proposals per image scattered over a 256 x 320 image: 43 of its 111 kept boxes have voters
WIDE = 1.0                            # a second sigma_t: NMS at 0.5 leaves neighbours of IoU < 0.5, p < exp(-10) at 0.025 - most moves are below an ulp


@pytest.fixture(scope="module")
def model_runs(lib):
    """_roi_heads(head=...) under var_voting off / on at sigma_t S / on at sigma_t WIDE (keys False, S, WIDE) x fix_vars False / True, the bits of every field; and the unvoted chain by hand
    through the C-ABI (candidates -> NMS -> finalize), as _roi_heads ran it before the vote existed."""
    from proben_amd import layers as L
    from proben_amd.rcnn import DetectorConfig, GeneralizedRCNN
    from proben_amd.synthetic import synthetic_state_dict
    case = C.get(MODEL_CASE)
    N, P, stride = case.head.shape
    K, D = case.K, case.max_det
    base = dict(num_classes=K, score_thresh=case.thr, nms_thresh=0.5, post_nms_topk=P, detections_per_image=D)
    model = GeneralizedRCNN(DetectorConfig(**base), synthetic_state_dict(50, K, 3, seed=4))
    hs = model.w.head_stride
    head = np.zeros((N * P, hs), np.float32)
    head[:, :stride] = case.head.reshape(N * P, stride)
    ins = [cu(case.props), cu(case.pcnt), cu(case.image_hw), cu(case.out_hw)]
    runs = {}
    for key, vote, sigma_t in ((False, False, S), (S, True, S), (WIDE, True, WIDE)):
        for f in (False, True):
            model.cfg = DetectorConfig(var_voting=vote, var_voting_sigma_t=sigma_t, fix_vars=f, **base)
            det = model._roi_heads(None, *ins, N, head=cu(head))
            runs[key, f] = {k: det[m].cpu().numpy() for k, m in FIELDS}
    # by hand
    cmax = P                                                                    # score_thresh 0.5: one class per proposal at most
    p = lib.ptr
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")    # noqa: E731
    cb, cs, cc, cr, ccnt, ctot, probs = f32(N, cmax, 4), f32(N, cmax), i32(N, cmax), i32(N, cmax, 2), i32(N), i32(N), f32(N, P, K + 1)
    hd = cu(head)
    lib.check(lib.lib().pe_boxhead_candidates(p(hd), hs, N, P, K, p(ins[1]), p(ins[0]), p(ins[2]), (ctypes.c_float * 4)(*C.REG_W),
                                              C.SCALE_CLAMP, case.thr, cmax, p(cb), p(cs), p(cc), p(cr), p(ccnt), p(ctot), p(probs),
                                              lib.stream()), "pe_boxhead_candidates")
    keep, kcnt = L.nms_batched_raw(cb, cs, cc, ccnt, None, 0.5, 0, D)
    for f in (False, True):
        o = dict(boxes=f32(N, D, 4), scores=f32(N, D), classes=i32(N, D), logits=f32(N, D, K + 1), probs=f32(N, D, K), vars=f32(N, D),
                 rows=i32(N, D), counts=i32(N))
        lib.check(lib.lib().pe_boxhead_finalize(p(hd), hs, N, P, K, cmax, D, int(f), p(probs), p(cb), p(cs), p(cc), p(cr), p(keep), p(kcnt),
                                                p(ins[2]), p(ins[3]), p(o["boxes"]), p(o["scores"]), p(o["classes"]), p(o["logits"]),
                                                p(o["probs"]), p(o["vars"]), p(o["rows"]), p(o["counts"]), lib.stream()), "pe_boxhead_finalize")
        runs["hand", f] = {k: v.cpu().numpy() for k, v in o.items()}
    runs["variances"] = device_variances(lib, head[:, :stride].copy(), K).reshape(N, P)
    return case, runs


def live(run_):
    """Every field over [:count] of every image, as bits."""
    return [{k: np.ascontiguousarray(v[n, :m]).view(np.int32) for k, v in run_.items() if k != "counts"} for n, m in enumerate(run_["counts"])]


@pytest.mark.parametrize("fix_vars", [False, True])
def test_var_voting_off_is_the_unvoted_chain_bit_for_bit(model_runs, fix_vars):
    case, runs = model_runs
    np.testing.assert_array_equal(runs[False, fix_vars]["counts"], runs["hand", fix_vars]["counts"])
    for n, (a, b) in enumerate(zip(live(runs[False, fix_vars]), live(runs["hand", fix_vars]))):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"image {n}: {k}")


# At the default sigma_t the case's neighbours (IoU < 0.5 after NMS) weigh p < exp(-10): two kept boxes move by more than an ulp, so that
# row checks the default's plumbing and that the rest stays put; the WIDE row is the one that would notice a vote that does nothing.
@pytest.mark.parametrize("sigma_t,least_moved", [(S, 1), (WIDE, 20)])
@pytest.mark.parametrize("fix_vars", [False, True])
def test_var_voting_through_the_model(model_runs, fix_vars, sigma_t, least_moved):
    """Boxes against the restatement chain C.candidates -> C.keep_of -> vote -> C.finalize on the voted boxes; every other field, vars
    included, is the unvoted run's bit for bit.  At the default sigma_t and at a wide one, where most kept boxes with a neighbour move."""
    case, runs = model_runs
    got, plain = runs[sigma_t, fix_vars], runs[False, fix_vars]
    np.testing.assert_array_equal(got["counts"], plain["counts"])
    for n, (a, b) in enumerate(zip(live(got), live(plain))):
        for k in a:
            if k != "boxes":
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"image {n}: {k} changed under voting")
    moved = 0
    for n in range(len(case.pcnt)):
        cand = C.candidates(case, n)
        assert cand["total"] <= case.cand_max
        keep, _ = C.keep_of(case, n, cand)
        c = C.capped(cand)
        voted = V.vote(c["boxes"].astype(F32), c["classes"], runs["variances"][n][c["orow"]], keep, sigma_t)
        det = C.finalize(case, n, dict(cand, boxes=voted.astype(np.float64)), keep, int(fix_vars))
        m = det["count"]
        assert m == int(got["counts"][n])
        np.testing.assert_array_equal(got["rows"][n, :m], det["rows"])
        assert V.within_one_ulp(got["boxes"][n, :m], det["boxes"].astype(F32)), (n, np.abs(got["boxes"][n, :m] - det["boxes"]).max())
        moved += int((got["boxes"][n, :m] != plain["boxes"][n, :m]).any(1).sum())
    assert moved >= least_moved, f"voting moved {moved} boxes of the case"
