"""csrc/nms.hip index for index against oracle/nms.py where a random test does not look: IoU exactly at the threshold, degenerate
boxes, non-finite scores and coordinates, rows that take no part, and the sizes at which the kernels switch paths (tests/nms_cases.py
has the builders; tests/test_nms_edges_cpu.py shows on the CPU that every case tells a wrong rule from the right one).

Every case goes through layers.nms_batched_raw - with the presorted shortcut of the sort kernel on and off wherever the padded
size reaches 1024 - and, where it is one full image, through layers.batched_nms and (one class) layers.nms.  No tolerance
anywhere: keep lists and counts must be the oracle's."""
import numpy as np
import pytest
import torch

import nms_cases as C
from oracle import nms as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import proben_amd  # noqa: F401
    from proben_amd import layers
    return layers


@pytest.fixture(scope="module")
def hooks():
    from proben_amd import _lib
    return _lib.test_hooks()


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def same_lists(what, case, keep, cnt, want):
    """keep [B, max_out], cnt [B] against the oracle's lists; the message names the first output index that differs."""
    keep, cnt = np.asarray(keep), np.asarray(cnt)
    for b, w in enumerate(want):
        got = keep[b, : max(0, min(int(cnt[b]), keep.shape[1]))]
        m = min(len(got), len(w))
        diff = np.nonzero(got[:m] != w[:m])[0]
        if len(diff):
            i = int(diff[0])
            def row(r):
                if not 0 <= r < case.scores.shape[1]:
                    return f"row {r} (no row of the input)"
                return f"row {r} (score bits {int(C.f32_bits(case.scores[b])[r]):#010x}, box {case.boxes[b][r].tolist()})"
            raise AssertionError(f"{what}, image {b}: first difference at output index {i}: got {row(int(got[i]))}, "
                                 f"want {row(int(w[i]))}; counts got {int(cnt[b])}, want {len(w)}")
        assert int(cnt[b]) == len(w), f"{what}, image {b}: the first {m} rows agree; counts got {int(cnt[b])}, want {len(w)}"


def run_raw(L, case):
    keep, cnt = L.nms_batched_raw(cu(case.boxes), cu(case.scores), cu(case.idxs), cu(case.counts), cu(case.valid), case.thr,
                                  case.mode, case.max_out)
    return keep.cpu().numpy(), cnt.cpu().numpy()


def hook_settings(case):
    return (1, 0) if C.n_pad_of(case.scores.shape[1]) >= 1024 else (1,)


def raw_both_settings(L, hooks, name, case, want):
    try:
        for on in hook_settings(case):
            hooks.pe_test_set_nms_presorted(on)
            keep, cnt = run_raw(L, case)
            same_lists(f"{name}: nms_batched_raw (presorted shortcut {'on' if on else 'off'})", case, keep, cnt, want)
    finally:
        hooks.pe_test_set_nms_presorted(1)


RAW_NAMES = C.names("threshold", "threshold_wide", "degenerate", "nonfinite_scores", "nonfinite_boxes", "dead_rows", "seams")


@pytest.mark.parametrize("name", RAW_NAMES)
def test_nms_batched_raw_matches_oracle(L, hooks, name):
    raw_both_settings(L, hooks, name, C.get(name), C.want(name))


def one_full_image(name):
    case = C.get(name)
    B, n = case.scores.shape
    return B == 1 and case.counts is None and case.valid is None and case.max_out == n


FULL_NAMES = [n for n in RAW_NAMES if one_full_image(n)]
ORACLE_AGAIN_MAX = 5200        # rows up to which a second oracle run (the other dispatch form) is affordable


def batched_mode(case):
    return 1 if case.boxes.size > 20000 else 0      # torchvision's dispatch rule on a GPU


@pytest.mark.parametrize("name", [n for n in FULL_NAMES
                                  if batched_mode(C.get(n)) == C.get(n).mode or C.get(n).scores.shape[1] <= ORACLE_AGAIN_MAX])
def test_batched_nms_matches_oracle(L, name):
    """layers.batched_nms takes the coordinate trick up to 20000 box elements and the per-class form beyond, like torchvision:
    a single-class case with a non-finite coordinate has one answer as nms and another as batched_nms."""
    case = C.get(name)
    if batched_mode(case) == case.mode:
        want = C.want(name)
    else:
        with np.errstate(all="ignore"):
            want = [O.batched_nms_f32(case.boxes[0], case.scores[0], case.idxs[0], case.thr, device_type="cuda")]
    got = L.batched_nms(cu(case.boxes[0]), cu(case.scores[0]), cu(case.idxs[0]), case.thr)
    assert got.dtype == torch.int64
    got = got.cpu().numpy()
    same_lists(f"{name}: batched_nms", case, got[None], [len(got)], want)


@pytest.mark.parametrize("name", [n for n in FULL_NAMES if len(np.unique(C.get(n).idxs)) == 1
                                  and (C.get(n).mode == 1 or C.get(n).scores.shape[1] <= ORACLE_AGAIN_MAX)])
def test_nms_matches_oracle(L, name):
    """layers.nms has no coordinate trick: a non-finite coordinate stays in its own row."""
    case = C.get(name)
    if case.mode == 1:
        want = C.want(name)
    else:
        with np.errstate(all="ignore"):
            want = [O.nms_f32(case.boxes[0], case.scores[0], case.thr)]
    got = L.nms(cu(case.boxes[0]), cu(case.scores[0]), case.thr)
    assert got.dtype == torch.int64
    got = got.cpu().numpy()
    same_lists(f"{name}: nms", case, got[None], [len(got)], want)


@pytest.mark.parametrize("name", C.names("dead_rows"))
def test_dead_rows_never_take_part(L, hooks, name):
    """NaN, +-Inf, -5 and 1e30 in rows that are masked out or beyond counts: the same keep lists as with those rows zeroed."""
    case = C.get(name)
    zeroed = C.zero_dead_rows(case)
    raw_both_settings(L, hooks, name + " (dead rows zeroed)", zeroed, C.want(name))
    keep, cnt = run_raw(L, case)
    keep0, cnt0 = run_raw(L, zeroed)
    np.testing.assert_array_equal(cnt, cnt0)
    for b in range(len(cnt)):
        np.testing.assert_array_equal(keep[b, : cnt[b]], keep0[b, : cnt0[b]])


@pytest.mark.parametrize("name", ["seam_batch_counts0", "seam_batch_valid0"])
def test_gather_boxes_copies_bits_and_zero_fills(L, name):
    """pe_gather_boxes on the NMS output of the seam batch (one image keeps nothing): row p < counts[n] holds the bits of input
    row keep[n, p] - the gathered tensors are random bit patterns, NaN payloads and subnormals included - and every row from
    counts[n] on is zero."""
    from proben_amd import _lib
    case = C.get(name)
    B, n = case.scores.shape
    keep, cnt = L.nms_batched_raw(cu(case.boxes), cu(case.scores), cu(case.idxs), cu(case.counts), cu(case.valid), case.thr,
                                  case.mode, case.max_out)
    same_lists(name, case, keep.cpu().numpy(), cnt.cpu().numpy(), C.want(name))
    rng = np.random.default_rng(C.seed_of("gather", name))
    boxes = rng.integers(-2 ** 31, 2 ** 31, (B, n, 4)).astype(np.int32)
    scores = rng.integers(-2 ** 31, 2 ** 31, (B, n)).astype(np.int32)
    out_b = torch.full((B, case.max_out, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out_s = torch.full((B, case.max_out), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    db, ds = cu(boxes), cu(scores)
    st = _lib.lib().pe_gather_boxes(_lib.ptr(db), _lib.ptr(ds), _lib.ptr(keep), _lib.ptr(cnt), B, n, case.max_out,
                                    _lib.ptr(out_b), _lib.ptr(out_s), _lib.stream())
    _lib.check(st, "pe_gather_boxes")
    out_b, out_s = out_b.cpu().numpy(), out_s.cpu().numpy()
    for b, w in enumerate(C.want(name)):
        np.testing.assert_array_equal(out_b[b, : len(w)], boxes[b][w])
        np.testing.assert_array_equal(out_s[b, : len(w)], scores[b][w])
        assert not out_b[b, len(w):].any() and not out_s[b, len(w):].any()
    assert len(C.want(name)[1]) == 0


@pytest.mark.parametrize("n", C.SCRATCH_N)
def test_nms_stays_inside_the_scratch_it_asks_for(n):
    """pe_nms_batched with exactly pe_nms_scratch_bytes(B, n) bytes, B = 3, between two 4 KiB guards of 0xA5: the result is the
    oracle's and no guard byte changes."""
    from proben_amd import _lib
    name = f"scratch_n{n}"
    case = C.get(name)
    B, GUARD = case.scores.shape[0], 4096
    lib = _lib.lib()
    nbytes = int(lib.pe_nms_scratch_bytes(B, n))
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    scratch = buf[GUARD: GUARD + nbytes]
    keep = torch.full((B, case.max_out), -1, dtype=torch.int32, device="cuda")
    cnt = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    b, s, i, c = cu(case.boxes), cu(case.scores), cu(case.idxs), cu(case.counts)
    st = lib.pe_nms_batched(_lib.ptr(b), _lib.ptr(s), _lib.ptr(i), _lib.ptr(c), None, B, n, float(case.thr), case.mode,
                            case.max_out, _lib.ptr(keep), _lib.ptr(cnt), _lib.ptr(scratch), nbytes, _lib.stream())
    _lib.check(st, "pe_nms_batched")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()), "bytes in front of the scratch were written"
    assert bool((buf[GUARD + nbytes:] == 0xA5).all()), "bytes behind the stated scratch size were written"
    same_lists(name, case, keep.cpu().numpy(), cnt.cpu().numpy(), C.want(name))
    st = lib.pe_nms_batched(_lib.ptr(b), _lib.ptr(s), _lib.ptr(i), _lib.ptr(c), None, B, n, float(case.thr), case.mode,
                            case.max_out, _lib.ptr(keep), _lib.ptr(cnt), _lib.ptr(scratch), nbytes - 1, _lib.stream())
    assert st != 0, "one byte less than the stated size must be refused"
