"""The RPN proposal selection (csrc/rpn.hip) candidate by candidate - `cand_boxes`, `cand_scores`, `cand_level`, `cand_valid` and their
ORDER, with no NMS in between to repair it - against a CPU restatement of the first half of `oracle.detector.find_top_proposals`; and
the three box decoders (rpn.hip, boxhead.hip, misc.hip) on rows whose only bad value is one delta or one box coordinate.

Order rule: logit descending, ties by anchor index (h, w, a) ascending - torch's stable descending sort, which puts every NaN first
whatever its sign or payload.  The cases put ties at the cut (grid, flat, plateau, zeros), a plateau across the slice seam at anchor
index 16 383, signed zeros, NaNs of four bit patterns, +-inf logits and single non-finite deltas under selected anchors; the
geometries cover one-stage levels, a level of exactly 16 383 keys, two slices with a short second one and three slices.

Every GPU test first asserts on the CPU that its case holds what it is meant to hold (a tie group the cut splits, the plateau across
the seam, ...), that a wrong anchor of a split tie group would show as a wrong box (the group's taken members and the next 64 are
>= 1e-2 apart, 100 x the box tolerance), and that no expected candidate has a clipped extent in (0, 1e-2), where the device expf
could flip `valid`.  A seed that breaks one of these is replaced, no row is left out."""
import ctypes
import functools

import numpy as np
import pytest
import torch

STRIDES = [4, 8, 16, 32, 64]
SLICE = 16383                      # csrc/rpn.hip kSliceKeys: levels above it are selected in slices (or from memory without scratch)
CHUNK = 1024                       # threads per block: the ordered compaction of the tie group walks the keys in chunks of it
SHAPES = {
    "G1": [(20, 26), (10, 13), (5, 7), (3, 4), (1, 1)],          # one stage; three levels with total < k; a one-cell level
    "G2": [(43, 127), (43, 128), (74, 74), (13, 16), (7, 8)],    # 16 383 keys (one stage); 16 512 (second slice: 129 keys < k); 16 428
    "G3": [(100, 128), (50, 64), (25, 32), (13, 16), (7, 8)],    # three slices on the first level
}
# Unpadded image sizes (clipping).  "tight": the image the pyramid belongs to - boxes clip on all four sides.  "wide": for the small
# top-k values, whose cut falls inside the coarse levels too: anchors of 256 / 512 px in a tight image mostly clip to the whole image,
# and two members of a tie group could then not be told apart by their boxes.
SIZES = {
    ("G1", "tight"): [(75, 100), (80, 104)], ("G1", "wide"): [(1500, 1900), (1600, 2000)],
    ("G2", "tight"): [(1150, 1170), (1184, 1184)],
    ("G3", "tight"): [(390, 500), (400, 512)], ("G3", "wide"): [(1500, 1900), (1600, 2000)],
}
NAN_BITS = [0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFFFFFFF]
FLOOD_LEVEL = {"G1": 0, "G2": 1, "G3": 0}

# (geometry, family, pre_nms_topk, image sizes, seed).  The seeds: the first of 10 x, 10 x + 1, ... with which check_case() holds.
def _cases(family, seeds, ks=(1000,)):
    return [(g, family, k, "wide" if k <= 64 else "tight", seed) for g, seed in seeds.items() for k in ks if k == 1000 or g != "G2"]


CASES = (_cases("grid", {"G1": 101, "G2": 1020, "G3": 103}, ks=(1, 64, 1000, 1024))
         + _cases("flat", {"G1": 110, "G2": 1111, "G3": 112})
         + _cases("plateau", {"G2": 120, "G3": 121})
         + _cases("zeros", {"G1": 130, "G2": 131, "G3": 1320})
         + _cases("nonfinite", {"G1": 140, "G2": 141, "G3": 142})
         + _cases("nan-flood", {"G1": 150, "G2": 151, "G3": 1521}))
ROUTE_CASES = [c for c in CASES if c[0] in ("G2", "G3") and c[1] in ("grid", "plateau", "nonfinite") and c[2] == 1000]


def _id(case):
    return f"{case[0]}-{case[1]}-k{case[2]}"


def _spec():
    from oracle import detector as D
    return D.DetectorSpec()


# ------------------------------------------------------------------------------------------------ reference
def _level_candidates(hd, hw, stride, lvl, size, spec, pre_nms_topk):
    """One (image, level): hd [H, W, 16].  The reference's steps, plus what the case conditions need (all logits, all decoded boxes)."""
    from oracle import detector as D
    H, W = hw
    anchors = D.grid_anchors((H, W), stride, D.cell_anchors(spec.anchor_sizes[lvl], spec.aspect_ratios))
    lg = hd[:, :, :3].reshape(-1)                                     # (h, w, a) order
    dl = hd[:, :, 3:15].reshape(-1, 4)
    k = min(pre_nms_topk, H * W * 3)
    srt, idx = lg.sort(descending=True, stable=True)                  # rpn_outputs.py: full sort, NaN first, ties by index
    idx, score = idx[:k], srt[:k]
    raw_all = D.apply_deltas(dl, anchors, (1.0, 1.0, 1.0, 1.0))       # float32, every anchor - like the reference
    raw = raw_all[idx]
    valid = torch.isfinite(raw).all(dim=1) & torch.isfinite(score)
    box = D.clip_boxes(raw, size)                                     # the UNPADDED size
    valid = valid & ((box[:, 2] - box[:, 0]) > 0) & ((box[:, 3] - box[:, 1]) > 0)
    return {"boxes": box, "scores": score, "level": torch.full((k,), lvl, dtype=torch.int64), "valid": valid, "index": idx,
            "raw": raw, "logits": lg, "raw_all": raw_all}


def _expected(heads, shapes, strides, sizes, spec, pre_nms_topk):
    N = heads[0].shape[0]
    per_level = [[_level_candidates(hd[n], hw, st, lvl, sizes[n], spec, pre_nms_topk)
                  for lvl, (hd, hw, st) in enumerate(zip(heads, shapes, strides))] for n in range(N)]
    images = [{key: torch.cat([lv[key] for lv in levels]) for key in ("boxes", "scores", "level", "valid")} for levels in per_level]
    return images, per_level


def expected_candidates(heads, shapes, strides, sizes, spec, pre_nms_topk):
    """CPU restatement of the first half of oracle.detector.find_top_proposals (everything before NMS), from the oracle's own
    cell_anchors / grid_anchors / apply_deltas / clip_boxes.  heads[l]: [N, H, W, 16] (columns 0..2 logits, 3..14 deltas).
    Returns per image {"boxes" [ncand, 4], "scores", "level", "valid"} in candidate order (level-major, rank within the level)."""
    return _expected(heads, shapes, strides, sizes, spec, pre_nms_topk)[0]


def _oracle_test_inputs(two_stage):
    """The inputs of tests/test_ops_gpu.py::test_rpn_select_matches_oracle."""
    g = torch.Generator().manual_seed(77)
    N = 2
    shapes = [(100, 128), (50, 64), (25, 32), (13, 16), (7, 8)] if two_stage else [(40, 52), (20, 26), (10, 13), (5, 7), (3, 4)]
    heads = []
    for (h, w) in shapes:
        hd = torch.randn(N, h, w, 16, generator=g)
        hd[..., 3:15] *= 0.5
        hd[0, 0, 0, 0] = float("nan")
        hd[1, 1, 1, 5] = float("inf")
        hd[:, 2, :, 1] = 0.25
        heads.append(hd)
    sizes = [(390, 500), (400, 512)] if two_stage else [(150, 200), (160, 208)]
    return heads, shapes, sizes


@pytest.mark.parametrize("two_stage", [False, True])
def test_expected_candidates_pin_the_oracle(two_stage):
    """The helper's valid rows through the oracle's NMS at 0.7, first 1000 == oracle.detector.select_proposals, exactly."""
    from oracle import detector as D
    from oracle import nms as onms
    spec = D.DetectorSpec()
    heads, shapes, sizes = _oracle_test_inputs(two_stage)
    lg_l = [hd[..., :3].permute(0, 3, 1, 2).contiguous() for hd in heads]
    dl_l = [hd[..., 3:15].permute(0, 3, 1, 2).contiguous() for hd in heads]
    want = D.select_proposals(lg_l, dl_l, STRIDES, sizes, spec)
    got = expected_candidates(heads, shapes, STRIDES, sizes, spec, spec.pre_nms_topk)
    for n, e in enumerate(got):
        v = e["valid"]
        assert 0 < int(v.sum()) < len(v)
        b, s, l = e["boxes"][v], e["scores"][v], e["level"][v]
        keep = onms.batched_nms_f32(b.numpy(), s.numpy(), l.numpy(), 0.7, device_type=spec.nms_device_semantics)
        keep = torch.from_numpy(keep)[:1000]
        assert torch.equal(b[keep], want[n][0]) and torch.equal(s[keep], want[n][1])


# ------------------------------------------------------------------------------------------------ cases
def _set_bits(t, index, bits):
    """t: contiguous float32 [L]; writes raw bit patterns."""
    t.view(torch.int32)[index] = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32)


def _delta(hd, n, anchor, col):
    """Position of one delta of one anchor inside the head tensor [N, H, W, 16]."""
    N, H, W, _ = hd.shape
    return hd.view(N, H * W, 16)[n, anchor // 3], 3 + (anchor % 3) * 4 + col


@functools.lru_cache(maxsize=None)
def _case(case):
    """-> (heads, shapes, sizes, k, info).  info[(n, level)] holds what the family planted there."""
    geom, family, k, size_key, seed = case
    shapes, sizes = SHAPES[geom], SIZES[(geom, size_key)]
    g = torch.Generator().manual_seed(seed)
    N, heads, info = 2, [], {}
    for lvl, (h, w) in enumerate(shapes):
        hd = torch.randn(N, h, w, 16, generator=g)
        hd[..., 3:15] *= 0.5                                          # random deltas: a wrong anchor is a wrong box
        total = h * w * 3
        lg = hd[..., :3].reshape(N, total).contiguous()
        for n in range(N):
            if family == "grid":                                      # ties everywhere, the cut included
                lg[n] = torch.round(torch.randn(total, generator=g) * 4) / 4
            elif family == "flat":
                lg[n] = 0.75 * lvl - 1.5 * n
            elif family == "plateau":
                lg[n] = torch.randn(total, generator=g) - 10.0
                if total > SLICE + 2200:
                    start, run = SLICE - (400, 2000)[n], 2500          # image 0: the taken members straddle the seam
                elif total > SLICE:
                    start, run = 14000, total - 14000                  # to the end of the level, 45 / 129 anchors after the seam
                else:
                    start, run = total // 3, total // 2
                n_above = min((300, 10)[n], total // 8)
                outside = torch.cat([torch.arange(0, start), torch.arange(start + run, total)])
                above = outside[torch.randperm(len(outside), generator=g)[:n_above]]
                lg[n, start:start + run] = 0.5
                lg[n, above] = 1.0 + torch.rand(n_above, generator=g)
                info[(n, lvl)] = {"start": start, "run": run, "n_above": n_above}
            elif family == "zeros":
                lg[n] = torch.where(torch.rand(total, generator=g) < 0.5, 0.0, -0.0)
                pos = torch.randperm(total, generator=g)[:min(100, total // 4)]
                lg[n, pos] = 0.5 + torch.rand(len(pos), generator=g)
                info[(n, lvl)] = {"n_pos": len(pos)}
            elif family == "nonfinite":
                if total >= 64:
                    at = torch.randperm(total, generator=g)[:13].tolist()
                    _set_bits(lg[n], at[:4], NAN_BITS)
                    lg[n, at[4]], lg[n, at[5]] = float("inf"), float("-inf")
                    plants = [(0, float("nan")), (2, float("nan")), (2, float("inf")), (2, float("-inf")), (0, float("inf")),
                              (3, float("nan")), (1, float("nan"))]
                    for j, (a, (col, val)) in enumerate(zip(at[6:], plants)):
                        lg[n, a] = 50.0 + j                           # high enough to be selected
                        row, c = _delta(hd, n, a, col)
                        row[c] = val
                    info[(n, lvl)] = {"nan": at[:4], "pinf": at[4], "ninf": at[5], "deltas": list(zip(at[6:], plants))}
                else:
                    _set_bits(lg[n], [total - 1], [NAN_BITS[1]])      # every anchor is taken: the negative NaN must come FIRST
                    info[(n, lvl)] = {"nan": [total - 1]}
            elif family == "nan-flood":
                if lvl == FLOOD_LEVEL[geom]:
                    at = torch.randperm(total, generator=g)[:1200]    # more than k NaNs, fewer than k of either sign
                    pick = torch.randint(0, 4, (len(at),), generator=g).tolist()
                    _set_bits(lg[n], at, [NAN_BITS[p] for p in pick])
                    info[(n, lvl)] = {"flood": len(at)}
            else:
                raise AssertionError(family)
        hd[..., :3] = lg.view(N, h, w, 3)
        heads.append(hd)
    return heads, shapes, sizes, k, info


@functools.lru_cache(maxsize=None)
def _case_expected(case):
    heads, shapes, sizes, k, _ = _case(case)
    return _expected(heads, shapes, STRIDES, sizes, _spec(), k)


def _same_key(lg, t):
    """The members of the tie group of the value t under the order rule: every NaN ties with every NaN, -0.0 with +0.0."""
    return torch.isnan(lg) if bool(torch.isnan(t)) else lg == t


def check_case(case):
    """The conditions that keep the comparison honest, and that the case holds what it is meant to hold.  CPU only.
    Returns {(n, level): (tie group size at the cut, members of it taken)} for the levels the cut splits."""
    from oracle import detector as D
    geom, family, k, _, _ = case
    heads, shapes, sizes, _, info = _case(case)
    images, per_level = _case_expected(case)
    splits = {}
    for n, levels in enumerate(per_level):
        for lvl, e in enumerate(levels):
            total, kk = len(e["logits"]), len(e["index"])
            assert kk == min(k, total)
            # no borderline validity: a clipped extent is exactly 0 or at least 1e-2
            fin = torch.isfinite(e["raw"]).all(dim=1)
            ext = torch.stack([e["boxes"][fin, 2] - e["boxes"][fin, 0], e["boxes"][fin, 3] - e["boxes"][fin, 1]], dim=1)
            assert bool(((ext == 0) | (ext >= 1e-2)).all()), (case, n, lvl, "borderline extent", ext[(ext != 0) & (ext < 1e-2)])
            # the tie group at the cut
            member = _same_key(e["logits"], e["scores"][-1]).nonzero().squeeze(1)            # ascending anchor index
            taken = int(_same_key(e["scores"], e["scores"][-1]).sum())
            assert torch.equal(e["index"][kk - taken:], member[:taken]), (case, n, lvl)      # the reference's own tie rule
            if len(member) == taken:
                continue
            splits[(n, lvl)] = (len(member), taken)
            # discriminating boxes: the taken members and the next 64, pairwise >= 1e-2 apart (valid ones: only those are compared)
            m = member[:taken + 64]
            mb = D.clip_boxes(e["raw_all"][m], sizes[n])
            ok = torch.isfinite(e["raw_all"][m]).all(dim=1) & ((mb[:, 2] - mb[:, 0]) > 0) & ((mb[:, 3] - mb[:, 1]) > 0)
            mb = mb[ok]
            dist = (mb[:, None, :] - mb[None, :, :]).abs().amax(dim=2)
            dist.fill_diagonal_(float("inf"))
            assert len(mb) < 2 or float(dist.min()) >= 1e-2, (case, n, lvl, "tie members too close", float(dist.min()))
    big = [(n, lvl) for n in range(2) for lvl, (h, w) in enumerate(shapes) if h * w * 3 > k]
    if family == "grid":
        # the cut splits a tie group on every level of at least 1500 anchors, where a group at the cut has ~10 members or more
        # (k = 1 is the edge of k itself: its cut is the maximum, tied or not)
        if k >= 64:
            must = [key for key in big if shapes[key[1]][0] * shapes[key[1]][1] * 3 >= 1500]
            assert must and all(key in splits for key in must), (case, sorted(splits))
    elif family == "flat":
        assert all(key in splits for key in big)
        for n, levels in enumerate(per_level):
            for e in levels:
                assert torch.equal(e["index"], torch.arange(len(e["index"])))               # the first k anchors
    elif family == "plateau":
        seam = [key for key in big if shapes[key[1]][0] * shapes[key[1]][1] * 3 > SLICE]
        assert seam and all(key in splits for key in big)
        for (n, lvl) in seam:
            p, e = info[(n, lvl)], per_level[n][lvl]
            size, taken = splits[(n, lvl)]
            assert p["run"] > 2048 and p["start"] <= SLICE < p["start"] + p["run"] and p["n_above"] < k
            assert size == p["run"] and taken == k - p["n_above"] and 0 < taken < size
            first, last = int(e["index"][k - taken]), int(e["index"][-1])
            assert first == p["start"] and first // CHUNK < last // CHUNK                    # the base is carried over a chunk
        # three slices, image 0: the taken members lie on both sides of the slice seam
        if geom == "G3":
            e = per_level[0][0]
            assert int(e["index"][-1]) > SLICE > int(e["index"][k - splits[(0, 0)][1]])
    elif family == "zeros":
        for key in big:
            n_pos = info[key]["n_pos"]
            sc = per_level[key[0]][key[1]]["scores"]
            assert key in splits and splits[key][1] == k - n_pos and 0 < n_pos < k
            bits = sc[n_pos:].view(torch.int32)
            assert bool((sc[:n_pos] > 0).all()) and bool((bits == 0).any()) and bool((bits == -(1 << 31)).any())   # +0.0 and -0.0
    elif family == "nonfinite":
        planted = set()
        for (n, lvl), p in info.items():
            e = per_level[n][lvl]
            lg_bits = e["logits"].view(torch.int32)[p["nan"]].tolist()
            planted.update(b & 0xFFFFFFFF for b in lg_bits)
            assert bool(torch.isnan(e["scores"][:len(p["nan"])]).all()) and sorted(e["index"][:len(p["nan"])].tolist()) == sorted(p["nan"])
            if "deltas" not in p:
                continue
            sel = {int(a): i for i, a in enumerate(e["index"].tolist())}
            assert p["pinf"] in sel and not bool(e["valid"][sel[p["pinf"]]])
            assert (p["ninf"] in sel) == (len(e["logits"]) <= k)
            for a, (col, val) in p["deltas"]:
                assert a in sel, (case, n, lvl, a)
                only_clamped = col == 2 and val == float("inf")                              # +inf in dw: clamped, a valid box
                assert bool(e["valid"][sel[a]]) == only_clamped, (case, n, lvl, a, col, val)
                assert bool(torch.isfinite(e["raw"][sel[a]]).all()) == (only_clamped or (col == 2 and val == float("-inf")))
        assert planted == set(NAN_BITS)
    elif family == "nan-flood":
        lvl = FLOOD_LEVEL[geom]
        for n in range(2):
            e = per_level[n][lvl]
            assert info[(n, lvl)]["flood"] > k and bool(torch.isnan(e["scores"]).all()) and not bool(e["valid"].any())
            bits = e["logits"].view(torch.int32)[torch.isnan(e["logits"])]
            assert 0 < int((bits < 0).sum()) < k and 0 < int((bits > 0).sum()) < k           # a key that ranks by sign takes finite logits
            assert {b & 0xFFFFFFFF for b in bits.tolist()} == set(NAN_BITS)
            assert (n, lvl) in splits
    for n, im in enumerate(images):
        assert int(im["valid"].sum()) > 0
    return splits


# ------------------------------------------------------------------------------------------------ device side
def run_select(heads, shapes, strides, sizes, spec, pre_nms_topk, scratch="exact"):
    """pe_rpn_select_topk through ctypes -> (cand_boxes, cand_scores, cand_level, cand_valid) on the CPU, nothing in between.
    scratch: "exact" = pe_rpn_scratch_bytes, "none" = no scratch pointer, "short" = 8 bytes less than needed."""
    import proben_amd  # noqa: F401
    from proben_amd import _lib
    from proben_amd.rcnn import SCALE_CLAMP, cell_anchor_table
    lib = _lib.lib()
    N, nl = heads[0].shape[0], len(shapes)
    hd_dev = [h.cuda().contiguous() for h in heads]
    ncand = sum(min(pre_nms_topk, h * w * 3) for h, w in shapes)
    cb = torch.full((N, ncand, 4), -7777.0, device="cuda")
    cs = torch.full((N, ncand), -7777.0, device="cuda")
    cl = torch.full((N, ncand), -7, dtype=torch.int32, device="cuda")
    cv = torch.full((N, ncand), 7, dtype=torch.uint8, device="cuda")
    ptrs = (ctypes.c_void_p * nl)(*[h.data_ptr() for h in hd_dev])
    hw = (ctypes.c_int32 * (2 * nl))(*sum([list(s) for s in shapes], []))
    cells = (ctypes.c_float * (12 * nl))(*cell_anchor_table(spec.anchor_sizes[:nl], spec.aspect_ratios))
    sz = torch.tensor(sizes, dtype=torch.int32).cuda()
    full = int(lib.pe_rpn_scratch_bytes(hw, nl, N))
    assert (full > 0) == any(h * w * 3 > SLICE for h, w in shapes)
    buf = torch.empty(max(full, 8), dtype=torch.uint8, device="cuda")
    if scratch == "exact":
        sp, sbytes = _lib.ptr(buf), full
    elif scratch == "short":
        assert full >= 8
        sp, sbytes = _lib.ptr(buf), full - 8
    else:
        assert scratch == "none"
        sp, sbytes = None, 0
    st = lib.pe_rpn_select_topk(ptrs, hw, (ctypes.c_int32 * nl)(*strides[:nl]), cells, nl, N, 16, pre_nms_topk, _lib.ptr(sz),
                                SCALE_CLAMP, _lib.ptr(cb), _lib.ptr(cs), _lib.ptr(cl), _lib.ptr(cv), ncand, sp, sbytes, _lib.stream())
    _lib.check(st, "pe_rpn_select_topk")
    torch.cuda.synchronize()
    return cb.cpu(), cs.cpu(), cl.cpu(), cv.cpu()


def assert_candidates(got, want, what):
    """Every (image, candidate): level and valid exact; score bitwise (NaN where the expected score is NaN); boxes of valid rows."""
    cb, cs, cl, cv = got
    for n, w in enumerate(want):
        assert cl.shape[1] == len(w["level"])
        bad = (cl[n].long() != w["level"]).nonzero().squeeze(1)
        assert len(bad) == 0, (what, n, "cand_level", bad[:8].tolist())
        nan = torch.isnan(w["scores"])
        bad = (torch.isnan(cs[n]) != nan).nonzero().squeeze(1)
        assert len(bad) == 0, (what, n, "cand_scores: NaN places", bad[:8].tolist(), cs[n][bad[:8]].tolist(), w["scores"][bad[:8]].tolist())
        bad = ((cs[n].view(torch.int32) != w["scores"].view(torch.int32)) & ~nan).nonzero().squeeze(1)
        assert len(bad) == 0, (what, n, "cand_scores: bits", bad[:8].tolist(), cs[n][bad[:8]].tolist(), w["scores"][bad[:8]].tolist())
        bad = (cv[n] != w["valid"].to(torch.uint8)).nonzero().squeeze(1)
        assert len(bad) == 0, (what, n, "cand_valid", bad[:8].tolist(), cv[n][bad[:8]].tolist(), w["scores"][bad[:8]].tolist())
        v = w["valid"]
        err = (cb[n][v] - w["boxes"][v]).abs().max().item()
        print(f"{what} image {n}: {int(v.sum())}/{len(v)} valid, {int(nan.sum())} NaN scores, max |box error| {err:.3g}")
        np.testing.assert_allclose(cb[n][v].numpy(), w["boxes"][v].numpy(), rtol=1e-5, atol=1e-4,     # expf: device vs libm
                                   err_msg=f"{what} image {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_rpn_candidates_match_the_reference(case):
    splits = check_case(case)
    heads, shapes, sizes, k, _ = _case(case)
    print(f"{_id(case)}: cut splits a tie group on (image, level) -> (group, taken): {splits}")
    got = run_select(heads, shapes, STRIDES, sizes, _spec(), k, scratch="exact")
    assert_candidates(got, _case_expected(case)[0], _id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROUTE_CASES, ids=_id)
def test_rpn_routes_are_identical(case):
    """Slices + merge (scratch given), the whole level from memory (no scratch) and the same with a scratch 8 bytes short:
    the four outputs byte for byte, the boxes of invalid rows included."""
    check_case(case)
    heads, shapes, sizes, k, _ = _case(case)
    assert any(h * w * 3 > SLICE for h, w in shapes)
    outs = {r: run_select(heads, shapes, STRIDES, sizes, _spec(), k, scratch=r) for r in ("exact", "none", "short")}
    for r in ("none", "short"):
        for name, a, b in zip(("cand_boxes", "cand_scores", "cand_level", "cand_valid"), outs["exact"], outs[r]):
            assert a.numpy().tobytes() == b.numpy().tobytes(), (_id(case), r, name)
    assert_candidates(outs["none"], _case_expected(case)[0], _id(case) + " (no scratch)")


# ------------------------------------------------------------------------------------------------ decoders
def _rand_boxes(g, n, span=800.0, wh=250.0):
    xy = torch.rand(n, 2, generator=g) * span
    return torch.cat([xy, xy + 1.0 + torch.rand(n, 2, generator=g) * wh], dim=1)


BAD = (float("nan"), float("inf"), float("-inf"))


@pytest.mark.gpu
@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)])
def test_apply_deltas_on_single_bad_columns(weights):
    """Box2BoxTransform.apply_deltas (pe_box2box_apply_deltas) against oracle.detector.apply_deltas: NaN, +inf and -inf one at a time
    in each delta column and in each box coordinate, every plant in a row of its own.  torch.clamp(max=) propagates NaN."""
    import proben_amd
    from oracle import detector as D
    g = torch.Generator().manual_seed(61)
    R, k = 64, 3
    boxes = _rand_boxes(g, R)
    d = torch.randn(R, 4 * k, generator=g) * 0.5 * torch.tensor(weights).repeat(k)
    d[2, 2], d[3, 7], d[4, 10] = 30.0 * weights[2], 30.0 * weights[3], -30.0 * weights[2]     # finite, beyond the clamp / far below
    plants, r = [], 8
    for col in range(4):
        for v in BAD:
            cls = r % k
            d[r, 4 * cls + col] = v
            plants.append((r, cls, col, v))
            r += 1
    box_rows = []
    for coord in range(4):
        for v in BAD:
            boxes[r, coord] = v
            box_rows.append(r)
            r += 1
    assert r <= R
    want = D.apply_deltas(d, boxes, weights)
    fw = torch.isfinite(want)
    # the case: a bad delta poisons its own class only, except that +inf in dw / dh is clamped and -inf gives a zero extent (both
    # finite); a bad coordinate poisons every class of its row; every other row is finite
    for (row, cls, col, v) in plants:
        own = fw[row, 4 * cls: 4 * cls + 4]
        others = torch.cat([fw[row, :4 * cls], fw[row, 4 * cls + 4:]])
        assert bool(others.all()) and bool(own.all()) == (col >= 2 and v in (float("inf"), float("-inf"))), (row, cls, col, v)
    assert all(bool((~fw[row]).view(k, 4).any(dim=1).all()) for row in box_rows)
    clean = [i for i in range(R) if i not in box_rows and i not in [p[0] for p in plants]]
    assert bool(fw[clean].all())
    got = proben_amd.Box2BoxTransform(weights).apply_deltas(d.cuda(), boxes.cuda()).cpu()
    fg = torch.isfinite(got)
    assert torch.equal(fg, fw), {"hip_only_nonfinite": (~fg & fw).nonzero().tolist(), "oracle_only_nonfinite": (fg & ~fw).nonzero().tolist()}
    np.testing.assert_allclose(got[fw].numpy(), want[fw].numpy(), rtol=3e-6, atol=1e-4)


@pytest.mark.gpu
def test_boxhead_drops_rows_with_one_nan_extent_delta():
    """pe_boxhead_candidates + pe_boxhead_finalize against select_detections + postprocess, as test_boxhead_matches_oracle_quirks does,
    on rows that are finite except for a NaN in dw of one class or in dh of another, and whose confident class is a THIRD one: the
    reference decodes every class, finds a NaN box and drops the whole row, every class of it."""
    import proben_amd  # noqa: F401
    from oracle import detector as D
    from proben_amd import _lib
    from proben_amd import layers as L
    from proben_amd.rcnn import SCALE_CLAMP
    g = torch.Generator().manual_seed(67)
    N, P, K, stride = 2, 64, 3, 24
    head = torch.zeros(N, P, stride)
    head[..., : K + 1] = torch.randn(N, P, K + 1, generator=g) * 2.5
    head[..., K + 1: 5 * K + 1] = torch.randn(N, P, 4 * K, generator=g)
    head[..., 5 * K + 1] = torch.randn(N, P, generator=g) * 0.5
    # (image, row, class with the NaN, dw = 2 / dh = 3, confident class)
    plants = [(0, 7, 0, 2, 1), (0, 20, 2, 3, 0), (0, 41, 1, 3, 2), (1, 3, 1, 2, 0), (1, 30, 0, 3, 2)]
    for (n, r, c, col, top) in plants:
        head[n, r, K + 1 + 4 * c + col] = float("nan")
        head[n, r, top] = 9.0
    props = torch.stack([_rand_boxes(g, P) for _ in range(N)])
    pcnt = torch.tensor([64, 40], dtype=torch.int32)
    sizes, outs = [(800, 1000), (768, 960)], [(512, 640), (492, 614)]
    spec = D.DetectorSpec()
    probs_ref = torch.softmax(head[..., : K + 1], dim=-1)
    for (n, r, c, col, top) in plants:
        assert r < int(pcnt[n]) and top != c and float(probs_ref[n, r, top]) > spec.score_thresh
        assert int(torch.isnan(head[n, r]).sum()) == 1 and bool(torch.isfinite(props[n, r]).all())
    dev, cmax, D_ = "cuda", P * K, 100
    hd, pr = head.view(N * P, stride).cuda(), props.cuda()
    cb = torch.empty(N, cmax, 4, device=dev); cs = torch.empty(N, cmax, device=dev)
    cc = torch.empty(N, cmax, dtype=torch.int32, device=dev); cr = torch.empty(N, cmax, 2, dtype=torch.int32, device=dev)
    ccnt = torch.empty(N, dtype=torch.int32, device=dev); ctot = torch.empty(N, dtype=torch.int32, device=dev)
    probs = torch.empty(N, P, K + 1, device=dev)
    sz = torch.tensor(sizes, dtype=torch.int32, device=dev); osz = torch.tensor(outs, dtype=torch.int32, device=dev)
    lib = _lib.lib()
    _lib.check(lib.pe_boxhead_candidates(_lib.ptr(hd), stride, N, P, K, _lib.ptr(pcnt.cuda()), _lib.ptr(pr), _lib.ptr(sz),
                                         (ctypes.c_float * 4)(10, 10, 5, 5), SCALE_CLAMP, 0.5, cmax, _lib.ptr(cb), _lib.ptr(cs),
                                         _lib.ptr(cc), _lib.ptr(cr), _lib.ptr(ccnt), _lib.ptr(ctot), _lib.ptr(probs), _lib.stream()), "cand")
    assert torch.equal(ctot, ccnt)
    keep, kcnt = L.nms_batched_raw(cb, cs, cc, ccnt, None, 0.5, 0, D_)
    o = {k: torch.empty(s, dtype=t, device=dev) for k, s, t in [
        ("boxes", (N, D_, 4), torch.float32), ("scores", (N, D_), torch.float32), ("classes", (N, D_), torch.int32),
        ("logits", (N, D_, K + 1), torch.float32), ("probs", (N, D_, K), torch.float32), ("vars", (N, D_), torch.float32),
        ("rows", (N, D_), torch.int32), ("counts", (N,), torch.int32)]}
    _lib.check(lib.pe_boxhead_finalize(_lib.ptr(hd), stride, N, P, K, cmax, D_, 0, _lib.ptr(probs), _lib.ptr(cb), _lib.ptr(cs),
                                       _lib.ptr(cc), _lib.ptr(cr), _lib.ptr(keep), _lib.ptr(kcnt), _lib.ptr(sz), _lib.ptr(osz),
                                       _lib.ptr(o["boxes"]), _lib.ptr(o["scores"]), _lib.ptr(o["classes"]), _lib.ptr(o["logits"]),
                                       _lib.ptr(o["probs"]), _lib.ptr(o["vars"]), _lib.ptr(o["rows"]), _lib.ptr(o["counts"]),
                                       _lib.stream()), "final")
    for n in range(N):
        r = int(pcnt[n])
        h = head[n, :r]
        # quirk Q3 indexes the variance with candidate ids: the reference's candidate list must stay below the row count
        assert int((probs_ref[n, :r, :K] > spec.score_thresh).sum()) < r
        det = D.select_detections(h[:, : K + 1], h[:, K + 1: 5 * K + 1], torch.exp(h[:, 5 * K + 1: 5 * K + 2]), props[n, :r], sizes[n], spec)
        want = D.postprocess(det, sizes[n], outs[n])
        c = int(o["counts"][n])
        print(f"image {n}: {c} detections, the reference {len(want['boxes'])}; candidates {int(ccnt[n])}")
        assert len(want["boxes"]) > 0
        assert c == len(want["boxes"]), (n, c, len(want["boxes"]))
        np.testing.assert_array_equal(o["classes"][n, :c].cpu().numpy(), want["classes"].numpy())
        np.testing.assert_allclose(o["scores"][n, :c].cpu().numpy(), want["scores"].numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(o["boxes"][n, :c].cpu().numpy(), want["boxes"].numpy(), rtol=1e-5, atol=2e-4)
        np.testing.assert_array_equal(o["logits"][n, :c].cpu().numpy(), want["class_logits"].numpy())
        np.testing.assert_allclose(o["probs"][n, :c].cpu().numpy(), want["prob_score"].numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(o["vars"][n, :c].cpu().numpy(), want["vars"].numpy().reshape(-1), rtol=2e-6)
