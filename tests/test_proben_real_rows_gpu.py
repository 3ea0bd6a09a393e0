"""Kernel-only A/B of ProbEn on the detector rows it is actually fed.

The oracle detectors' rows of tests/golden/fused_map_sets.npz (frame, box x4, score, class, prob x3, var) are saturated the way a trained
box head's are: f64 sum(p) above 1 (a negative background term and a NaN score after fusion), 1 - sum(p) below 1e-6, scores of exactly
1.0f - which the Dirichlet rows of the synthetic tests never are.  The same rows go through the product's fusion (per-batch device dicts
in forward_batch's layout -> fusion.fuse_detections -> pe_proben_pack_detections -> pe_proben_fuse_batch, parity_map.hip_fused_rows) and
through the oracle's per-image driver (parity_map.oracle_fused_rows); no detector runs.  Frame by frame the fused rows must be the same
(count, classes, NaN places, finite scores to 1e-6, float32 boxes) and so must the COCO AP / AP50 / AP75 of the two routes (to 1e-9):
the kernel part of the fused-mAP delta of DESIGN.md 9.2 is zero, set by set."""
import os

import numpy as np
import pytest

from parity_map import coco_stats, fixture_batches, fixture_ground_truth, fused_rows_mismatch, hip_fused_rows, oracle_fused_rows

pytestmark = pytest.mark.gpu

ALL_SETS = [("probEn", "v-avg"), ("avg", "s-avg")]
SOME_SETS = [("probEn", "s-avg"), ("avg", "v-avg"), ("max", "avg"), ("probEn", "argmax")]
_SETS = {}


def fixture_sets(golden_dir):
    """[(seed, oracle thermal rows, oracle RGB rows, ground truth)] of all 24 sets; the ground truth is labelled_frames' own (the
    frames themselves are not needed here)."""
    if "sets" not in _SETS:
        e = np.load(os.path.join(golden_dir, "fused_map_sets.npz"))
        n = int(e["n_frames"])
        seeds = sorted(int(k[2:]) for k in e.files if k.startswith("t_") and f"r_{k[2:]}" in e.files)
        gts = fixture_ground_truth(n, seeds)
        _SETS["sets"] = (n, [(s, e[f"t_{s}"], e[f"r_{s}"], g) for s, g in zip(seeds, gts)])
    return _SETS["sets"]


def test_the_fixture_rows_are_saturated(golden_dir):
    """The premise: the rows exercise the edge the synthetic cases never reach (counted on the first set, seed 7002)."""
    n, sets = fixture_sets(golden_dir)
    assert len(sets) == 24
    rows = np.concatenate(sets[0][1:3])
    p = rows[:, 7:10].astype(np.float64)
    bg = 1.0 - p[:, 0] - p[:, 1] - p[:, 2]
    assert (bg < 0).sum() >= 10 and (bg < 1e-6).sum() >= 100 and (rows[:, 5] == np.float32(1.0)).sum() >= 10


@pytest.mark.parametrize("method", ALL_SETS + SOME_SETS, ids=lambda m: "/".join(m))
def test_product_fusion_equals_the_oracle_on_the_detector_rows(golden_dir, method):
    n, sets = fixture_sets(golden_dir)
    if method in SOME_SETS:
        sets = sets[::6]        # four sets spread over the seeds
    assert len(sets) >= 4
    for seed, rt, rr, gts in sets:
        ora = oracle_fused_rows(rt, rr, n, method)
        hip = hip_fused_rows(fixture_batches(rt, rr, n), method)
        mm = fused_rows_mismatch(ora, hip)
        assert mm is None, (method, seed, mm)
        so, sh = coco_stats(gts, ora), coco_stats(gts, hip)
        np.testing.assert_allclose(sh[:3], so[:3], rtol=0, atol=1e-9, err_msg=f"{method} seed {seed}: kernel-only AP delta")
