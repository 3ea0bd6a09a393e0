"""The calibration statistics against tests/golden/stat_sums_parent.npz: what temperature_nll, pool_nll, reliability,
reliability_scores and variance_stats returned at the commit before their second passes became one kernel
(tests/golden/gen_stat_sums.py describes the cases and builds the inputs; DESIGN.md names the commit).  Bit for bit, by tobytes()
on every returned float64 and every returned integer, the two flag values among them."""
import importlib.util
import os

import numpy as np
import pytest

def _generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_stat_sums.py")
    spec = importlib.util.spec_from_file_location("gen_stat_sums", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "stat_sums_parent.npz"))


@pytest.mark.gpu
@pytest.mark.parametrize("family,case", GEN.CASES, ids=[GEN.case_name(f, c) for f, c in GEN.CASES])
def test_the_statistic_reproduces_the_parents_bits(golden, family, case):
    name = GEN.case_name(family, case)
    f64, i64 = GEN.run_case(family, case)
    want_f, want_i = golden[name + "_f64"], golden[name + "_i64"]
    assert f64.dtype == want_f.dtype == np.float64 and f64.shape == want_f.shape, (name, f64.shape, want_f.shape)
    assert i64.dtype == want_i.dtype == np.int64 and i64.shape == want_i.shape, (name, i64.shape, want_i.shape)
    assert i64.tobytes() == want_i.tobytes(), f"{name}: integers {i64.tolist()} != {want_i.tolist()}"
    assert f64.tobytes() == want_f.tobytes(), f"{name}: {int((f64.view(np.int64) != want_f.view(np.int64)).sum())} of {f64.size} doubles differ"


def test_the_file_holds_what_it_is_meant_to_hold(golden):
    """The fixture itself: a case per name and nothing else, finite sums, excluded items in every case with the last index among
    them, and the workgroup counts 1, 5, 17 and 1024 (capped) in every family."""
    assert sorted(golden.files) == sorted(GEN.case_name(f, c) + s for f, c in GEN.CASES for s in ("_f64", "_i64"))
    blocks, beyond_cap = {}, set()
    for family, case in GEN.CASES:
        name = GEN.case_name(family, case)
        items, bad, last = GEN.items_and_excluded(family, case, golden[name + "_i64"])
        assert np.isfinite(golden[name + "_f64"]).all(), name
        assert 0 < bad < items / 2 and last == items - 1, (name, items, bad, last)
        per = 4 if family in ("temperature", "pool") else 256
        blocks.setdefault(family, set()).add(min(-(-items // per), 1024))
        if items > 1024 * per:          # work beyond the cap: the grid-stride loop runs
            beyond_cap.add(family)
    assert all(v == {1, 5, 17, 1024} for v in blocks.values()) and len(blocks) == 4, blocks
    assert beyond_cap == set(blocks), beyond_cap
