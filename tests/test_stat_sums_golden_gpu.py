"""The calibration statistics against tests/golden/stat_sums_parent.npz and stat_sums_parent2.npz: what temperature_nll, pool_nll,
reliability, reliability_scores and variance_stats returned at the commit before their second passes became one kernel, and what
bias_nll and box_pair_stats returned at the commit before the first passes were unified (tests/golden/gen_stat_sums.py describes the
cases and builds the inputs; DESIGN.md names the commits).  Bit for bit, by tobytes() on every returned float64 and every returned
integer, the two flag values among them."""
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
    return {name: np.load(os.path.join(golden_dir, name)) for name in GEN.FILES}


ALL = [(name, f, c) for name, cases in GEN.FILES.items() for f, c in cases]


@pytest.mark.gpu
@pytest.mark.parametrize("file,family,case", ALL, ids=[GEN.case_name(f, c) for _, f, c in ALL])
def test_the_statistic_reproduces_the_parents_bits(golden, file, family, case):
    name = GEN.case_name(family, case)
    f64, i64 = GEN.run_case(family, case)
    want_f, want_i = golden[file][name + "_f64"], golden[file][name + "_i64"]
    assert f64.dtype == want_f.dtype == np.float64 and f64.shape == want_f.shape, (name, f64.shape, want_f.shape)
    assert i64.dtype == want_i.dtype == np.int64 and i64.shape == want_i.shape, (name, i64.shape, want_i.shape)
    assert i64.tobytes() == want_i.tobytes(), f"{name}: integers {i64.tolist()} != {want_i.tolist()}"
    assert f64.tobytes() == want_f.tobytes(), f"{name}: {int((f64.view(np.int64) != want_f.view(np.int64)).sum())} of {f64.size} doubles differ"


def test_the_file_holds_what_it_is_meant_to_hold(golden):
    """The fixtures themselves: a case per name and nothing else, finite sums, excluded items in every case with the last index among
    them, and the workgroup counts 1, 5, 17 and 1024 (capped) in every family."""
    blocks, beyond_cap = {}, set()
    for file, cases in GEN.FILES.items():
        assert sorted(golden[file].files) == sorted(GEN.case_name(f, c) + s for f, c in cases for s in ("_f64", "_i64"))
        for family, case in cases:
            name = GEN.case_name(family, case)
            items, bad, last = GEN.items_and_excluded(family, case, golden[file][name + "_i64"])
            assert np.isfinite(golden[file][name + "_f64"]).all(), name
            assert 0 < bad < items / 2 and last == items - 1, (name, items, bad, last)
            units, per = GEN.first_pass_units(family, case)
            blocks.setdefault(family, set()).add(min(-(-units // per), 1024))
            if units > 1024 * per:          # work beyond the cap: the grid-stride loop runs
                beyond_cap.add(family)
    assert all(v == {1, 5, 17, 1024} for v in blocks.values()) and len(blocks) == 6, blocks
    assert beyond_cap == set(blocks), beyond_cap
