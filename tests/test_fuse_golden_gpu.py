"""fusion.fuse_batch against tests/golden/fuse_parent.npz: what it returned at the commit before csrc/proben.hip's rules, LDS layout and
argument table were each stated once (tests/golden/gen_fuse_parent.py describes the runs and builds the inputs; DESIGN.md section 24
names the commit).  Bit for bit, by tobytes(): the counts, every image's live rows of boxes, scores, classes, keep, vars and members, and
the whole of the prefilled arrays cluster, log_posterior and pattern."""
import importlib.util
import os

import numpy as np
import pytest


def _generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_fuse_parent.py")
    spec = importlib.util.spec_from_file_location("gen_fuse_parent", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()
RUNS = GEN.runs()


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "fuse_parent.npz"))
    return {k: z[k] for k in z.files}


def _want(golden, r, i, f):
    k = int(golden["index"][r, i, f])
    return None if k < 0 else golden["blob"][int(golden["ends"][k - 1]) if k else 0:int(golden["ends"][k])].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(len(RUNS)), ids=[GEN.run_name(run) for run in RUNS])
def test_fuse_batch_reproduces_the_parents_bits(golden, r):
    name = GEN.run_name(RUNS[r])
    assert golden["runs"][r] == name
    got = GEN.run_case(RUNS[r])
    for f, field in enumerate(GEN.FIELDS):
        images = len(got[field]) if field in got else 0
        for i in range(golden["index"].shape[1]):
            want = _want(golden, r, i, f)
            assert (want is not None) == (i < images), f"{name}: image {i} {field}: the output is {'missing' if want else 'unexpected'}"
            if want is not None:
                have = np.ascontiguousarray(got[field][i])
                assert have.tobytes() == want, f"{name}: image {i} {field} differs: {have.tolist()} != {np.frombuffer(want, have.dtype).tolist()}"


def test_the_file_holds_what_it_is_meant_to_hold(golden):
    """The fixture itself: a row of the index per run and nothing else, every byte string used, the outputs each mode has and no others,
    the overflowing image answered with -1, both sides of the form switch present, and a size that stays small."""
    assert list(golden["runs"]) == [GEN.run_name(run) for run in RUNS] and list(golden["fields"]) == list(GEN.FIELDS)
    index = golden["index"]
    assert index.shape == (len(RUNS), len(GEN.SIZES), len(GEN.FIELDS))
    assert sorted(set(index[index >= 0].tolist())) == list(range(len(golden["ends"]))) and int(golden["ends"][-1]) == len(golden["blob"])
    for r, ((s, box, pool, post, pres, prior, D), form, R) in enumerate(RUNS):
        have = {field for f, field in enumerate(GEN.FIELDS) if index[r, 0, f] >= 0}
        want = {"counts", "boxes", "scores", "classes", "keep"} | ({"cluster"} if pool or pres else set()) | \
            ({"log_posterior", "vars", "members"} if post else set()) | ({"pattern"} if pres else set())
        assert have == want, (GEN.run_name(RUNS[r]), have)
        counts = [np.frombuffer(_want(golden, r, i, 0), np.int32)[0] for i in range(1 if form == "over" else len(GEN.SIZES))]
        assert counts == [-1] if form == "over" else min(counts) >= 0 and counts[0] == 0 and counts[1] == 1, (GEN.run_name(RUNS[r]), counts)
    assert {R for _, _, R in RUNS} >= {GEN.form_switch(GEN.K + 1, 0, 0), GEN.form_switch(GEN.K + 1, 0, 0) + 2,
                                       GEN.form_switch(GEN.K + 1, 1, 1), GEN.form_switch(GEN.K + 1, 1, 1) + 2}
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuse_parent.npz")) < 256 * 1024


def test_the_file_tells_the_summation_order(golden):
    """Every "probEn-log" case: the float32 score the file holds for the "cancel" group (gen_fuse_parent.SPECIAL) differs in bits from
    the score with the members summed in reversed order and lies nearer to the score in cluster order (the host's restatement of the
    rule; its exp may differ from the device's in the last float64 bit, the two orders differ by many float32 steps)."""
    pivot = GEN.SPECIAL["cancel"][2]
    for r, (case, form, R) in enumerate(RUNS):
        if case[0] != "probEn-log" or form != "counts" or R != GEN.TIGHT:
            continue
        fwd, rev = next((v, w) for _, v, w, b, row in GEN.host_scores(case) if (b, row) == (GEN.BIG, pivot))
        keep = np.frombuffer(_want(golden, r, GEN.BIG, GEN.FIELDS.index("keep")), np.int32)
        have = np.frombuffer(_want(golden, r, GEN.BIG, GEN.FIELDS.index("scores")), np.float32)[list(keep).index(pivot)]
        assert have.tobytes() != np.float32(rev).tobytes() and abs(float(have) - fwd) < abs(float(have) - rev), (GEN.run_name(RUNS[r]), have, fwd, rev)
