"""fusion.fuse_detections and late_fusion.late_fusion against tests/golden/fuse_options_parent.npz: what they gave, for fifteen
combinations of the fusion's options over two small sets of detector outputs, at the commit before the options moved into
options.FusionOptions (tests/golden/gen_fuse_options.py describes the inputs and the combinations; DESIGN.md section 20 names the
commit).  Every combination is replayed through the keywords, through options= and through one FusionOptions used for two consecutive
calls; bit for bit, by tobytes() on the live rows, NaNs included."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gen(golden_dir):
    spec = importlib.util.spec_from_file_location("gen_fuse_options", os.path.join(golden_dir, "gen_fuse_options.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden(golden_dir, gen):
    z = np.load(os.path.join(golden_dir, "fuse_options_parent.npz"))
    return z, gen.unpack(z["recorded_index"], z["recorded"])


def _same(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k}"


def _recorded(rec, prefix):
    return {k[len(prefix):]: v for k, v in rec.items() if k.startswith(prefix)}


def _host(gen, z, nd):
    return [{k: z[f"n{nd}_d{d}_{k}"] for k in gen.INPUTS} for d in range(nd)]


def _options(gen, z, nd, keys):
    kw = gen.options(nd, keys)
    if gen.E in kw:
        kw[gen.E] = z[f"n{nd}_presence"]           # the table the file was recorded with
    return kw


@pytest.mark.parametrize("idx", range(15))
@pytest.mark.parametrize("nd", [2, 3])
def test_fuse_detections_reproduces_the_parents_bits(golden, gen, nd, idx):
    from proben_amd import fusion as F
    from proben_amd.options import FusionOptions
    z, rec = golden
    assert len(gen.COMBOS) == 15
    score, box, keys = gen.COMBOS[idx]
    want = _recorded(rec, f"{gen.case_name(nd, idx)}_out_")
    assert want["counts"][0] < want["in_counts"][0] and want["counts"][2] == want["in_counts"][2] > 0 and want["counts"][1] == 0
    dets = gen.to_device(_host(gen, z, nd))
    kw = _options(gen, z, nd, keys)
    _same(gen.live_rows(F.fuse_detections(dets, score, box, max_class=gen.MAX_CLASS, **kw)), want, "keywords")
    opts = FusionOptions(score, box, num_detectors=nd, who="test", **kw)
    _same(gen.live_rows(F.fuse_detections(dets, max_class=gen.MAX_CLASS, options=opts)), want, "options=")
    # the pipeline's use: one object, two calls - the second uploads nothing
    dev = dets[0]["scores"].device
    reused = FusionOptions(score, box, num_detectors=nd, who="test", **kw)
    first = gen.live_rows(F.fuse_detections(dets, max_class=gen.MAX_CLASS, options=reused))
    up = reused.on(dev, gen.K + 1)
    ptrs = [None if t is None else t.data_ptr() for t in up]
    for name in ("class_prior", "pool_weights", "presence", "box_correlation"):
        assert (kw.get(name) is None) == (getattr(up, "log_prior" if name == "class_prior" else name) is None), name
    second = gen.live_rows(F.fuse_detections(dets, max_class=gen.MAX_CLASS, options=reused))
    _same(first, want, "reused, first call")
    _same(second, want, "reused, second call")
    again = reused.on(dev, gen.K + 1)
    assert all(a is b for a, b in zip(up, again)) and [None if t is None else t.data_ptr() for t in again] == ptrs
    assert len(reused._on) == 1


@pytest.mark.parametrize("idx", [0, 7, 14])
@pytest.mark.parametrize("nd", [2, 3])
def test_late_fusion_reproduces_the_parents_bits(golden, gen, nd, idx):
    from proben_amd.late_fusion import late_fusion
    from proben_amd.options import FusionOptions
    z, rec = golden
    assert tuple(gen.LATE) == (0, 7, 14)
    score, box, keys = gen.COMBOS[idx]
    want = _recorded(rec, f"{gen.case_name(nd, idx)}_late_")
    assert want["len"].tolist() == [6 if gen.Q in keys else 3, 0, 6 if gen.Q in keys else 3]
    j1 = gen.j1_of(_host(gen, z, nd))
    kw = _options(gen, z, nd, keys)
    _same(gen.late_rows(late_fusion(j1, [score, box], **kw)), want, "keywords")
    opts = FusionOptions(score, box, num_detectors=nd, who="test", **kw)
    _same(gen.late_rows(late_fusion(j1, [score, box], options=opts)), want, "options=")
    _same(gen.late_rows(late_fusion(j1, [score, box], options=opts)), want, "options=, second call")
    torch.cuda.synchronize()


def test_the_file_holds_what_it_is_meant_to_hold(golden, gen, golden_dir):
    """Every combination and both detector sets are there; clusters of 1, 2 and 3 rows occur wherever the sizes are recorded; the
    saturated row is among the inputs; the file stays small."""
    z, rec = golden
    for nd in gen.SETS:
        for idx, (_, _, keys) in enumerate(gen.COMBOS):
            out = _recorded(rec, f"{gen.case_name(nd, idx)}_out_")
            assert {"boxes", "scores", "classes", "counts", "in_counts", "offsets", "stride"} <= set(out)
            if gen.Q in keys:
                assert {1, 2, 3} <= set(out["members"].tolist())
            assert ("cluster" in out) == bool({gen.W, gen.E, gen.C} & set(keys)) and ("pattern" in out) == (gen.E in keys)
        assert (z[f"n{nd}_d1_class_logits"][0, 0] == [800.0, -800.0, -800.0, -800.0]).all()
    assert os.path.getsize(os.path.join(golden_dir, "fuse_options_parent.npz")) < 64 * 1024
