"""options.FusionOptions without a device: the messages the entry points have always given come from building the object with the entry
point's name, options= beside an option keyword is refused, the detector counts of weights, table and matrix are held against each
other, and from_args gives what demo_probEn's six per-option resolvers gave (flag, else the calibration file's entry, else none; the
expected values are written out here)."""
import numpy as np
import pytest
import torch

NAMES = ["thermal_only", "early_fusion"]
TABLE = [[0.0, 0.0, 0.0, 0.0], [-0.1, -0.9, 0.2, 0.0], [-1.3, 0.1, 0.3, 0.0], [1.6, 1.5, 1.1, 0.0]]
MATRIX = [[0.1, 0.4], [0.4, 0.2]]
LOG = ("probEn-log", "v-avg")


def _opts(*a, **kw):
    from proben_amd.options import FusionOptions
    return FusionOptions(*a, **kw)


@pytest.mark.parametrize("who", ["fuse_batch", "fusion", "fuse_detections", "late_fusion", "FramePairPipeline"])
def test_the_messages_of_the_entry_points(who):
    table, corr = np.zeros((4, 4)), np.array(MATRIX)
    for mode in ("probEn", "avg", "max"):
        for kw, msg in ((dict(class_prior=[0.2, 0.5, 0.2, 0.1]), "class_prior belongs to score_fusion 'probEn-log'"),
                        (dict(pool_weights=[1.0, 1.0]), "pool_weights belong to score_fusion 'probEn-log'"),
                        (dict(with_posterior=True), "with_posterior belongs to score_fusion 'probEn-log'"),
                        (dict(presence=table), "presence belongs to score_fusion 'probEn-log'")):
            with pytest.raises(ValueError, match=f"{who}: {msg}"):
                _opts(mode, "v-avg", who=who, num_detectors=2, **kw)
        with pytest.raises(ValueError, match=f"{who}: box_fusion 'c-avg' belongs to score_fusion 'probEn-log'"):
            _opts(mode, "c-avg", box_correlation=corr, who=who)
    with pytest.raises(ValueError, match=f"{who}: unknown score_fusion 'probEn-lg'"):
        _opts("probEn-lg", who=who)
    with pytest.raises(ValueError, match=f"{who}: box_fusion 'c-avg' needs a box_correlation"):
        _opts("probEn-log", "c-avg", who=who)
    with pytest.raises(ValueError, match=f"{who}: box_correlation belongs to box_fusion 'c-avg'"):
        _opts(*LOG, box_correlation=corr, who=who)
    with pytest.raises(ValueError, match=f"{who}: 2 temperatures for 3 detectors"):
        _opts(temperatures=[1.0, 2.0], num_detectors=3, who=who)
    with pytest.raises(ValueError, match=f"{who}: 3 variance scales for 2 detectors"):
        _opts(variance_scales=[1.0, 2.0, 3.0], num_detectors=2, who=who)
    with pytest.raises(ValueError, match="variance scale of detector 2 -2.0 is not finite and > 0"):
        _opts(variance_scales=[1.0, -2.0], num_detectors=2, who=who)
    for bad, msg in (([1.0], f"{who}: 1 pool weights for 2 detectors"), ([float("nan"), 1.0], "not finite"),
                     ([-1.0, 1.0], "not finite and >= 0"), ([0.0, 0.0], "all 0")):
        with pytest.raises(ValueError, match=msg):
            _opts(*LOG, pool_weights=bad, num_detectors=2, who=who)
    with pytest.raises(ValueError, match=f"{who}: presence has 4 rows for 3 detectors"):
        _opts(*LOG, presence=table, num_detectors=3, who=who)
    with pytest.raises(ValueError, match=f"{who}: presence: entry .*nan.* \\(pattern 0, column 0\\) is not finite"):
        _opts(*LOG, presence=np.full((4, 4), np.nan), num_detectors=2, who=who)
    with pytest.raises(ValueError, match=f"{who}: box_correlation is over 2 detectors, not 3"):
        _opts("probEn-log", "c-avg", box_correlation=corr, num_detectors=3, who=who)
    with pytest.raises(ValueError, match=f"{who}: box_correlation is not symmetric"):
        _opts("probEn-log", "c-avg", box_correlation=[[0.0, 0.1], [0.2, 0.0]], num_detectors=2, who=who)
    with pytest.raises(ValueError, match="class_prior .* has an entry that is not finite and > 0"):
        _opts(*LOG, class_prior=[0.5, 0.0, 0.25, 0.25], who=who)


def test_what_the_object_holds():
    o = _opts(*LOG, class_prior=[1, 1, 1, 1], num_detectors=2)
    assert o.temperatures == [1.0, 1.0] and o.logp and not o.cavg and not o.needs_row_source and not o.needs_cluster
    np.testing.assert_array_equal(o.class_prior, [0.25] * 4)
    plain = _opts(num_detectors=2)
    assert plain.temperatures is None and not plain.logp and plain.class_prior is None and plain.named(NAMES) == {}
    for kw in (dict(pool_weights=[0.5, 2.0]), dict(presence=TABLE), dict(box_fusion="c-avg", box_correlation=MATRIX)):
        o = _opts("probEn-log", **kw)
        assert o.needs_row_source and o.needs_cluster and o.num_detectors == 2 and o.temperatures == [1.0, 1.0]
    assert _opts(*LOG, with_posterior=True).num_detectors is None
    full = _opts("probEn-log", "c-avg", [1.5, 0.8], [0.1, 0.2, 0.3, 0.4], [0.5, 2.0], [0.6, 0.5], True, TABLE, MATRIX, num_detectors=2)
    assert list(full.named(NAMES)) == ["temperatures", "class_prior", "variance_scales", "pool_weights", "presence", "box_correlation"]
    assert full.named(NAMES)["presence"] == {"detectors": NAMES, "table": TABLE}
    assert full.named(NAMES)["box_correlation"] == {"detectors": NAMES, "matrix": MATRIX}
    assert full.named(NAMES)["temperatures"] == {"thermal_only": 1.5, "early_fusion": 0.8}
    other = full.replace(box_fusion="v-avg", box_correlation=None, with_posterior=False)
    assert other.pool_weights == [0.6, 0.5] and other.box_correlation is None and not other.with_posterior and full.with_posterior


def test_detector_counts_are_held_against_each_other():
    three = np.zeros((3, 3))
    with pytest.raises(ValueError, match="who: 2 pool weights beside a box correlation over 3 detectors"):
        _opts("probEn-log", "c-avg", pool_weights=[1.0, 1.0], box_correlation=three, who="who")
    with pytest.raises(ValueError, match="who: 3 pool weights beside a presence table over 2 detectors"):
        _opts(*LOG, pool_weights=[1.0, 1.0, 1.0], presence=TABLE, who="who")
    with pytest.raises(ValueError, match="who: a box correlation over 3 detectors beside a presence table over 2"):
        _opts("probEn-log", "c-avg", presence=TABLE, box_correlation=three, who="who")


def test_options_beside_an_option_keyword_is_a_type_error():
    from proben_amd import fusion as F
    from proben_amd.late_fusion import apply_late_fusion_and_evaluate, fused_clusters, late_fusion, presence_rows
    from proben_amd.pipeline import FramePairPipeline
    o = _opts(*LOG, num_detectors=2)
    t = torch.zeros((2, 4), dtype=torch.float64)
    info = {"img_name": "x", "bbox": [[0.0, 0.0, 10.0, 10.0]], "score": [0.9], "class": [0], "prob": [[0.9, 0.05, 0.03]], "vars": [[1.0]]}
    calls = [lambda kw: F.fuse_batch(t, t[:, 0], t[:, :3], t[:, 0], t[:, 0].int(), torch.tensor([0, 2], dtype=torch.int32), options=o, **kw),
             lambda kw: F.fuse_detections([], options=o, **kw),
             lambda kw: late_fusion([{}, {}], list(LOG), options=o, **kw),
             lambda kw: FramePairPipeline([None, None], options=o, **kw),
             lambda kw: apply_late_fusion_and_evaluate(None, None, {}, {}, list(LOG), options=o, **kw)]
    for kw in (dict(class_prior=[0.1, 0.2, 0.3, 0.4]), dict(pool_weights=[1.0, 1.0]), dict(with_posterior=True), dict(presence=TABLE),
               dict(box_correlation=MATRIX)):
        for call in calls[:4] if "with_posterior" in kw else calls:       # the driver has fused_out for it
            with pytest.raises(TypeError, match="options= was given together with " + next(iter(kw))):
                call(kw)
    for kw in (dict(temperatures=[1.0, 1.0]), dict(variance_scales=[1.0, 1.0])):
        for call in calls[1:] + [lambda kw: fused_clusters([{}, {}], options=o, **kw), lambda kw: presence_rows([{}, {}], options=o, **kw),
                                 lambda kw: F.fusion(list(LOG), info, info, options=o, **kw)]:
            with pytest.raises(TypeError, match="options= was given together with " + next(iter(kw))):
                call(kw)
    with pytest.raises(TypeError, match="another fusion"):
        F.fuse_detections([], "avg", options=o)
    with pytest.raises(ValueError, match="fuse_detections: options for 2 detectors, 3 given"):
        F.fuse_detections([{}, {}, {}], options=o)
    pipe = FramePairPipeline([None, None], options=o, concurrent=False)
    assert pipe.options is o and pipe.method == LOG and pipe.temperatures == [1.0, 1.0] and pipe.logp


# ---- from_args ------------------------------------------------------------------------------------------------------------------------

def _file(tmp_path, presence_over=NAMES):
    from proben_amd import calibration as C
    p = str(tmp_path / "cal.json")
    C.save(p, {"thermal_only": 1.5, "early_fusion": 0.8, "middle_fusion": 2.0}, class_prior=[1, 2, 3, 4],
           pool_weights={"thermal_only": 0.6, "early_fusion": 0.5, "middle_fusion": 0.25},
           presence={"detectors": list(presence_over), "columns": 4, "table": TABLE, "hi": None},
           box_correlation={"detectors": NAMES, "matrix": MATRIX}, fitted_image_ids=[3, 5])
    C.save_variance(p, {"thermal_only": 0.25, "early_fusion": 4.0, "middle_fusion": 1.0})
    return p


def _from_args(monkeypatch, argv, names=NAMES):
    from proben_amd import calibration as C
    from proben_amd.opt import config_parser
    from proben_amd.options import FusionOptions
    loads, said = [], []
    real = C.load
    monkeypatch.setattr(C, "load", lambda path: loads.append(path) or real(path))
    opts = FusionOptions.from_args(config_parser(argv + ["--detectors", ",".join(names)]), names, say=said.append)
    return opts, loads, said


def test_from_args_flags_only(monkeypatch):
    o, loads, said = _from_args(monkeypatch, ["--score_fusion", "probEn-log", "--box_fusion", "c-avg", "--temperatures", "early_fusion=0.9,thermal_only=1.4",
                                              "--class_prior", "2,5,2,1", "--variance_scales", "0.5,2", "--pool_weights", "0.6,0.5",
                                              "--presence", "thermal_only=-0.1:-0.9:0:0,thermal_only+early_fusion=1:2:3:0",
                                              "--box_correlation", "0.6", "--write_fused", "f.json"])
    assert loads == [] and said == [] and o.fitted == set()
    assert o.temperatures == [1.4, 0.9] and o.variance_scales == [0.5, 2.0] and o.pool_weights == [0.6, 0.5] and o.with_posterior
    assert o.named(NAMES)["class_prior"] == (np.array([2.0, 5.0, 2.0, 1.0]) / 10.0).tolist()
    assert o.presence.tolist() == [[0.0] * 4, [-0.1, -0.9, 0.0, 0.0], [0.0] * 4, [1.0, 2.0, 3.0, 0.0]]
    assert o.box_correlation.tolist() == [[0.0, 0.6], [0.6, 0.0]]
    assert (o.score_fusion, o.box_fusion, o.num_detectors) == ("probEn-log", "c-avg", 2)
    none, loads, said = _from_args(monkeypatch, [])
    assert none.named(NAMES) == {} and not none.with_posterior and loads == [] and said == []
    log, _, _ = _from_args(monkeypatch, ["--score_fusion", "probEn-log"])
    assert log.named(NAMES) == {"temperatures": {"thermal_only": 1.0, "early_fusion": 1.0}}
    with pytest.raises(ValueError, match="needs --box_correlation or a --calibration file"):
        _from_args(monkeypatch, ["--score_fusion", "probEn-log", "--box_fusion", "c-avg"])


def test_from_args_file_only(monkeypatch, tmp_path):
    p = _file(tmp_path)
    o, loads, said = _from_args(monkeypatch, ["--score_fusion", "probEn-log", "--box_fusion", "c-avg", "--calibration", p])
    assert loads == [p] and o.fitted == {3, 5} and not o.with_posterior
    assert o.temperatures == [1.5, 0.8] and o.variance_scales == [0.25, 4.0] and o.pool_weights == [0.6, 0.5]
    assert o.named(NAMES)["class_prior"] == [0.1, 0.2, 0.3, 0.4]
    assert o.presence.tolist() == TABLE and o.box_correlation.tolist() == MATRIX
    assert said == [f"variance scales of {p}: thermal_only=0.25, early_fusion=4",
                    f"pool weights of {p}: thermal_only=0.6, early_fusion=0.5",
                    f"presence table of {p}: thermal_only=-0.1:-0.9:0.2:0, early_fusion=-1.3:0.1:0.3:0, thermal_only+early_fusion=1.6:1.5:1.1:0",
                    f"box correlation of {p}: thermal_only:thermal_only=0.1, thermal_only:early_fusion=0.4, early_fusion:early_fusion=0.2"]
    # by name: the other order of --detectors turns every per-detector value, the table's bits and the matrix around
    r, _, _ = _from_args(monkeypatch, ["--score_fusion", "probEn-log", "--box_fusion", "c-avg", "--calibration", p], NAMES[::-1])
    assert r.temperatures == [0.8, 1.5] and r.variance_scales == [4.0, 0.25] and r.pool_weights == [0.5, 0.6]
    assert r.presence.tolist() == [TABLE[0], TABLE[2], TABLE[1], TABLE[3]] and r.box_correlation.tolist() == [[0.2, 0.4], [0.4, 0.1]]


def test_from_args_flag_over_file(monkeypatch, tmp_path):
    p = _file(tmp_path)
    o, loads, said = _from_args(monkeypatch, ["--score_fusion", "probEn-log", "--box_fusion", "c-avg", "--calibration", p, "--pool_weights", "0.9,0.1",
                                              "--variance_scales", "early_fusion=3,thermal_only=7", "--class_prior", "1,1,1,1",
                                              "--presence", "early_fusion=1:1:1:0", "--box_correlation", "thermal_only:early_fusion=-0.25"])
    assert loads == [p] and said == []
    assert o.temperatures == [1.5, 0.8] and o.variance_scales == [7.0, 3.0] and o.pool_weights == [0.9, 0.1]
    assert o.named(NAMES)["class_prior"] == [0.25] * 4
    assert o.presence.tolist() == [[0.0] * 4, [0.0] * 4, [1.0, 1.0, 1.0, 0.0], [0.0] * 4]
    assert o.box_correlation.tolist() == [[0.0, -0.25], [-0.25, 0.0]]


def test_from_args_does_not_read_what_the_fusion_has_no_use_for(monkeypatch, tmp_path):
    """The file's presence table is over other detectors: resolving it fails, so a run that passes did not read it."""
    p = _file(tmp_path, presence_over=["thermal_only", "middle_fusion"])
    for mode in ("probEn", "avg", "max"):
        o, loads, said = _from_args(monkeypatch, ["--score_fusion", mode, "--calibration", p])
        assert loads == [p] and said == [f"variance scales of {p}: thermal_only=0.25, early_fusion=4"]
        assert o.named(NAMES) == {"temperatures": {"thermal_only": 1.5, "early_fusion": 0.8},
                                  "variance_scales": {"thermal_only": 0.25, "early_fusion": 4.0}}
        assert o.class_prior is None and o.pool_weights is None and o.presence is None and o.box_correlation is None
    with pytest.raises(ValueError, match="the presence table is over thermal_only,middle_fusion, not thermal_only,early_fusion"):
        _from_args(monkeypatch, ["--score_fusion", "probEn-log", "--calibration", p])
    good = _file(tmp_path)
    o, _, _ = _from_args(monkeypatch, ["--score_fusion", "probEn-log", "--calibration", good])       # v-avg: the matrix is not read
    assert o.box_correlation is None and o.presence.tolist() == TABLE
