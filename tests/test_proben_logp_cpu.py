"""Log-posterior ProbEn (score_fusion "probEn-log") without a GPU: the argument checks of the three entry points answer before any
device work, the class prior is validated everywhere it can enter, and the calibration file carries it only when asked to."""
import ctypes
import json

import numpy as np
import pytest
import torch


def _lib():
    from proben_amd import _lib
    return _lib.lib()


def _err():
    return _lib().pe_last_error().decode()


ONE = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced: every call below fails in its argument checks


def _fuse_logp(**kw):
    a = dict(boxes=ONE, scores=ONE, log_probs=ONE, variances=ONE, classes=ONE, offsets=ONE, row_counts=None, passthrough=None,
             num_images=1, num_classes=3, max_rows=64, box_mode=0, log_prior=None, out_boxes=ONE, out_scores=ONE, out_classes=ONE,
             out_keep=ONE, out_counts=ONE)
    a.update(kw)
    return _lib().pe_proben_fuse_batch_logp(a["boxes"], a["scores"], a["log_probs"], a["variances"], a["classes"], a["offsets"],
                                            a["row_counts"], a["passthrough"], a["num_images"], a["num_classes"], a["max_rows"],
                                            a["box_mode"], 0.5, 640.0, 512.0, a["log_prior"], a["out_boxes"], a["out_scores"],
                                            a["out_classes"], a["out_keep"], a["out_counts"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(num_images=-1), "num_images < 0"),
    (dict(log_probs=None), "null input pointer"),
    (dict(boxes=None), "null input pointer"),
    (dict(out_keep=None), "null output pointer"),
    (dict(num_classes=0), r"num_classes 0 not in \[1,62\]"),
    (dict(num_classes=63), r"num_classes 63 not in \[1,62\]"),
    (dict(max_rows=0), r"max_rows_per_image 0 not in \[1,2048\]"),
    (dict(max_rows=2049), r"max_rows_per_image 2049 not in \[1,2048\]"),
    (dict(box_mode=4), "bad box_mode 4"),
    (dict(box_mode=-1), "bad box_mode -1"),
])
def test_fuse_batch_logp_argument_checks(kw, msg):
    import re
    assert _fuse_logp(**kw) == -1           # PE_ERR_INVALID_ARG
    assert re.search("pe_proben_fuse_batch_logp: " + msg, _err()), _err()


def test_fuse_batch_logp_refuses_a_bound_that_does_not_fit_and_takes_no_images():
    assert _fuse_logp(max_rows=2000) == -2  # PE_ERR_UNSUPPORTED: 2 000 rows of K + 1 = 4 columns are above 160 KiB
    assert "pe_proben_fuse_batch_logp" in _err() and "LDS" in _err()
    assert _fuse_logp(num_images=0, boxes=None) == 0


def test_the_existing_fuse_entry_still_refuses_the_new_score_mode():
    """An unchanged-behaviour guard, not a demonstration of the feature: pe_proben_fuse_batch refused score_mode > 3 before this mode
    existed and still does (it passes on the parent too); the new mode is reachable through pe_proben_fuse_batch_logp only."""
    L = _lib()
    st = L.pe_proben_fuse_batch(ONE, ONE, ONE, ONE, ONE, ONE, None, None, 1, 3, 64, 4, 0, 0.5, 640.0, 512.0, ONE, ONE, ONE, ONE, ONE, None)
    assert st == -1 and "bad score_mode 4" in _err()


def _pack_lp(**kw):
    tabs = (ctypes.c_void_p * 2)(8, 8)
    temps = (ctypes.c_double * 2)(*kw.pop("temps", (1.0, 1.0)))
    a = dict(boxes=tabs, classes=tabs, logits=tabs, vars=tabs, counts=tabs, temps=temps, nd=2, B=1, D=10, K=3, max_class=2, S=20,
             ob=ONE, os=ONE, op=ONE, olp=ONE, ov=ONE, oc=ONE, ooff=ONE, ocnt=ONE, osingle=ONE)
    a.update(kw)
    return _lib().pe_proben_pack_log_posteriors(a["boxes"], a["classes"], a["logits"], a["vars"], a["counts"], a["temps"], a["nd"], a["B"],
                                                a["D"], a["K"], a["max_class"], a["S"], a["ob"], a["os"], a["op"], a["olp"], a["ov"],
                                                a["oc"], a["ooff"], a["ocnt"], a["osingle"], None)


@pytest.mark.parametrize("kw,msg", [
    (dict(nd=5), "num_detectors 5"),
    (dict(K=0), "num_classes 0"),
    (dict(S=19), "row_stride 19 < 20"),
    (dict(logits=None), "null pointer"),
    (dict(olp=None), r"null output \(out_log_probs\)"),
    (dict(ob=None), "null output"),
    (dict(temps=(1.0, 0.0)), "temperature 0 of detector 1 is not finite and > 0"),
    (dict(temps=(float("nan"), 1.0)), "of detector 0 is not finite and > 0"),
    (dict(logits=(ctypes.c_void_p * 2)(8, 0)), "null pointer of detector 1"),
])
def test_pack_log_posteriors_argument_checks(kw, msg):
    import re
    assert _pack_lp(**kw) == -1
    assert re.search("pe_proben_pack_log_posteriors: .*" + msg, _err()), _err()


@pytest.mark.parametrize("args,msg", [
    ((ONE, 4, 4, 0.0, ONE), "temperature 0 is not finite and > 0"),
    ((ONE, 4, 4, float("inf"), ONE), "temperature inf is not finite and > 0"),
    ((ONE, -1, 4, 1.0, ONE), "num_rows -1"),
    ((ONE, 4, 1, 1.0, ONE), r"num_columns 1 \(K \+ 1\) < 2"),
    ((None, 4, 4, 1.0, ONE), "null pointer"),
    ((ONE, 4, 4, 1.0, None), "null pointer"),
])
def test_log_softmax_argument_checks(args, msg):
    import re
    assert _lib().pe_log_softmax(*args, None) == -1
    assert re.search("pe_log_softmax: " + msg, _err()), _err()


# ---- the class prior ------------------------------------------------------------------------------------------------------------

def test_class_prior_validation():
    from proben_amd.calibration import check_class_prior, parse_class_prior
    p = check_class_prior([2, 5, 2, 1])
    np.testing.assert_array_equal(p, np.array([2, 5, 2, 1]) / 10.0)
    assert p.dtype == np.float64
    np.testing.assert_array_equal(parse_class_prior("0.2, 0.5,0.2,0.1"), np.array([0.2, 0.5, 0.2, 0.1]) / (0.2 + 0.5 + 0.2 + 0.1))
    np.testing.assert_array_equal(check_class_prior([0.3, 0.7], 2), [0.3, 0.7])
    for bad in ([0.5, 0.0, 0.5], [0.5, -0.1, 0.6], [0.5, float("nan")], [0.5, float("inf")], [1.0], [], [[0.5, 0.5]], "abc", [0.5, None]):
        with pytest.raises(ValueError):
            check_class_prior(bad)
    with pytest.raises(ValueError, match=r"lists 3 entries for K \+ 1 = 4"):
        check_class_prior([0.2, 0.3, 0.5], 4)
    for bad in ("0.2,x,0.1", "0.2,,0.8", "", "0.5,0"):
        with pytest.raises(ValueError, match="class_prior"):
            parse_class_prior(bad)


def test_cli_class_prior_flag(capsys):
    from proben_amd.opt import config_parser
    a = config_parser(["--score_fusion", "probEn-log", "--class_prior", "0.2,0.5,0.2,0.1", "--box_fusion", "argmax"])
    assert a.score_fusion == "probEn-log" and a.class_prior == "0.2,0.5,0.2,0.1"
    assert config_parser([]).class_prior is None and config_parser([]).score_fusion == "probEn"
    for sf in ("probEn", "avg", "max"):
        with pytest.raises(SystemExit) as e:
            config_parser(["--score_fusion", sf, "--class_prior", "0.2,0.5,0.2,0.1"])
        assert e.value.code == 2
        assert "--class_prior belongs to --score_fusion probEn-log" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        config_parser(["--score_fusion", "probEn-log", "--class_prior", "0.2,0,0.8"])
    assert "not finite and > 0" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        config_parser(["--score_fusion", "probEn-logs"])


def _info(n=2):
    return {"img_name": "x", "bbox": [[0.0, 0.0, 10.0, 10.0]] * n, "score": [0.9] * n, "class": [0] * n, "prob": [[0.9, 0.05, 0.03]] * n,
            "vars": [[1.0]] * n, "class_logits": [[3.0, 0.0, -1.0, -2.0]] * n}


@pytest.mark.parametrize("sf", ["probEn", "avg", "max"])
def test_class_prior_with_another_score_fusion_raises(sf):
    """Before anything touches the device: these run on a machine without one."""
    from proben_amd import fusion as F
    from proben_amd.late_fusion import late_fusion
    from proben_amd.pipeline import FramePairPipeline
    prior = [0.2, 0.5, 0.2, 0.1]
    t = torch.zeros((2, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match="class_prior belongs to score_fusion 'probEn-log'"):
        F.fusion([sf, "v-avg"], _info(), _info(), class_prior=prior)
    with pytest.raises(ValueError, match="class_prior belongs to score_fusion 'probEn-log'"):
        F.fuse_batch(t, t[:, 0], t[:, :3], t[:, 0], t[:, 0].int(), torch.tensor([0, 2], dtype=torch.int32), sf, "v-avg", class_prior=prior)
    with pytest.raises(ValueError, match="class_prior belongs to score_fusion 'probEn-log'"):
        F.fuse_detections([], sf, "v-avg", class_prior=prior)
    with pytest.raises(ValueError, match="class_prior belongs to score_fusion 'probEn-log'"):
        late_fusion([{}, {}], [sf, "v-avg"], class_prior=prior)
    with pytest.raises(ValueError, match="class_prior belongs to score_fusion 'probEn-log'"):
        FramePairPipeline([], sf, "v-avg", class_prior=prior)


def test_bad_priors_and_missing_inputs_raise_in_the_new_mode():
    from proben_amd import fusion as F
    from proben_amd.late_fusion import late_fusion
    from proben_amd.pipeline import FramePairPipeline
    with pytest.raises(ValueError, match="not finite and > 0"):
        FramePairPipeline([], "probEn-log", "v-avg", class_prior=[0.5, 0.0, 0.25, 0.25])
    pipe = FramePairPipeline([object(), object()], "probEn-log", "s-avg", concurrent=False, class_prior=[1, 1, 1, 1])
    assert pipe.temperatures == [1.0, 1.0] and pipe.logp          # temperatures=None means T = 1 for every detector
    np.testing.assert_array_equal(pipe.class_prior, [0.25] * 4)
    default = FramePairPipeline([object(), object()], concurrent=False)
    assert default.temperatures is None and not default.logp and default.class_prior is None
    with pytest.raises(ValueError, match="unknown score_fusion"):
        FramePairPipeline([], "probEn-lg")
    t = torch.zeros((2, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"needs log_probs \[Ntot, K\+1\]"):
        F.fuse_batch(t, t[:, 0], t[:, :3], t[:, 0], t[:, 0].int(), torch.tensor([0, 2], dtype=torch.int32), "probEn-log", "v-avg")
    # prediction files without class_logits are refused by name before the first launch
    det = {"image": ["a"], "boxes": [[[0, 0, 1, 1]]], "scores": [[0.9]], "classes": [[0]], "image_id": [1], "probs": [[[0.9, 0.05, 0.03]]],
           "vars": [[[1.0]]], "class_logits": [[[]]]}
    with pytest.raises(ValueError, match="val_x.json: no class_logits"):
        late_fusion([det, det], ["probEn-log", "v-avg"], names=["val_x.json", "val_y.json"])
    info = dict(_info(), class_logits=None)
    with pytest.raises(ValueError, match="carries no class_logits"):
        F.fusion(["probEn-log", "v-avg"], info, info)


def test_calibration_file_round_trips_a_class_prior(tmp_path):
    from proben_amd import calibration as C
    plain, with_prior = tmp_path / "a.json", tmp_path / "b.json"
    kw = dict(nll={"thermal_only": {"before": 2.0, "after": 1.0}}, rows={"thermal_only": 10}, holdout=0.5, fitted_image_ids=[1, 2])
    C.save(plain, {"thermal_only": 1.5}, **kw)
    rec = json.load(open(plain))
    assert list(rec) == ["detectors", "nll", "rows", "holdout", "fitted_image_ids"]          # exactly the keys it had
    assert "class_prior" not in C.load(plain)
    C.save(with_prior, {"thermal_only": 1.5}, class_prior=[6, 2, 1, 1], **kw)
    got = C.load(with_prior)
    assert got["class_prior"] == [0.6, 0.2, 0.1, 0.1]
    assert {k: v for k, v in got.items() if k != "class_prior"} == C.load(plain)
    with pytest.raises(ValueError, match="not finite and > 0"):
        C.save(tmp_path / "c.json", {"thermal_only": 1.5}, class_prior=[1, 0, 1])
    bad = dict(rec, class_prior=[0.5, -0.5, 1.0])
    json.dump(bad, open(tmp_path / "d.json", "w"))
    with pytest.raises(ValueError, match="d.json: class_prior"):
        C.load(tmp_path / "d.json")


def test_header_declares_the_mode_and_the_entry_points():
    import os
    from proben_amd import _lib, fusion as F
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "proben_hip.h")).read()
    assert "#define PE_SCORE_PROBEN_LOGP 4" in hdr and F.SCORE_MODES["probEn-log"] == 4
    for name in ("pe_proben_pack_log_posteriors", "pe_log_softmax", "pe_proben_fuse_batch_logp"):
        assert f"int {name}(" in hdr and name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
