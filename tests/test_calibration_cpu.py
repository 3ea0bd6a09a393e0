"""Temperature calibration without a GPU: the argument checks of pe_proben_pack_logits / pe_calibrated_softmax / pe_temperature_nll
(they answer before any device work and name the offending value), calibration.match_labels on hand-worked cases, the calibration
file, and the drivers' flag handling."""
import ctypes
import json

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.lib()


def _err(L):
    return L.pe_last_error().decode()


def _pack(L, temps, nd=2, tables=True, outs=True, row_stride=None, D=8):
    """pe_proben_pack_logits with plausible (never dereferenced) pointers."""
    tab = (ctypes.c_void_p * 5)(*([4096] * 5)) if tables else None
    T = (ctypes.c_double * 5)(*(list(temps) + [1.0] * (5 - len(temps)))) if temps is not None else None
    o = 4096 if outs else None
    return L.pe_proben_pack_logits(tab, tab, tab, tab, tab, T, nd, 2, D, 3, 2, nd * D if row_stride is None else row_stride,
                                   o, o, o, o, o, o, o, o, None)


@pytest.mark.parametrize("bad,shown", [(0.0, "0"), (-1.5, "-1.5"), (float("nan"), "nan"), (float("inf"), "inf")])
def test_bad_temperatures_are_named(L, bad, shown):
    assert _pack(L, [1.0, bad]) == -1
    assert "pe_proben_pack_logits" in _err(L) and shown in _err(L) and "detector 1" in _err(L)
    assert L.pe_calibrated_softmax(4096, 10, 4, bad, 4096, None) == -1
    assert "pe_calibrated_softmax" in _err(L) and shown in _err(L)
    ts = (ctypes.c_double * 3)(1.0, 2.0, bad)
    assert L.pe_temperature_nll(4096, 4096, 10, 4, ts, 3, 4096, 4096, 4096, None) == -1
    assert "pe_temperature_nll" in _err(L) and shown in _err(L) and "candidate 2" in _err(L)


def test_pack_logits_limits(L):
    assert _pack(L, [1.0] * 5, nd=5) == -1 and "num_detectors 5" in _err(L)
    assert _pack(L, [], nd=0) == -1 and "num_detectors 0" in _err(L)
    assert _pack(L, [1.0, 1.0], row_stride=15) == -1 and "row_stride 15 < 16" in _err(L)
    assert _pack(L, [1.0, 1.0], tables=False) == -1 and "null pointer" in _err(L)
    assert _pack(L, None) == -1 and "null pointer" in _err(L)
    assert _pack(L, [1.0, 1.0], outs=False) == -1 and "null output" in _err(L)
    tab = (ctypes.c_void_p * 2)(4096, 0)           # detector 1 has no logits
    ok = (ctypes.c_void_p * 2)(4096, 4096)
    T = (ctypes.c_double * 2)(1.0, 1.0)
    assert L.pe_proben_pack_logits(ok, ok, tab, ok, ok, T, 2, 2, 8, 3, 2, 16, *([4096] * 8), None) == -1
    assert "null pointer of detector 1" in _err(L)


def test_temperature_nll_limits(L):
    ts = (ctypes.c_double * 65)(*([1.0] * 65))
    assert L.pe_temperature_nll(4096, 4096, 10, 4, ts, 0, 4096, 4096, 4096, None) == -1 and "num_temperatures 0" in _err(L)
    assert L.pe_temperature_nll(4096, 4096, 10, 4, ts, 65, 4096, 4096, 4096, None) == -1 and "num_temperatures 65" in _err(L)
    assert L.pe_temperature_nll(4096, 4096, 10, 4, None, 3, 4096, 4096, 4096, None) == -1 and "null pointer" in _err(L)
    assert L.pe_temperature_nll(None, 4096, 10, 4, ts, 3, 4096, 4096, 4096, None) == -1 and "null pointer (logits" in _err(L)
    assert L.pe_temperature_nll(4096, None, 10, 4, ts, 3, 4096, 4096, 4096, None) == -1 and "null pointer (logits" in _err(L)
    assert L.pe_temperature_nll(4096, 4096, 10, 4, ts, 3, None, 4096, 4096, None) == -1 and "null pointer (workspace" in _err(L)
    assert L.pe_temperature_nll(4096, 4096, 10, 4, ts, 3, 4096, 4096, None, None) == -1 and "null pointer (workspace" in _err(L)
    assert L.pe_temperature_nll(4096, 4096, 10, 1, ts, 3, 4096, 4096, 4096, None) == -1 and "num_columns 1" in _err(L)
    assert L.pe_temperature_nll(4096, 4096, -3, 4, ts, 3, 4096, 4096, 4096, None) == -1 and "num_rows -3" in _err(L)
    assert L.pe_calibrated_softmax(None, 10, 4, 1.0, 4096, None) == -1 and "null pointer" in _err(L)
    assert L.pe_calibrated_softmax(4096, 10, 1, 1.0, 4096, None) == -1 and "num_columns 1" in _err(L)


def test_python_layer_refuses_cpu_tensors_and_bad_temperatures(L):
    import proben_amd
    from proben_amd import calibration as C
    with pytest.raises(proben_amd._lib.HipLibraryError):
        C.calibrated_probs(torch.zeros((4, 4)), 1.0)
    with pytest.raises(proben_amd._lib.HipLibraryError):
        C.temperature_nll(torch.zeros((4, 4)), torch.zeros((4,), dtype=torch.int32), [1.0])
    for bad in (0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="not finite and > 0"):
            C.check_temperature(bad)
    with pytest.raises(ValueError, match="2 temperatures for 3 detectors"):
        from proben_amd.pipeline import FramePairPipeline
        FramePairPipeline([None, None, None], temperatures=[1.0, 2.0], concurrent=False)


# ---- match_labels, by hand -------------------------------------------------------------------------------------------------

def test_match_labels_equal_iou_takes_the_lower_index():
    from proben_amd.calibration import match_labels
    # the detection covers both ground-truth boxes' halves: IoU 50 / 100 with either
    lab = match_labels([[0, 0, 10, 10]], [0], [[0, 0, 10, 5], [0, 5, 10, 10]], [2, 1])
    assert lab.tolist() == [2] and lab.dtype == torch.int32
    lab = match_labels([[0, 0, 10, 10]], [0], [[0, 5, 10, 10], [0, 0, 10, 5]], [1, 2])
    assert lab.tolist() == [1]


def test_match_labels_iou_of_exactly_one_half_counts_and_the_own_class_does_not():
    from proben_amd.calibration import match_labels
    # inter 8 x 4 = 32, union 32 + 64 - 32 = 64: IoU = 0.5 exactly; one unit less overlap -> 28 / 68 < 0.5
    boxes = [[0, 0, 8, 4], [0, 0, 7, 4], [100, 100, 110, 110]]
    lab = match_labels(boxes, [0, 0, 0], [[0, 0, 8, 8]], [1])
    assert lab.tolist() == [1, 3, 3]                      # predicted class 0 plays no part; 3 = background at K = 3
    assert match_labels(boxes, [0, 0, 0], [[0, 0, 8, 8]], [1], iou_thresh=0.4).tolist() == [1, 1, 3]
    # the best-overlapping box decides, not the first above the threshold
    lab = match_labels([[0, 0, 10, 10]], [2], [[0, 0, 10, 6], [0, 0, 10, 9]], [0, 1])
    assert lab.tolist() == [1]


def test_match_labels_without_ground_truth_everything_is_background():
    from proben_amd.calibration import match_labels
    assert match_labels([[0, 0, 5, 5], [1, 1, 2, 2]], [0, 1], [], []).tolist() == [3, 3]
    assert match_labels([[0, 0, 5, 5]], [0], np.zeros((0, 4)), np.zeros((0,)), num_classes=1).tolist() == [1]
    assert match_labels([], [], [[0, 0, 5, 5]], [1]).tolist() == []


def test_match_labels_ignores_crowd_boxes():
    from proben_amd.calibration import match_labels
    gt, cls = [[0, 0, 10, 10], [0, 0, 10, 7]], [0, 2]
    assert match_labels([[0, 0, 10, 10]], [1], gt, cls).tolist() == [0]
    assert match_labels([[0, 0, 10, 10]], [1], gt, cls, gt_crowd=[1, 0]).tolist() == [2]     # the perfect match is a crowd box
    assert match_labels([[0, 0, 10, 10]], [1], gt, cls, gt_crowd=[1, 1]).tolist() == [3]


# ---- calibration file, flags -----------------------------------------------------------------------------------------------

def test_calibration_file_round_trip(tmp_path):
    from proben_amd import calibration as C
    p = tmp_path / "cal.json"
    C.save(p, {"thermal_only": 1.37, "early_fusion": 0.8125}, {"thermal_only": {"before": 10.5, "after": 9.25}}, {"thermal_only": 1200},
           holdout=0.5, fitted_image_ids=[10, 11])
    rec = C.load(p)
    assert rec["detectors"] == {"thermal_only": 1.37, "early_fusion": 0.8125}
    assert rec["nll"]["thermal_only"] == {"before": 10.5, "after": 9.25} and rec["rows"] == {"thermal_only": 1200}
    assert rec["holdout"] == 0.5 and rec["fitted_image_ids"] == [10, 11]
    assert set(json.load(open(p))) >= {"detectors", "nll", "rows"}
    with pytest.raises(ValueError, match="early_fusion"):
        C.save(p, {"early_fusion": 0.0})
    (tmp_path / "bad.json").write_text(json.dumps({"detectors": {"thermal_only": -1}}))
    with pytest.raises(ValueError, match="thermal_only"):
        C.load(tmp_path / "bad.json")
    (tmp_path / "none.json").write_text("{}")
    with pytest.raises(ValueError, match="not a calibration file"):
        C.load(tmp_path / "none.json")


def test_temperatures_match_detectors_by_position_or_by_name():
    from proben_amd import calibration as C
    names = ["thermal_only", "early_fusion", "middle_fusion"]
    assert C.parse_temperatures("1.5,0.8,2", names) == [1.5, 0.8, 2.0]
    assert C.parse_temperatures("middle_fusion=2,thermal_only=1.5,early_fusion=0.8", names) == [1.5, 0.8, 2.0]
    assert C.resolve({"early_fusion": 0.8, "thermal_only": 1.5, "rgb_only": 3.0}, names[:2], "cal.json") == [1.5, 0.8]
    with pytest.raises(ValueError, match="2 values for 3"):
        C.parse_temperatures("1.5,0.8", names)
    with pytest.raises(ValueError, match="no temperature for middle_fusion"):
        C.parse_temperatures("thermal_only=1.5,early_fusion=0.8", names)
    with pytest.raises(ValueError, match="mixes"):
        C.parse_temperatures("1.5,early_fusion=0.8,2", names)
    with pytest.raises(ValueError, match="not finite and > 0"):
        C.parse_temperatures("1.5,0,2", names)
    with pytest.raises(ValueError, match="cal.json has no temperature for middle_fusion"):
        C.resolve({"thermal_only": 1.0, "early_fusion": 1.0}, names, "cal.json")


def test_cli_flags_are_mutually_exclusive(capsys):
    from proben_amd.opt import config_parser
    a = config_parser(["--temperatures", "1,2"])
    assert a.temperatures == "1,2" and a.calibration is None
    a = config_parser(["--calibration", "c.json"])
    assert a.calibration == "c.json" and a.temperatures is None
    a = config_parser([])
    assert a.temperatures is None and a.calibration is None
    with pytest.raises(SystemExit):
        config_parser(["--temperatures", "1,2", "--calibration", "c.json"])
    assert "not allowed with" in capsys.readouterr().err


def _j1(logits):
    return {"image": ["a.jpeg", "b.jpeg"], "boxes": [[[0, 0, 5, 5]], [[1, 1, 6, 6], [2, 2, 8, 8]]], "scores": [[0.9], [0.8, 0.7]],
            "classes": [[0], [1, 2]], "image_id": [1, 2], "class_logits": logits, "probs": [[[0.9, 0.05, 0.03]], [[0.1, 0.8, 0.05], [0.1, 0.1, 0.7]]],
            "vars": [[[1.0]], [[1.0], [1.0]]]}


def test_a_prediction_file_without_logits_is_refused_by_name(tmp_path):
    from proben_amd import calibration as C
    from proben_amd.cli import fit_temperature
    from proben_amd.late_fusion import late_fusion, write_j1
    empty = _j1([[[]], [[], []]])        # what predictions_to_j1 writes for a detector that did not output logits
    with pytest.raises(ValueError, match=r"out/val_thermal_only_predictions\.json: no class_logits"):
        C.require_logits(empty, "out/val_thermal_only_predictions.json")
    C.require_logits(_j1([[[1.0, 0, 0, 0]], [[0, 1.0, 0, 0], [0, 0, 1.0, 0]]]), "x")
    with pytest.raises(ValueError, match=r"second\.json: no class_logits"):
        late_fusion([_j1([[[1.0, 0, 0, 0]], [[0, 1.0, 0, 0], [0, 0, 1.0, 0]]]), empty], ["probEn", "v-avg"], temperatures=[1.0, 2.0],
                    names=["first.json", "second.json"])
    # the fit driver refuses it before it needs the device
    (tmp_path / "val").mkdir()
    json.dump({"images": [{"id": 1, "file_name": "a.jpeg", "height": 10, "width": 10}, {"id": 2, "file_name": "b.jpeg", "height": 10, "width": 10}],
               "annotations": [], "categories": [{"id": 1, "name": "person"}]}, open(tmp_path / "val" / "FLIR_thermal_RGBT_pairs_val.json", "w"))
    f = tmp_path / "val_thermal_only_predictions.json"
    write_j1(f, empty)
    with pytest.raises(ValueError, match=r"val_thermal_only_predictions\.json: no class_logits"):
        fit_temperature.main(["--predictions", str(f), "--dataset_path", str(tmp_path / "val"), "--out", str(tmp_path / "c.json"), "--holdout", "1.0"])
    assert fit_temperature.detector_name(str(f)) == "thermal_only"


def test_fusion_refuses_infos_without_logits():
    from proben_amd import fusion as F
    d = {"img_name": "a", "bbox": [[0, 0, 5, 5]], "score": [0.9], "class": [0], "prob": [[0.9, 0.05, 0.03]], "vars": [[1.0]]}
    with pytest.raises(ValueError, match="info_1 .* carries no class_logits"):
        F.fusion(["probEn", "v-avg"], d, d, temperatures=[1.0, 1.0])
    with pytest.raises(ValueError, match="3 temperatures for 2"):
        F.fusion(["probEn", "v-avg"], d, d, temperatures=[1.0, 1.0, 1.0])
