"""The fused detection as a full prediction (pe_proben_fuse_batch_posterior, fuse_batch(with_posterior=True), late_fusion.fused_to_j1,
demo_probEn --write_fused, calibration_report --fused-posterior): what can be checked without a GPU.  The np.longdouble restatement
the GPU tests (tests/test_posterior_gpu.py) compare the kernel against is tests/fuse_ref.py."""
import numpy as np
import pytest
import torch


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_flags_and_keywords_are_refused_outside_proben_log():
    from proben_amd import fusion as F
    from proben_amd.cli import calibration_report
    from proben_amd.late_fusion import late_fusion
    from proben_amd.opt import config_parser
    from proben_amd.pipeline import FramePairPipeline
    for mode in ("probEn", "avg", "max"):
        with pytest.raises(SystemExit):
            config_parser(["--write_fused", "fused.json", "--score_fusion", mode])
    with pytest.raises(SystemExit):
        config_parser(["--write_fused", "fused.json"])                  # the default score fusion is probEn
    assert config_parser(["--write_fused", "fused.json", "--score_fusion", "probEn-log"]).write_fused == "fused.json"
    assert config_parser([]).write_fused is None
    z = torch.zeros((0, 4), dtype=torch.float64)
    msg = "with_posterior belongs to score_fusion 'probEn-log'"
    for mode in ("probEn", "avg", "max", "probEn_binary"):
        with pytest.raises(ValueError, match=msg):
            F.fuse_batch(z, z[:, 0], z[:, :3], z[:, 0], z[:, 0].int(), torch.zeros(1, dtype=torch.int32), score_fusion=mode, with_posterior=True)
        with pytest.raises(ValueError, match=msg):
            F.fuse_detections([], mode, with_posterior=True)
        with pytest.raises(ValueError, match=msg):
            late_fusion([], [mode, "v-avg"], with_posterior=True)
        with pytest.raises(ValueError, match=msg):
            FramePairPipeline([], mode, with_posterior=True)
    rep = ["--predictions", "a.json", "b.json", "--dataset_path", "d", "--calibration", "c.json", "--fused-posterior"]
    with pytest.raises(SystemExit):
        calibration_report.parse(rep)                                   # --score_fusion defaults to probEn
    assert calibration_report.parse(rep + ["--score_fusion", "probEn-log"]).fused_posterior
    assert not calibration_report.parse(rep[:-1]).fused_posterior


def test_argument_checks_answer_without_a_gpu():
    """pe_proben_fuse_batch_posterior checks its arguments before any device work and explains itself through pe_last_error()."""
    import __graft_entry__ as g
    g.build()
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()  # noqa: E731
    P = 4096      # a non-null pointer that is never dereferenced
    who = "pe_proben_fuse_batch_posterior"

    def fuse(row_source=P, weights=P, nd=2, K=3, boxes=P, lq=P, var=P, mem=P, box_mode=0, rows=64, counts=P):
        return L.pe_proben_fuse_batch_posterior(boxes, P, P, P, P, row_source, P, None, None, 1, K, rows, box_mode, 0.5, 640.0, 512.0, None,
                                                weights, nd, P, P, P, P, counts, None, lq, var, mem, None)
    assert fuse(boxes=None) == -1 and f"{who}: null input pointer" in err()
    assert fuse(counts=None) == -1 and f"{who}: null output pointer" in err()
    assert fuse(row_source=None) == -1 and "row_source and pool_weights go together" in err()
    assert fuse(weights=None) == -1 and "row_source and pool_weights go together" in err()
    for kw in ({"lq": None}, {"var": None}, {"mem": None}):
        assert fuse(**kw) == -1 and "out_log_posterior / out_vars / out_members" in err()
    assert fuse(nd=0) == -1 and "num_detectors 0 not in [1,8]" in err()
    assert fuse(nd=9) == -1 and "num_detectors 9 not in [1,8]" in err()
    assert fuse(K=63) == -1 and "num_classes 63 not in [1,62]" in err()
    assert fuse(K=63, row_source=None, weights=None, nd=0) == -1 and "num_classes 63 not in [1,62]" in err()
    assert fuse(box_mode=4) == -1 and "bad box_mode 4" in err()
    assert fuse(rows=0) == -1 and "max_rows_per_image 0 not in [1,2048]" in err()
    assert fuse(rows=2000) == -2 and "LDS" in err()
    assert L.pe_proben_fuse_batch_posterior(None, None, None, None, None, None, None, None, None, 0, 3, 64, 0, 0.5, 640.0, 512.0, None, None, 0,
                                            None, None, None, None, None, None, None, None, None, None) == 0         # no image: nothing to do


# ---- fused_to_j1 ------------------------------------------------------------------------------------------------------------------

def test_fused_to_j1_on_hand_made_rows():
    from proben_amd.late_fusion import J1_KEYS, fused_to_j1
    dets = [{"image": ["a0", "a1", "a2"], "image_id": [10, 11, 12]}, {"image": ["b0", "b1", "b2"], "image_id": [20, 21, 22]}]
    lq0 = np.log(np.array([[0.7, 0.1, 0.1, 0.1], [0.05, 0.05, 0.1, 0.8], [0.2, 0.5, 0.2, 0.1]]))
    img0 = (np.array([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0], [9.5, 10.5, 11.5, 12.5]]), torch.tensor([0.7, 0.8, 0.5]), torch.tensor([0.0, 3.0, 1.0]),
            lq0, np.array([0.25, 1.5, 2.0]), np.array([2, 3, 1], np.int32))
    img2 = (np.zeros((0, 4)), torch.zeros(0), torch.zeros(0), np.zeros((0, 4)), np.zeros(0), np.zeros(0, np.int32))
    j1, dropped = fused_to_j1(dets, [img0, None, img2])
    assert dropped == 1                                                  # img0's second row is background (class K = 3)
    assert list(j1) == J1_KEYS
    assert j1["image"] == ["b0", "b1", "b2"] and j1["image_id"] == [20, 21, 22]          # dets[1]'s, as the driver pairs them
    assert j1["boxes"] == [[[1.0, 2.0, 3.0, 4.0], [9.5, 10.5, 11.5, 12.5]], [], []]
    assert j1["scores"] == [[float(np.float32(0.7)), 0.5], [], []]
    assert j1["classes"] == [[0, 1], [], []] and all(isinstance(c, int) for c in j1["classes"][0])
    assert j1["class_logits"] == [[lq0[0].tolist(), lq0[2].tolist()], [], []]
    assert j1["probs"] == [[np.exp(lq0[0, :3]).tolist(), np.exp(lq0[2, :3]).tolist()], [], []]
    assert j1["vars"] == [[[0.25], [2.0]], [], []]
    # the file is a valid probEn-log input at T = 1: softmax(class_logits / 1) is the posterior it carries
    lg = np.asarray(j1["class_logits"][0])
    sm = np.exp(lg - lg.max(1, keepdims=True))
    np.testing.assert_allclose(sm / sm.sum(1, keepdims=True), np.exp(lq0[[0, 2]]), rtol=1e-15)
    import json
    assert json.loads(json.dumps(j1)) == j1
    with pytest.raises(ValueError, match="carry no posterior"):
        fused_to_j1(dets, [img0[:3], None, None])
