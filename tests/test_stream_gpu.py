"""Frame pairs from disk through one-pass ProbEn: the fused fusion-input kernel (pe_fusion_input_pack) against the host build, and
`demo_probEn --one-pass` against the two-stage route (save_predictions per detector -> demo_probEn) and against itself over two
ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from fuse_inputs import weights, write_flir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    import argparse
    import proben_amd
    from proben_amd.cli.save_predictions import build_cfg
    tmp = tmp_path_factory.mktemp("w")
    out = {}
    for seed, m in enumerate(("early_fusion", "middle_fusion"), 1):
        out[m] = proben_amd.DefaultPredictor(build_cfg(argparse.Namespace(fusion_method=m, model_path=weights(tmp, m, seed)))).model
    return out


@pytest.mark.parametrize("th_hw,rgb_hw,resize_to", [
    ((64, 80), (64, 80), "rse"),          # RGB at the thermal size
    ((256, 320), (800, 900), "rse"),      # RGB downscaled to the thermal size
    ((256, 320), (120, 150), "rse"),      # RGB upscaled
    ((255, 321), (301, 397), "rse"),      # odd sizes
    ((96, 128), (150, 170), None),        # no ResizeShortestEdge (resized size == thermal size)
    ((512, 640), (300, 400), (160, 200)), # strong down-resize: the tiles' windows exceed the LDS, per-pixel form
])
@pytest.mark.parametrize("method", ["early_fusion", "middle_fusion"])
def test_fusion_input_pack_is_bit_identical_to_the_host_build(models, method, th_hw, rgb_hw, resize_to):
    from proben_amd.cli.save_predictions import resize_bilinear
    from proben_amd.data import PairFrames, resize_shortest_edge_shape
    model = models[method]
    rng = np.random.default_rng(hash((th_hw, rgb_hw)) % 2 ** 32)
    n = 3
    th = rng.integers(0, 256, (n,) + th_hw + (3,), dtype=np.uint8)
    rgb = rng.integers(0, 256, (n,) + rgb_hw + (3,), dtype=np.uint8)
    host = []
    for i in range(n):           # cli/save_predictions.load_input after decode
        r = resize_bilinear(rgb[i], th_hw)
        host.append(np.concatenate([r, th[i][:, :, :1] if method == "early_fusion" else th[i]], axis=2).astype(np.float64))
    if resize_to == "rse":
        resize_to = resize_shortest_edge_shape(th_hw[0], th_hw[1], model.cfg.min_size_test, model.cfg.max_size_test)
    want, ws = model._preprocess(torch.from_numpy(np.stack(host).astype(np.float32)).cuda(), resize_to)
    got, gs = model._preprocess(PairFrames(torch.from_numpy(th).cuda(), torch.from_numpy(rgb).cuda()), resize_to)
    torch.cuda.synchronize()
    assert gs == ws and len(got) == len(want) == (1 if method == "early_fusion" else 2)
    for g, w in zip(got, want):
        assert g.shape == w.shape
        assert torch.equal(g, w), f"{int((g != w).sum())} of {g.numel()} values differ"


def _run_two_stage(root, tmp, names, paths, tag):
    from proben_amd.cli import demo_probEn, save_predictions
    pdir = tmp / f"two_{tag}"
    for m, p in zip(names, paths):
        save_predictions.main(["--dataset_path", str(root), "--fusion_method", m, "--model_path", p, "--prediction_path", str(pdir),
                               "--batch", "4"])
    out = tmp / f"out2_{tag}"
    res = demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names),
                            "--outfolder", str(out), "--dataset_name", f"flir_two_{tag}"])
    return pdir, out, res


def test_one_pass_equals_two_stages(tmp_path):
    from proben_amd.cli import demo_probEn
    root = tmp_path / "val"
    write_flir(root, 6, 96, 120, (150, 180))
    for tag, names in (("te", ["thermal_only", "early_fusion"]), ("tem", ["thermal_only", "early_fusion", "middle_fusion"])):
        paths = [weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
        pdir2, out2, res2 = _run_two_stage(root, tmp_path, names, paths, tag)
        pdir1, out1 = tmp_path / f"one_{tag}", tmp_path / f"out1_{tag}"
        res1 = demo_probEn.main(["--one-pass", "--dataset_path", str(root), "--detectors", ",".join(names), "--model_paths", ",".join(paths),
                                 "--workers", "2", "--batch", "4", "--write-predictions", "--prediction_path", str(pdir1),
                                 "--outfolder", str(out1), "--dataset_name", f"flir_one_{tag}"])
        for m in names:
            f = f"val_{m}_predictions.json"
            assert (pdir1 / f).read_bytes() == (pdir2 / f).read_bytes(), f
        r1 = json.load(open(out1 / "coco_instances_results.json"))
        r2 = json.load(open(out2 / "coco_instances_results.json"))
        assert len(r1) == len(r2) > 0
        assert [r["image_id"] for r in r1] == [r["image_id"] for r in r2]
        assert [r["category_id"] for r in r1] == [r["category_id"] for r in r2]
        np.testing.assert_allclose([r["score"] for r in r1], [r["score"] for r in r2], rtol=1e-6)
        np.testing.assert_allclose([r["bbox"] for r in r1], [r["bbox"] for r in r2], rtol=1e-6, atol=1e-4)
        for k in ("AP", "AP50", "AP75"):
            assert abs(res1["bbox"][k] - res2["bbox"][k]) <= 1e-6, (k, res1["bbox"][k], res2["bbox"][k])
        st = res1["one_pass"]
        assert st["pairs"] == 6 and st["timed_pairs"] == 2 and st["workers"] == 2
        assert (out1 / "FLIR_probEn_eval.json").exists()


def test_one_pass_refuses_rgb_only(tmp_path):
    from proben_amd.cli import demo_probEn
    root = tmp_path / "val"
    write_flir(root, 2, 64, 80, (64, 80))
    with pytest.raises(ValueError, match="two-stage route"):
        demo_probEn.main(["--one-pass", "--dataset_path", str(root), "--detectors", "rgb_only,thermal_only", "--outfolder", str(tmp_path / "o")])


def test_one_pass_world_size_2_equals_world_size_1(tmp_path):
    from proben_amd import launch
    root = tmp_path / "val"
    write_flir(root, 7, 96, 120, (150, 180))
    names = ["thermal_only", "early_fusion"]
    paths = [weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
    env = launch.launch_env()
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    env["PROBEN_DIST_BACKEND"] = "gloo"        # the two ranks share one device
    got = {}
    for world in (1, 2):
        out = tmp_path / f"w{world}"
        p = subprocess.run([sys.executable, "-m", "proben_amd.cli.demo_probEn", "--one-pass", "--dataset_path", str(root),
                            "--detectors", ",".join(names), "--model_paths", ",".join(paths), "--workers", "2", "--batch", "2",
                            "--outfolder", str(out), "--dataset_name", f"flir_w{world}", "--world-size", str(world)],
                           capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        assert "pairs/s" in p.stdout
        got[world] = ((out / "coco_instances_results.json").read_bytes(), json.load(open(out / "FLIR_probEn_eval.json")))
    assert got[1][0] == got[2][0] and len(json.loads(got[1][0])) > 0
    assert got[1][1] == got[2][1]
