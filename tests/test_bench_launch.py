"""bench.py's multi-rank entry (`--gpus N` must launch N ranks itself and never report an N-GPU line from
fewer devices).  Replaces what detectron2/engine/launch.py:24-84 does for the reference."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_launch_command_is_one_process_per_gpu_over_loopback():
    import bench
    cmd = bench.launch_command(["--gpus", "4", "--steps", "7"], 4, 12345)
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "12345"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"] and cmd[-5].endswith("bench.py")


def test_no_self_launch_when_already_under_a_launcher(monkeypatch):
    import bench
    monkeypatch.setenv("WORLD_SIZE", "2")
    called = []
    monkeypatch.setattr(bench.subprocess, "call", lambda *a, **k: called.append(a) or 0)
    bench.maybe_self_launch(bench.parse(["--gpus", "2"]), ["--gpus", "2"])   # returns: the ranks already exist
    bench.maybe_self_launch(bench.parse(["--gpus", "1"]), [])
    assert not called


def test_refuses_more_gpus_than_visible(monkeypatch):
    """CPU container: 0 devices visible -> `--gpus 2` exits with a message instead of measuring one device."""
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.maybe_self_launch(bench.parse(["--gpus", "64"]), ["--gpus", "64"])
    assert "only" in str(e.value) and "64" in str(e.value)


@pytest.mark.gpu
def test_bench_two_ranks_over_rccl():
    """`python bench.py --gpus 2` spawns two ranks, RCCL all-gathers the fused rows every step, and the line says
    n_gpus 2 (skipped on a 1-GPU box; there the refusal path is checked instead)."""
    import torch
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    args = ["--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "4", "--depth", "50", "--no-cpu-baseline", "--no-roofline", "--no-micro"]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=900)
    if torch.cuda.device_count() < 2:
        assert p.returncode != 0 and ("only %d GPU" % torch.cuda.device_count()) in (p.stderr + p.stdout)
        pytest.skip("one GPU visible: multi-rank launch not exercised (refusal path checked)")
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    assert "all_gather" in line["config"]["collective"]


def test_plain_run_is_the_default_and_layers_needs_full(capsys):
    """A plain `bench.py --steps N --warmup W` measures the headline only; the other legs and the per-launch table are behind --full."""
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.dump_outputs == "" and a.steps == 3 and a.warmup == 1
    assert bench.parse(["--full", "--layers", "x.txt"]).full
    with pytest.raises(SystemExit):
        bench.parse(["--layers", "x.txt"])
    assert "--full" in capsys.readouterr().err


def _fake_step(B=3, D=5, K=3, S=10):
    import torch
    g = torch.Generator().manual_seed(0)
    dets = []
    for cnt in ([2, 0, 5], [1, 4, 3]):
        dets.append({"boxes": torch.rand(B, D, 4, generator=g), "scores": torch.rand(B, D, generator=g),
                     "classes": torch.randint(0, K, (B, D), generator=g, dtype=torch.int32),
                     "class_logits": torch.rand(B, D, K + 1, generator=g), "prob_score": torch.rand(B, D, K, generator=g),
                     "vars": torch.rand(B, D, generator=g), "rows": torch.zeros(B, D, dtype=torch.int32),
                     "counts": torch.tensor(cnt, dtype=torch.int32)})
    fused = {"boxes": torch.rand(B * S, 4, generator=g, dtype=torch.float64), "scores": torch.rand(B * S, generator=g),
             "classes": torch.randint(0, K, (B * S,), generator=g).float(), "counts": torch.tensor([3, 0, 6], dtype=torch.int32),
             "offsets": torch.arange(B, dtype=torch.int32) * S, "stride": S, "keep": torch.zeros(B * S, dtype=torch.int32)}
    return dets, fused


def test_dump_outputs_writes_the_valid_rows_as_float(tmp_path):
    import numpy as np
    import bench
    dets, fused = _fake_step()
    shapes = bench.dump_outputs(dets, fused, str(tmp_path / "out"))
    names = {f[:-4] for f in os.listdir(tmp_path / "out")}
    assert names == set(shapes) and "images" not in names
    for i, d in enumerate(dets):
        cnt = d["counts"].numpy()
        assert np.array_equal(np.load(tmp_path / "out" / f"det{i}_counts.npy"), cnt)
        for k in ("boxes", "scores", "classes", "class_logits", "prob_score", "vars"):
            v = np.load(tmp_path / "out" / f"det{i}_{k}.npy")
            assert v.dtype in (np.float32, np.float64) and v.shape == tuple(d[k].shape)
            for b, c in enumerate(cnt):
                assert np.array_equal(v[b, :c], d[k][b, :c].numpy().astype(v.dtype)) and not v[b, c:].any()
    fb = np.load(tmp_path / "out" / "fused_boxes.npy")
    assert fb.dtype == np.float64 and fb.shape == (3, 10, 4)
    for b, c in enumerate(fused["counts"].tolist()):
        o = int(fused["offsets"][b])
        assert np.array_equal(fb[b, :c], fused["boxes"][o:o + c].numpy()) and not fb[b, c:].any()
    assert np.load(tmp_path / "out" / "fused_scores.npy").dtype == np.float32


def test_dump_outputs_samples_images_above_the_size_cap(tmp_path):
    import numpy as np
    import bench
    dets, fused = _fake_step()
    full = bench.dump_outputs(dets, fused, str(tmp_path / "a"))
    total = sum(np.load(tmp_path / "a" / (k + ".npy")).nbytes for k in full)
    bench.dump_outputs(dets, fused, str(tmp_path / "b"), max_bytes=total // 2)
    keep = np.load(tmp_path / "b" / "images.npy").astype(int)
    assert 0 < len(keep) < 3
    v = np.load(tmp_path / "b" / "det0_boxes.npy")
    assert np.array_equal(v, np.load(tmp_path / "a" / "det0_boxes.npy")[keep])
    bench.dump_outputs(dets, fused, str(tmp_path / "c"), max_bytes=total // 2)
    assert np.array_equal(np.load(tmp_path / "c" / "images.npy"), keep.astype(np.float64))


def _bench_line(args, timeout=900):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_last_step(tmp_path):
    """A plain run prints the headline line only (no power / roofline / micro / CPU legs) and --dump-outputs writes the last timed step."""
    import numpy as np
    out = tmp_path / "dump"
    line = _bench_line(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--depth", "50", "--dump-outputs", str(out)])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line
    assert not {"power", "sclk_mhz_windows", "roofline", "proben_micro", "cpu_baseline"} & set(line)
    fc = np.load(out / "fused_counts.npy")
    assert fc.shape == (4,) and abs(float(fc.mean()) - line["config"]["fused_rows_per_pair_mean"]) < 0.051
    for f in os.listdir(out):
        v = np.load(out / f)
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), f
    assert np.load(out / "det0_boxes.npy").shape[:1] == (4,) and (np.load(out / "det1_counts.npy") > 0).any()


@pytest.mark.gpu
def test_bench_full_run_keeps_the_other_legs():
    """--full still measures what moved out of the plain run: roofline, ProbEn micro-figure, CPU baseline (power where rocm-smi answers)."""
    line = _bench_line(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--depth", "50", "--full", "--cpu-pairs", "1",
                        "--cpu-threads", "4"])
    assert line["roofline"]["achieved"] > 0 and line["proben_micro"]["ms_per_launch"] > 0
    assert line["cpu_baseline"]["value"] > 0 and "power" in line
