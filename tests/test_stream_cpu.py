"""Streaming FLIR frame-pair loader (proben_amd.stream) and the argument checks of pe_fusion_input_pack - no GPU needed."""
import ctypes
import json

import numpy as np
import pytest


def _write_flir(root, n, H=48, W=64, rgb_hw=(72, 96), odd=()):
    """FLIR val layout with n pairs; pairs whose index is in `odd` get a thermal frame 8 rows taller (a size change)."""
    from PIL import Image
    rng = np.random.default_rng(7)
    (root / "thermal_8_bit").mkdir(parents=True)
    (root / "RGB").mkdir()
    images = []
    for i in range(n):
        stem = f"FLIR_{i:05d}"
        h = H + (8 if i in odd else 0)
        Image.fromarray(rng.integers(0, 255, (h, W, 3), dtype=np.uint8)).save(root / "thermal_8_bit" / (stem + ".jpeg"), quality=95)
        Image.fromarray(rng.integers(0, 255, rgb_hw + (3,), dtype=np.uint8)).save(root / "RGB" / (stem + ".jpg"), quality=95)
        images.append({"id": 100 + i, "file_name": f"thermal_8_bit/{stem}.jpeg", "height": h, "width": W})
    json.dump({"images": images, "annotations": [], "categories": [{"id": 1, "name": "person"}]},
              open(root / "FLIR_thermal_RGBT_pairs_val.json", "w"))
    return root


def _collect(loader):
    out = []
    for b in loader:
        out.append((list(b.ids), list(b.names), tuple(b.hw), b.thermal.numpy().copy(),
                    None if b.rgb is None else b.rgb.numpy().copy()))
    return out


def test_loader_order_content_and_rank_shards(tmp_path):
    from proben_amd.data import read_image
    from proben_amd.stream import FlirPairLoader
    root = _write_flir(tmp_path / "val", 7)
    whole = _collect(FlirPairLoader(str(root), batch=3, workers=0, pin=False))
    assert [len(b[0]) for b in whole] == [3, 3, 1]
    ids = [i for b in whole for i in b[0]]
    assert ids == [100 + i for i in range(7)]
    k = 0
    for bid, names, hw, th, rgb in whole:
        assert hw == (48, 64) and th.shape[1:] == (48, 64, 3) and rgb.shape[1:] == (72, 96, 3)
        for j, name in enumerate(names):
            assert name == f"FLIR_{k:05d}.jpeg"
            np.testing.assert_array_equal(th[j], read_image(str(root / "thermal_8_bit" / name), "BGR"))
            np.testing.assert_array_equal(rgb[j], read_image(str(root / "RGB" / f"FLIR_{k:05d}.jpg"), "BGR"))
            k += 1
    for W in (2, 3):
        parts = [_collect(FlirPairLoader(str(root), batch=3, workers=0, pin=False, rank=r, world=W)) for r in range(W)]
        got = [i for p in parts for b in p for i in b[0]]
        assert got == ids
        th = np.concatenate([b[3] for p in parts for b in p])
        np.testing.assert_array_equal(th, np.concatenate([b[3] for b in whole]))


def test_size_change_splits_a_batch_and_rgb_is_optional(tmp_path):
    from proben_amd.stream import FlirPairLoader
    root = _write_flir(tmp_path / "val", 6, odd=(2,))
    got = _collect(FlirPairLoader(str(root), batch=4, need_rgb=False, workers=0, pin=False))
    assert [b[0] for b in got] == [[100, 101], [102], [103, 104, 105]]
    assert [b[2] for b in got] == [(48, 64), (56, 64), (48, 64)]
    assert all(b[4] is None for b in got)


def test_workers_match_inline_decode_and_never_open_the_gpu(tmp_path):
    from proben_amd.stream import FlirPairLoader
    root = _write_flir(tmp_path / "val", 9, odd=(4,))
    inline = _collect(FlirPairLoader(str(root), batch=3, workers=0, pin=False))
    pooled = FlirPairLoader(str(root), batch=3, workers=3, prefetch=4, pin=False)
    par = _collect(pooled)
    assert len(inline) == len(par)
    for a, b in zip(inline, par):
        assert a[:3] == b[:3]
        np.testing.assert_array_equal(a[3], b[3])
        np.testing.assert_array_equal(a[4], b[4])
    probes = pooled.probe_workers()
    assert len(probes) == 3 and all(not cuda for _, cuda in probes)
    assert len({pid for pid, _ in probes}) == 3


def test_oversized_frames_and_worker_cap(tmp_path):
    from PIL import Image
    from proben_amd.data import read_image
    from proben_amd.stream import MAX_WORKERS, FlirPairLoader, check_workers
    root = _write_flir(tmp_path / "val", 4)
    big = np.random.default_rng(1).integers(0, 255, (90, 120, 3), dtype=np.uint8)
    Image.fromarray(big).save(root / "RGB" / "FLIR_00002.jpg", quality=95)
    got = _collect(FlirPairLoader(str(root), batch=4, workers=2, prefetch=2, pin=False))
    assert [b[0] for b in got] == [[100, 101], [102], [103]]     # the RGB size change closes the batch too
    np.testing.assert_array_equal(got[1][4][0], read_image(str(root / "RGB" / "FLIR_00002.jpg"), "BGR"))
    assert MAX_WORKERS == 15 and check_workers(None) == 4 and check_workers(15) == 15 and check_workers(0) == 0
    for bad in (16, -1):
        with pytest.raises(ValueError, match="--workers"):
            check_workers(bad)
    with pytest.raises(ValueError, match="--workers"):
        FlirPairLoader(str(root), batch=2, workers=64, pin=False)


def test_fusion_input_pack_argument_checks_answer_before_any_device_work():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()
    m = (ctypes.c_float * 4)(1, 2, 3, 4)
    s = (ctypes.c_float * 4)(1, 1, 1, 1)
    p = 4096

    def call(th=p, rgb=p, n=2, th_hw=(512, 640), rgb_hw=(1600, 1800), ch0=0, nch=4, dst=(800, 1000), pad=(800, 1024), mult=32,
             mean=m, std=s, out=p):
        return L.pe_fusion_input_pack(th, rgb, n, th_hw[0], th_hw[1], rgb_hw[0], rgb_hw[1], ch0, nch, dst[0], dst[1], pad[0], pad[1],
                                      mult, mean, std, out, None)
    assert call(th=None) != 0 and "null pointer" in err()
    assert call(out=None) != 0 and "null pointer" in err()
    assert call(mean=None) != 0 and "null pointer" in err()
    assert call(rgb=None) != 0 and "RGB batch" in err()
    assert call(nch=5) != 0 and "channel window" in err()
    assert call(ch0=3, nch=4) != 0 and "channel window" in err()
    assert call(ch0=-1) != 0 and "channel window" in err()
    assert call(n=0) != 0 and "num_images" in err()
    assert call(th_hw=(0, 640)) != 0 and "frame sizes" in err()
    assert call(rgb_hw=(1600, 0)) != 0 and "frame sizes" in err()
    assert call(dst=(801, 1000)) != 0 and "bad sizes" in err()
    assert call(pad=(800, 1040)) != 0 and "multiple of 32" in err()
    assert call(pad=(832, 1024)) != 0 and "multiple of 32" in err()
    assert call(mult=0) != 0 and "multiple of 0" in err()
