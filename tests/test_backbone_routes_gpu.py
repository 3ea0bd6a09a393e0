"""Which kernel takes every convolution of a forward: an R50 with synthetic weights, batch 1, at the two frame sizes and all 16 settings
of use_wd / fuse_tails / fuse_pairs / fuse_res2 of tests/golden/gen_backbone_routes.py, against the list recorded before the routes
moved from per-forward name lookups to the block records of weights.PackedDetector.  The list is layers.PROFILE's
(variant, shape) per launch, in launch order: a block that takes another route, a route that loses its turn in chain > pair > tail >
plain, or a record whose label changes, shows as a differing line."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import gen_backbone_routes as G  # noqa: E402

# one line of every route the all-on 64 x 512 forward must take (feature widths 128, 64, 32, 16 for res2 .. res5)
EVERY_ROUTE = {
    "res2 as the 64-wide chain": "bneck64_kernel<1, 1> | N1 16x128 64->64->256+sc->64 f320",
    "res3 pair": "conv1x1_pair_kernel | N1 8x64 128->512+id->128 f320",
    "res4 fused tail": "conv3x3_wd_kernel<1, 4, 4, 4, 0, 2> | N1 4x32 Cin256 Cout256->1024 k3+k1 s1 res1 f320",
    "res5 plain 3x3": "conv3x3rb_kernel<128, 128> | N1 2x16 Cin512 Cout512 k3 s1 res0 f320",
    "res5 plain conv3": "conv1x1_ring_kernel | N1 2x16 Cin512 Cout2048 k1 s1 res1 f320",
    "weights-direct 3x3": "conv3x3_wd_kernel<1, 4, 4, 4, 0, 0> | N1 8x64 Cin256 Cout256 k3 s1 res0 f320",
    "fused RPN head": "conv3x3_wd_kernel<1, 4, 4, 4, 0, 1> | N1 4x32 Cin256 Cout256+head k3 s1 res0 f321",
    "two-launch RPN head": "conv_igemm2_kernel<128, 64, 0, 1> | N1 2x16 Cin256 Cout15 k1 s1 res0 f321",
}


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "backbone_routes_r50.json")) as f:
        rec = json.load(f)
    assert set(rec) == {G.case_name(hw, st) for hw in G.FRAMES for st in G.SETTINGS}
    all_on = rec[G.case_name((64, 512), (1, 1, 1, 1))]
    missing = [what for what, line in EVERY_ROUTE.items() if line not in all_on]
    assert not missing, f"the fixture's all-on 64 x 512 forward takes no {missing}"
    # with its switch off a route's kernel is gone, and where the weights-direct rule fails (96 x 128 from res3 on) no tail is fused
    assert not any("bneck64" in line for line in rec[G.case_name((64, 512), (1, 1, 1, 0))])
    assert not any("conv1x1_pair" in line for line in rec[G.case_name((64, 512), (1, 1, 0, 1))])
    assert not any("k3+k1" in line for line in rec[G.case_name((64, 512), (1, 0, 1, 1))])
    assert not any("_wd_kernel" in line or "_wd9_kernel" in line for line in rec[G.case_name((64, 512), (0, 1, 1, 1))])
    assert not any("k3+k1" in line for line in rec[G.case_name((96, 128), (1, 1, 1, 1))])
    return rec


@pytest.fixture(scope="module")
def model():
    return G.make_model()


@pytest.mark.parametrize("setting", G.SETTINGS, ids=lambda s: "".join(map(str, s)))
@pytest.mark.parametrize("hw", G.FRAMES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_every_launch_of_a_forward_is_the_recorded_kernel_on_the_recorded_shape(recorded, model, hw, setting):
    assert G.routes(model, hw, setting) == recorded[G.case_name(hw, setting)]
