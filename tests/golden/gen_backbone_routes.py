"""Generate tests/golden/backbone_routes_r50.json: which kernel took every convolution launch of one forward of an R50 with synthetic
weights, as (variant, shape) of layers.PROFILE's records, for batch 1 at two frame sizes and all 16 settings of the detector's four A/B
switches.  Recorded on the GPU at the commit BEFORE the routes moved from name lookups in GeneralizedRCNN._bottom_up to block records
(DESIGN.md section 22 names it); tests/test_backbone_routes_gpu.py holds the forward to this list.

    python tests/golden/gen_backbone_routes.py [--out FILE]

Only attributes the detector has had since the switch they name are used, so the file runs unchanged on that commit.
  64 x 512   feature widths 128, 64, 32, 16 for res2 .. res5: the 64-wide chain, the res3 pair, the weights-direct 3x3, the fused tail at
             res4 and the plain path at res5 all occur, the fused RPN head on the wide levels only;
  96 x 128   widths 32, 16, 8, 4: the weights-direct rule fails from res3 on."""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

FRAMES = ((64, 512), (96, 128))
SWITCHES = ("use_wd", "fuse_tails", "fuse_pairs", "fuse_res2")
SETTINGS = tuple(itertools.product((1, 0), repeat=len(SWITCHES)))      # all on first


def case_name(hw, setting):
    return f"{hw[0]}x{hw[1]} " + " ".join(f"{s}={v}" for s, v in zip(SWITCHES, setting))


def make_model():
    import proben_amd  # noqa: F401
    from proben_amd.rcnn import DetectorConfig, GeneralizedRCNN
    from proben_amd.synthetic import synthetic_state_dict
    return GeneralizedRCNN(DetectorConfig(), synthetic_state_dict(50, 3, 3, seed=1))


def routes(model, hw, setting):
    """["variant | shape", ...] of one forward_batch of a single hw frame under the setting; the switches are put back."""
    import torch
    from proben_amd import layers as L
    from proben_amd.synthetic import synthetic_images
    frame = torch.from_numpy(synthetic_images(1, hw[0], hw[1], seed=7)).cuda()
    before = [getattr(model, s) for s in SWITCHES]
    L.PROFILE = []
    try:
        for s, v in zip(SWITCHES, setting):
            setattr(model, s, bool(v))
        model.forward_batch(frame, out_sizes=[hw])
        torch.cuda.synchronize()
        return [f"{r['variant']} | {r['shape']}" for r in L.PROFILE]
    finally:
        L.PROFILE = None
        for s, v in zip(SWITCHES, before):
            setattr(model, s, v)


def main():
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "backbone_routes_r50.json")
    model = make_model()
    rec = {case_name(hw, st): routes(model, hw, st) for hw in FRAMES for st in SETTINGS}
    with open(path, "w") as f:
        json.dump(rec, f, indent=0)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes;", {k: len(v) for k, v in rec.items()})


if __name__ == "__main__":
    main()
