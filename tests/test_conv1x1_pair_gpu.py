"""csrc/conv1x1_pair.hip against the two launches it replaces: conv3 + identity + ReLU on conv1x1_ring_kernel (residual mode 1) followed
by the next block's conv1 + ReLU on conv_igemm2_kernel<128, 128>, on the same tensors.  Both outputs are compared bit for bit (as int16):
the fused launch claims the same MFMA, the same k-slots, ascending K from zeroed fp32 accumulators, the ring kernel's epilogue order and
an fp16 hand-over between the products.  Shapes are the smallest at which its 64-pixel tiling can go wrong, and - the kernel is persistent,
one workgroup per CU - the smallest at which a workgroup walks a second and a third tile: only there do the second LDS stage, the prefetch
of the next tile, the re-use of a slot that held an output patch and the waits between them run at all.  Channels are res3's, the only
instantiation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CIN, CY, CN = 128, 512, 128
SHAPES = [(1, 3, 5),       # 15 pixels: one partial tile, less than one 32-pixel MFMA block
          (2, 5, 13),      # 130 pixels: crosses the 64- and 128-pixel tile boundaries, an image boundary inside a tile
          (1, 16, 16),     # 256 pixels: exact multiple
          (2, 100, 131),   # 26 200 pixels = 410 tiles on 256 CUs: workgroups of one and of two tiles, both LDS stages, the last tile partial
          (4, 100, 131)]   # 52 400 pixels = 819 tiles: three and four tiles per workgroup, every slot re-used after it held a patch
KINDS = ["randn", "ints", "cancel", "nonfinite"]
NAN, INF = float("nan"), float("inf")


def tile_rank(pixel, M, cus):
    """Position of the pixel's 64-pixel tile within its workgroup's run (0 = the run's first tile): the split of pe_conv1x1_pair_f16."""
    tiles = -(-M // 64)
    G = min(tiles, cus)
    t = pixel // 64
    wg = next(w for w in range(G) if w * tiles // G <= t < (w + 1) * tiles // G)
    return t - wg * tiles // G


def operands(kind, shape):
    """(t2, w3, b3, res, w1, b1) on the host.  ints: every product and sum is an integer below 2^24, so any summation order gives the same
    fp32 number and a mismatch is an indexing error.  cancel: along K the terms alternate in sign at about 2^10 times the size of their sum,
    so another K order or k-slot assignment changes the rounding of nearly every output."""
    N, H, W = shape
    M = N * H * W
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + M)
    rn = lambda *s: torch.randn(*s, generator=g)
    if kind == "ints":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        t2, w3, b3, res = ri(-3, 3, M, CIN), ri(-2, 2, CY, CIN), ri(-8, 8, CY), ri(-16, 16, M, CY)
        w1, b1 = ri(-2, 2, CN, CY), ri(-8, 8, CN)
    elif kind == "cancel":
        alt = lambda K: torch.where(torch.arange(K) % 2 == 0, 1.0, -1.0)
        t2 = alt(CIN) * 64.0 * (1.0 + rn(M, CIN) / 1024.0)
        w3 = 4.0 * (1.0 + rn(CY, CIN) / 1024.0)
        b3, res = rn(CY), rn(M, CY) + 2.0
        w1 = alt(CY) * 16.0 * (1.0 + rn(CN, CY) / 1024.0)
        b1 = rn(CN)
    else:
        t2, w3, b3, res = rn(M, CIN), rn(CY, CIN) / 8.0, rn(CY), rn(M, CY)
        w1, b1 = rn(CN, CY) / 16.0, rn(CN)
    t2, res = t2.half().view(N, H, W, CIN), res.half().view(N, H, W, CY)
    if kind == "nonfinite":
        # single (pixel, channel) positions, the launch's last pixel - the last valid row of a partial tile, next to its zero-fetched
        # neighbours - among them
        f2, fr = t2.view(M, CIN), res.view(M, CY)
        f2[M - 1, 5], f2[M // 2, 127], f2[0, 64] = NAN, INF, -INF
        fr[M - 1, 300], fr[1, 0], fr[M // 3, 511] = INF, NAN, -INF
        if M > 16384:      # ... and in tiles that are the second / third of their workgroup (asserted by the test for the device's CU count)
            f2[150, 17], fr[64 * 1 + 36, 200] = INF, NAN
    return t2, w3.half().view(CY, 1, 1, CIN), b3.float(), res, w1.half().view(CN, 1, 1, CY), b1.float()


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_launch_gives_the_bits_of_ring_conv3_then_igemm2_conv1(shape, kind):
    import proben_amd  # noqa: F401
    from proben_amd import layers as L
    N, H, W = shape
    M = N * H * W
    t2, w3, b3, res, w1, b1 = [t.cuda() for t in operands(kind, shape)]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if M > 16384:
        ranks = sorted({tile_rank(px, M, cus) for px in range(0, M, 64)})
        assert ranks[:2] == [0, 1] and (M < 50000 or len(ranks) >= 3), ranks      # workgroups really walk a second (and a third) tile
        if kind == "nonfinite":
            assert tile_rank(150, M, cus) >= 1 and tile_rank(M - 1, M, cus) >= 1 and max(tile_rank(150, M, cus), tile_rank(100, M, cus)) >= (2 if M > 50000 else 1)
    # the two-launch path under the default policy is the pair the issue names
    assert L.conv_variant_name(M, CY, 1, CIN, residual_mode=1) == "conv1x1_ring_kernel"
    assert L.conv_variant_name(M, CN, 1, CY) == "conv_igemm2_kernel<128, 128, 0, 1>"
    y_ref = L.conv2d_nhwc(t2, w3, b3, kernel=1, relu=True, residual=res, residual_mode=1)
    t1_ref = L.conv2d_nhwc(y_ref, w1, b1, kernel=1, relu=True)
    # outputs pre-filled: a row the launch does not write shows
    y = torch.full((N, H, W, CY), 7.0, dtype=torch.float16, device="cuda")
    t1 = torch.full((N, H, W, CN), 7.0, dtype=torch.float16, device="cuda")
    L.conv1x1_pair(t2, w3, b3, res, w1, b1, out=y, t1_next=t1)
    torch.cuda.synchronize()
    yr, tr = y_ref.float().cpu().numpy(), t1_ref.float().cpu().numpy()
    if kind == "nonfinite":
        assert np.isnan(yr).sum() >= 2 and np.isinf(yr).sum() >= 1 and not np.isfinite(tr).all()
        assert (~np.isfinite(yr.reshape(M, CY))).any(1).sum() <= 8      # a planted value reaches its own pixel only
    else:
        assert np.isfinite(yr).all() and np.isfinite(tr).all()
        assert (yr > 0).mean() > 0.05 and (tr > 0).mean() > 0.05, "the ReLUs leave something to compare"
    if not torch.equal(y.view(torch.int16), y_ref.view(torch.int16)):      # (the host comparison only for its report)
        np.testing.assert_array_equal(bits(y), bits(y_ref), err_msg="y")
    if not torch.equal(t1.view(torch.int16), t1_ref.view(torch.int16)):
        np.testing.assert_array_equal(bits(t1), bits(t1_ref), err_msg="t1'")


def test_detector_outputs_do_not_depend_on_pair_fusion_or_batch():
    """R50, synthetic weights: every output of forward_batch is bit-identical with and without the fused res3 launches, for one 96 x 128
    frame and for a batch of 3, and image 0's rows are the same in both batch sizes."""
    import proben_amd  # noqa: F401
    from proben_amd import layers as L
    from proben_amd.rcnn import DetectorConfig, GeneralizedRCNN
    from proben_amd.synthetic import synthetic_images, synthetic_state_dict
    model = GeneralizedRCNN(DetectorConfig(), synthetic_state_dict(50, 3, 3, seed=1))
    assert model.fuse_pairs is True
    frames = torch.from_numpy(synthetic_images(3, 96, 128, seed=7)).cuda()
    rows = ("boxes", "scores", "classes", "class_logits", "prob_score", "vars")      # valid up to counts[i]; the padding behind is not defined
    props = ("proposals", "proposal_logits")                                          # ... up to proposal_counts[i]
    same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    got = {}
    for n in (1, 3):
        for fuse in (True, False):
            model.fuse_pairs = fuse
            L.PROFILE = []
            try:
                got[n, fuse] = model.forward_batch(frames[:n], out_sizes=[(96, 128)] * n)
                names = [r["variant"] for r in L.PROFILE]
            finally:
                L.PROFILE = None
            assert names.count("conv1x1_pair_kernel") == (3 if fuse else 0), names      # res3's blocks 0->1, 1->2, 2->3
        a, b = got[n, True], got[n, False]
        tensors = {k for k, v in a.items() if isinstance(v, torch.Tensor)}
        assert tensors == set(rows) | set(props) | {"rows", "counts", "proposal_counts", "cand_total"}, tensors      # every output is compared below
        for k in ("counts", "proposal_counts", "cand_total"):
            assert same(a[k], b[k]), (n, k)
        assert a["image_sizes"] == b["image_sizes"] and a["out_sizes"] == b["out_sizes"]
        for i in range(n):
            c, pc = int(a["counts"][i]), int(a["proposal_counts"][i])
            assert pc > 0
            for k in rows + ("rows",):
                assert same(a[k][i, :c], b[k][i, :c]), (n, i, k)
            for k in props:
                assert same(a[k][i, :pc], b[k][i, :pc]), (n, i, k)
    one, three = got[1, True], got[3, True]
    c, pc = int(one["counts"][0]), int(one["proposal_counts"][0])
    assert c == int(three["counts"][0]) and pc == int(three["proposal_counts"][0])
    for k in rows:
        assert same(one[k][0, :c], three[k][0, :c]), k
    for k in props:
        assert same(one[k][0, :pc], three[k][0, :pc]), k
