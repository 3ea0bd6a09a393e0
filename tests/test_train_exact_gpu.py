"""The training half bit for bit (tests/train_exact.py has the references, tests/test_train_exact_cpu.py shows that the bit comparison
rejects the errors this module is after): pe_sgd_momentum_f32 through its C ABI and through FusedSGD against the float32 restatement
of its operation order, HipLinear's three GEMM launches on operands whose exact answer does not depend on the summation order, and
the skip and clip paths of box_head_train_step.  No tolerance appears in the SGD and HipLinear comparisons; the clip test has two
margins, both derived in the test from the measured norms."""
import math

import numpy as np
import pytest
import torch

import conv_exact as E
import train_exact as T

pytestmark = pytest.mark.gpu

GUARD = 8                   # elements in front of and behind the n the kernel is given: 32 bytes keep the slice 16-byte aligned


@pytest.fixture(scope="module")
def P():
    import proben_amd  # noqa: F401
    from proben_amd import _lib, layers, training
    from proben_amd.modeling import Box2BoxTransform

    class Namespace:
        pass
    ns = Namespace()
    ns.lib, ns.L, ns.T, ns.Box2BoxTransform = _lib, layers, training, Box2BoxTransform
    return ns


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. fused SGD, by bits
def guarded(values, fill, dtype):
    """[GUARD of fill | values | GUARD of fill] on the device."""
    buf = np.full(len(values) + 2 * GUARD, fill, dtype=dtype)
    buf[GUARD:GUARD + len(values)] = values
    return torch.from_numpy(buf).cuda()


@pytest.mark.parametrize("cfg", T.SGD_CONFIGS, ids=[c.name for c in T.SGD_CONFIGS])
@pytest.mark.parametrize("n", T.SGD_SIZES)
def test_sgd_kernel_reproduces_the_float32_restatement_bit_for_bit(P, n, cfg):
    """The C ABI on slices of flat buffers: vector part, the n % 4 scalar tail (n = 1, 2, 3: the tail alone), more vectors than the
    256 * 16 block cap lets one pass cover (4 194 304 + 1027: the grid-stride loop runs twice, and there is a tail).  Step 0 has
    first_step = 1 over a momentum buffer and a shadow full of NaN - nothing of either may be read -, steps 1 and 2 continue from
    the kernel's own state.  p, m and the shadow carry the restatement's bytes after every step; the guard elements on both sides
    of all four buffers, the gradients and - with a null shadow pointer - the whole shadow buffer keep theirs."""
    p0, _, grads = T.sgd_operands(n, cfg)
    p, m, h = guarded(p0, 123.25, np.float32), guarded(np.full(n, np.nan, np.float32), -7.5, np.float32), guarded(np.full(n, np.nan, np.float16), 3.0, np.float16)
    h_before = host(h).copy()
    want = T.sgd_run(p0, np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float16), grads, cfg)
    inner = slice(GUARD, GUARD + n)
    for s, g_host in enumerate(grads):
        g = guarded(g_host, 11.0, np.float32)
        st = P.lib.lib().pe_sgd_momentum_f32(P.lib.ptr(p[GUARD:]), P.lib.ptr(g[GUARD:]), P.lib.ptr(m[GUARD:]), P.lib.ptr(h[GUARD:]) if cfg.shadow else None,
                                            n, cfg.lr, cfg.mu, cfg.wd, cfg.gs, int(s == 0), P.lib.stream())
        P.lib.check(st, "pe_sgd_momentum_f32")
        torch.cuda.synchronize()
        got = {"p": host(p), "m": host(m), "h": host(h), "g": host(g)}
        wp, wm, wh = want[s]
        assert not np.isnan(got["p"]).any() and not np.isnan(got["m"]).any(), f"step {s}: NaN: the first step read the momentum buffer"
        T.same_bits(got["p"][inner], wp, f"{cfg.name} n={n} step {s}: p")
        T.same_bits(got["m"][inner], wm, f"{cfg.name} n={n} step {s}: m")
        if cfg.shadow:
            T.same_bits(got["h"][inner], wh, f"{cfg.name} n={n} step {s}: shadow")
        else:
            assert got["h"].tobytes() == h_before.tobytes(), "a null shadow pointer, and the shadow buffer changed"
        T.same_bits(got["g"][inner], g_host, "the gradients are read only")
        for key, fill in (("p", 123.25), ("m", -7.5), ("h", 3.0), ("g", 11.0)):
            a = got[key]
            assert a[:GUARD].tobytes() == a[-GUARD:].tobytes() == np.full(GUARD, fill, a.dtype).tobytes(), f"{cfg.name} n={n} step {s}: guard of {key} overwritten"


def test_fused_sgd_groups_and_lr_override_follow_the_restatement_per_run(P):
    """FusedSGD over FlatParams whose tensor sizes are no multiples of 4: a bias group with its own lr factor (1.3: base * factor
    narrowed once is another float than the factors narrowed and multiplied, for every base rate used) and its own weight decay,
    an `lr=` override on the later steps.  Three steps against the restatement applied to every runs() range, by bits; the padding
    elements between the tensors stay zero in master, momentum and shadow."""
    shapes = {"a.weight": (37, 19), "b.weight": (5, 3), "a.bias": (37,), "b.bias": (5,)}
    flat = P.T.FlatParams(shapes, "cuda")
    assert [r[0] for r in flat.runs()] == ["weights", "bias"] and any(math.prod(s) % 4 for s in shapes.values())
    rng = np.random.default_rng(5)
    real = np.zeros(flat.numel, dtype=bool)
    for name in flat.names:
        o, cnt = flat.offsets[name]
        real[o:o + cnt] = True
    fill = lambda: np.where(real, rng.standard_normal(flat.numel, dtype=np.float32), np.float32(0))
    p = fill()
    flat.master.copy_(torch.from_numpy(p))
    flat.refresh_shadow()
    base, mu, wd, factor, wd_bias, gs = 0.02, 0.9, 0.01, 1.3, 0.003, 1.0 / (3 * 1024.0)
    opt = P.T.FusedSGD(flat, lr=base, momentum=mu, weight_decay=wd, bias_lr_factor=factor, weight_decay_bias=wd_bias)
    hyper = {"weights": (1.0, wd), "bias": (factor, wd_bias)}
    m, h = np.zeros_like(p), p.astype(np.float16)
    for s, lr in enumerate([None, 0.03, 0.01]):
        b = base if lr is None else lr
        assert np.float32(b * factor) != np.float32(b) * np.float32(factor)
        g = fill() / np.float32(gs)
        flat.grad.copy_(torch.from_numpy(g))
        opt.step(grad_scale=gs, lr=lr)
        for group, o, cnt in flat.runs():
            r = slice(o, o + cnt)
            f, w = hyper[group]
            p[r], m[r], h[r] = T.sgd_step_f32(p[r], g[r], m[r], h[r], b * f, mu, w, gs, s == 0)
        T.same_bits(host(flat.master), p, f"step {s}: master")
        T.same_bits(host(flat.momentum), m, f"step {s}: momentum")
        T.same_bits(host(flat.shadow), h, f"step {s}: shadow")
        for buf in (flat.master, flat.momentum, flat.shadow):
            pad = host(buf)[~real]
            assert pad.size == 8 and pad.tobytes() == bytes(pad.nbytes), f"step {s}: padding elements are not +0"
    assert opt.steps == 3


# ------------------------------------------------------------------------------------------------ 2. HipLinear on exact operands, by bits
@pytest.mark.parametrize("c", T.LINEAR_CASES, ids=[c.name for c in T.LINEAR_CASES])
def test_hip_linear_forward_and_backward_are_bit_exact_on_grid_operands(P, c):
    """y, x.grad, weight.grad and bias.grad of HipLinear.apply + backward against the float64 reference: the forward launch with its
    bias, dX = dY W without a bias to fp16 and dW = dY^T X without a bias to fp32 over the row count padded to 64, the ReLU mask,
    the transposes and the padding in Python around them.  The kernels asked for are the ones the library routes the three launches
    to, by its own answer for each launch's real arguments (has_bias = False and out_f32 decide the route)."""
    T.linear_conditions(c)
    o, want = T.linear_clean(c)
    name = P.L.conv_variant_name
    rows = c.M + c.pad
    assert name(c.M, c.N, 1, c.K, out_f32=c.out_f32, has_bias=True, in_pixels=c.M) == c.fwd
    assert name(c.M, c.K, 1, c.N, out_f32=False, has_bias=False, in_pixels=c.M) == c.dx
    assert name(c.N, c.K, 1, rows, out_f32=True, has_bias=False, in_pixels=c.N) == c.dw
    x = o["x"].half().cuda().requires_grad_()
    w = o["w"].float().cuda().requires_grad_()
    b = o["b"].float().cuda().requires_grad_()
    y = P.T.HipLinear.apply(x, w, b, w.detach().half(), c.relu, c.out_f32)
    y.backward(o["dy"].to(y.dtype).cuda())
    torch.cuda.synchronize()
    assert y.dtype == (torch.float32 if c.out_f32 else torch.float16)
    assert x.grad.dtype == torch.float16 and w.grad.dtype == torch.float32 and b.grad.dtype == torch.float32
    E.assert_bits(y, want["y"], f"{c.name}: y")
    E.assert_bits(x.grad, want["dx"], f"{c.name}: x.grad")
    E.assert_bits(w.grad, want["dw"], f"{c.name}: weight.grad")
    E.assert_bits(b.grad, want["db"], f"{c.name}: bias.grad")


def test_hip_linear_refuses_an_output_width_that_is_no_multiple_of_64(P):
    """dX reduces over the output width, and the GEMM takes reductions in whole 64-wide steps: a 72-wide layer gets the library's
    argument error from backward, and no gradient comes back."""
    g = torch.Generator().manual_seed(1)
    x = (E.ints(g, (64, 64), 8) / 8).half().cuda().requires_grad_()
    w = (E.ints(g, (72, 64), 8) / 8).float().cuda().requires_grad_()
    b = torch.zeros(72, device="cuda", requires_grad=True)
    with pytest.raises(P.lib.HipLibraryError, match="64"):
        y = P.T.HipLinear.apply(x, w, b, w.detach().half(), False, False)
        y.backward(torch.ones_like(y))
    assert x.grad is None and w.grad is None and b.grad is None


# ------------------------------------------------------------------------------------------------ 3. skip and clip in box_head_train_step
K_CLASSES, R, C, FC = 3, 96, 64, 128


def make_head(P, **sgd):
    head = P.T.BoxHead(49 * C, K_CLASSES, "cuda", fc_dim=FC, seed=5)
    return head, P.T.FusedSGD(head.flat, **sgd)


def batch(P):
    pooled, prop, gt, cls = (t.cuda() for t in T.box_batch(R, C, K_CLASSES))
    return pooled, prop, gt, cls, P.Box2BoxTransform(weights=(10.0, 10.0, 5.0, 5.0))


def state(flat):
    return {k: getattr(flat, k).clone() for k in ("master", "momentum", "shadow")}


def test_skipped_step_leaves_every_buffer_and_the_step_count_untouched(P):
    """A finite loss under a loss scale of 2^30: the fp16 activation gradient overflows, flat.grad is not finite (both asserted), the
    call returns skipped = 1.0, master, momentum and shadow keep their bits and optimizer.steps stays 0.  The momentum buffer is
    pre-filled with 0.5 in front of the skipped call: were the step count advanced after all, the following normal step would read
    it (over a zeroed buffer mu * 0 + d is d, and a lost first step would not show).  That step is bit-equal, in all three
    buffers, to the first step of a twin head that never saw the skipped call."""
    sgd = dict(lr=0.02, momentum=0.9, weight_decay=1e-4)
    head, opt = make_head(P, **sgd)
    twin, opt_twin = make_head(P, **sgd)
    data = batch(P)
    head.flat.momentum.fill_(0.5)
    before = state(head.flat)
    assert torch.equal(before["master"], twin.flat.master)
    out = P.T.box_head_train_step(head, opt, None, *data, loss_scale=2.0 ** 30)
    assert out.pop("skipped") == 1.0
    assert len(out) == 3 and all(math.isfinite(v) for v in out.values()), out
    assert not bool(torch.isfinite(head.flat.grad).all())
    for k, v in state(head.flat).items():
        T.same_bits(host(v), host(before[k]), f"{k} after a skipped step")
    assert opt.steps == 0
    out = P.T.box_head_train_step(head, opt, None, *data, loss_scale=1024.0)
    out_twin = P.T.box_head_train_step(twin, opt_twin, None, *data, loss_scale=1024.0)
    assert "skipped" not in out and out == out_twin and opt.steps == opt_twin.steps == 1
    assert not torch.equal(head.flat.master, before["master"])
    for k, v in state(head.flat).items():
        T.same_bits(host(v), host(getattr(twin.flat, k)), f"{k} after the step that follows a skipped one")


def test_per_tensor_clipping_scales_exactly_the_tensors_above_the_threshold(P):
    """Momentum 0, weight decay 0, lr 4 and loss scale 1024 (powers of two: lr * m and the un-scaling are exact), so that a
    tensor's update is lr times its (clipped) gradient.  The threshold is the geometric mean of the smallest and the largest
    scaled gradient norm of an unclipped twin's first step.  Tensors below it: the twin's bits.  Tensors above it, in float64:
        lr clip s (1 - 1e-5) <= ||dp||_2 <= lr clip (1 + 1e-5),   s = ns / (ns + 1e-6)
    with ns the tensor's scaled norm as the step computes it: the coefficient clip / (ns + 1e-6) brings the norm to clip * s, not to
    clip.  The 1e-5 is the rounding margin; train_exact.clip_rounding_margin derives it for each tensor from its size and from
    ||p||_2 / (lr clip) - the subtraction p - lr m rounds relative to p, which is why lr is large here - and it must come out under
    1e-5.  The issue's floor lr clip (1 - 1e-3) is asserted as well, with the slack 1 - s it has to cover."""
    lr, loss_scale = 4.0, 1024.0
    sgd = dict(lr=lr, momentum=0.0, weight_decay=0.0)
    twin, opt_twin = make_head(P, **sgd)
    head, opt = make_head(P, **sgd)
    data = batch(P)
    start = twin.flat.master.clone()
    P.T.box_head_train_step(twin, opt_twin, None, *data, loss_scale=loss_scale)
    flat = twin.flat
    ns = {}
    for name in flat.names:
        o, n = flat.offsets[name]
        ns[name] = float(flat.grad[o:o + n].norm()) * (1.0 / loss_scale)
    clip = math.sqrt(min(ns.values()) * max(ns.values()))
    above = [n for n in flat.names if ns[n] > clip]
    below = [n for n in flat.names if ns[n] < clip]
    assert above and below and len(above) + len(below) == len(flat.names), ns
    out = P.T.box_head_train_step(head, opt, None, *data, loss_scale=loss_scale, clip_grad_norm=clip)
    assert "skipped" not in out
    print(f"clip {clip:.4g}; scaled norms {ns}")
    for name in flat.names:
        o, n = flat.offsets[name]
        r = slice(o, o + n)
        if name in below:
            T.same_bits(host(head.flat.master[r]), host(twin.flat.master[r]), f"{name}: below the threshold")
            T.same_bits(host(head.flat.shadow[r]), host(twin.flat.shadow[r]), f"{name}: below the threshold, shadow")
            continue
        margin = T.clip_rounding_margin(n, float(start[r].double().norm()), lr, clip)
        s = ns[name] / (ns[name] + 1e-6)
        dp = float((head.flat.master[r].double() - start[r].double()).norm())
        print(f"{name}: ||dp|| / (lr clip) - 1 = {dp / (lr * clip) - 1:.3e}, s - 1 = {s - 1:.3e}, rounding margin {margin:.3e}")
        assert margin <= 1e-5 and (1 - s) + 1e-5 <= 1e-3, (name, margin, s)
        assert dp <= lr * clip * (1 + 1e-5), (name, dp, lr * clip)
        assert dp >= lr * clip * s * (1 - 1e-5), (name, dp, lr * clip * s)
        assert dp >= lr * clip * (1 - 1e-3), (name, dp, lr * clip)
        assert not torch.equal(head.flat.master[r], twin.flat.master[r])
