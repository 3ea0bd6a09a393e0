"""tests/train_exact.py on the host: the float32 restatement of the fused SGD step against its longdouble restatement within a
bound derived from the terms, the generator's conditions on every HipLinear operand set tests/test_train_exact_gpu.py uses, and -
the point of the module - the mutants that the bit comparison has to reject: a contracted or reordered optimiser kernel, a first
step that reads the momentum buffer, an unwritten tail, a stale shadow, a ReLU mask that lets y == 0 through, a wrong ragged row,
padded rows that count, a bias where the launch has none.  Every one of them passes the tolerances of tests/test_training_gpu.py."""
import numpy as np
import pytest
import torch

import conv_exact as E
import train_exact as T

ids = lambda cases: [c.name for c in cases]
CPU_SIZES = [n for n in T.SGD_SIZES if n < 10 ** 5]
MUTANT_N = 4 * 256 * 3 + 2                               # three whole blocks of vectors and a two-element tail


# ------------------------------------------------------------------------------------------------ fused SGD: the restatement
@pytest.mark.parametrize("cfg", T.SGD_CONFIGS, ids=ids(T.SGD_CONFIGS))
@pytest.mark.parametrize("n", CPU_SIZES)
def test_float32_restatement_stays_within_the_derived_bound_of_the_longdouble_one(n, cfg):
    """Step by step from the SAME fp32 state (the float32 trajectory's), so that the bound is that of one call: per element
    |p32 - p| and |m32 - m| stay under the sums of the absolute terms times half an ulp per rounding (train_exact.sgd_step_longdouble) -
    and the bound is tight enough to mean something: under 8 half-ulps of the largest term of the element."""
    p, m, grads = T.sgd_operands(n, cfg)
    h = p.astype(np.float16)
    for s, g in enumerate(grads):
        p2, m2, h2 = T.sgd_step_f32(p, g, m, h, cfg.lr, cfg.mu, cfg.wd, cfg.gs, s == 0)
        pl, ml, ep, em = T.sgd_step_longdouble(p, g, m, cfg.lr, cfg.mu, cfg.wd, cfg.gs, s == 0)
        assert bool((np.abs(p2.astype(np.longdouble) - pl) <= ep).all()), (n, s)
        assert bool((np.abs(m2.astype(np.longdouble) - ml) <= em).all()), (n, s)
        lr, mu, wd, gs = (np.longdouble(v) for v in T.sgd_scalars(cfg.lr, cfg.mu, cfg.wd, cfg.gs))
        big = np.maximum.reduce([np.abs(g * gs), np.abs(wd * p), np.abs(mu * m) * (s > 0), np.abs(ml), np.abs(p.astype(np.longdouble)), np.abs(pl)])
        assert bool((ep <= 8 * T.U * big * 1.001 + 1e-44).all()) and bool((em <= 8 * T.U * big * 1.001 + 1e-44).all())
        assert h2.dtype == np.float16 and h2.tobytes() == p2.astype(np.float16).tobytes()
        p, m, h = p2, m2, h2


def test_scalars_are_narrowed_once_from_the_double_product():
    """FusedSGD passes base * factor formed in double; narrowing the factors first gives another float for these values."""
    lr, factor = 0.03, 1.3
    assert T.sgd_scalars(lr * factor, 0.9, 0.0, 1.0)[0] == np.float32(lr * factor)
    assert np.float32(lr * factor) != np.float32(lr) * np.float32(factor)


def test_first_step_ignores_a_nan_momentum_buffer():
    cfg = T.SGD_CONFIGS[0]
    p, _, grads = T.sgd_operands(1025, cfg)
    nan = np.full_like(p, np.nan)
    for q in T.sgd_run(p, nan, p.astype(np.float16), grads, cfg):
        assert all(bool(np.isfinite(v.astype(np.float32)).all()) for v in q)


# ------------------------------------------------------------------------------------------------ fused SGD: the mutants
def _runs(cfg, mutant, mutant_steps=None):
    p, m0, grads = T.sgd_operands(MUTANT_N, cfg)
    h0 = np.full(MUTANT_N, 3.0, np.float16)
    return (p, m0, h0), T.sgd_run(p, m0, h0, grads, cfg), T.sgd_run(p, m0, h0, grads, cfg, mutant, mutant_steps)


@pytest.mark.parametrize("mutant,step,field", [("fma_d", 0, 1), ("fma_d", 1, 1), ("fma_m", 1, 1), ("fma_p", 0, 0), ("fma_p", 1, 0),
                                               ("reads_momentum", 0, 1), ("stale_shadow", 0, 2), ("stale_shadow", 2, 2)])
def test_mutant_changes_at_least_one_percent_of_the_elements_it_can_affect(mutant, step, field):
    """The mutant acts at `step` only, from the restatement's own state before it: the share of elements of its own output
    (0: p, 1: m, 2: h) whose bits change.  Contraction removes one rounding, so it shows wherever that rounding was not exact."""
    cfg = T.SGD_CONFIGS[0]
    _, want, got = _runs(cfg, mutant, {step})
    for s in range(step):
        for a, b in zip(got[s], want[s]):
            assert a.tobytes() == b.tobytes()                       # the mutant has not acted yet
    share = T.differing(got[step][field], want[step][field])
    assert share >= 0.01, (mutant, step, share)
    with pytest.raises(AssertionError, match="differ in bits"):
        T.same_bits(got[step][field], want[step][field])


def test_contracted_momentum_line_cannot_show_on_the_first_step():
    """first_step takes d as it is: the mutant of line 2 can only affect later steps (the case list above starts it at step 1)."""
    _, want, got = _runs(T.SGD_CONFIGS[0], "fma_m", {0})
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], want[0]))


@pytest.mark.parametrize("cfg", T.SGD_CONFIGS, ids=ids(T.SGD_CONFIGS))
@pytest.mark.parametrize("n", [n for n in CPU_SIZES if n % 4])
@pytest.mark.parametrize("step", range(T.SGD_STEPS))
def test_mutant_unwritten_tail_changes_every_tail_element(n, cfg, step):
    p, m0, grads = T.sgd_operands(n, cfg)
    h0 = np.full(n, 3.0, np.float16)
    want = T.sgd_run(p, m0, h0, grads, cfg)
    got = T.sgd_run(p, m0, h0, grads, cfg, "tail_unwritten", {step})
    t = n - n % 4
    for f in (0, 1):                                                # p and m, every tail element; the vector part is untouched
        assert bool((got[step][f][t:] != want[step][f][t:]).all()), (n, step, f)
        assert got[step][f][:t].tobytes() == want[step][f][:t].tobytes()
    assert bool((got[step][2][t:] != want[step][2][t:]).any())


# ------------------------------------------------------------------------------------------------ HipLinear: the generator's conditions
@pytest.mark.parametrize("c", T.LINEAR_CASES, ids=ids(T.LINEAR_CASES))
def test_linear_operands_meet_the_conditions_at_every_accumulation_point(c):
    stats = T.linear_conditions(c)
    assert [s["name"].split(".")[1] for s in stats] == ["y", "dx", "dw", "db"]
    assert all(s["log2_budget_used"] < 20 for s in stats)
    assert ("ties" in stats[0]) == (not c.out_f32) and "ties" in stats[1]
    o, want = T.linear_clean(c)
    for key, dt in (("x", torch.float16), ("w", torch.float16), ("dy", torch.float16), ("b", torch.float32)):
        assert bool((o[key].to(dt).double() == o[key]).all()), f"{key} not representable in the kernel's input type"
    assert (want["y"].dtype, want["dx"].dtype, want["dw"].dtype, want["db"].dtype) == (
        torch.float32 if c.out_f32 else torch.float16, torch.float16, torch.float32, torch.float32)
    assert all(bool(torch.isfinite(v).all()) for v in want.values())
    assert float((o["x"][0] @ o["w"][0] + o["b"][0]).abs()) == 0.0 and float(o["dy"][0, 0]) != 0.0    # the planted pre-activation
    if c.relu:
        zeroed = (want["y"] <= 0).double().mean()
        assert 0.2 <= float(zeroed) <= 0.8, float(zeroed)
        edge = (want["y"] == 0) & (o["dy"] != 0)
        assert bool(edge[0, 0]) and int(edge.sum()) > 1              # y exactly 0 under a dy that is not: what the mask's > decides


def test_linear_cases_cover_the_shapes_they_are_there_for():
    a, b, c, d = T.LINEAR_CASES
    assert a.K == 64 and a.pad == 14 and a.out_f32                                   # one K-step, rows padded 50 -> 64
    assert b.M > 128 and b.M % 64 and (b.M + b.pad) // 64 == 3 and b.N % 128 == 64   # a ragged second row tile, dW over three K-steps, half a column tile
    assert c.pad == 0 and c.K == 1024 and c.out_f32                                  # the predictor: whole rows
    assert d.fwd == T.RING and d.M % 64 and d.dx == d.dw == T.IG128                 # ring forward, both backward launches generic


def test_linear_reference_is_torch_autograd_in_float64():
    """The hand-written backward equals autograd's on the same operands (no rounding of y: out_f32 cases and the mask's sign only)."""
    for c in T.LINEAR_CASES:
        o, _ = T.linear_clean(c)
        exact, _ = T.linear_stages(c, o)
        x, w, b = (o[k].clone().requires_grad_() for k in ("x", "w", "b"))
        y = x @ w.t() + b
        y = torch.relu(y) if c.relu else y
        y.backward(o["dy"])
        assert torch.equal(y.detach(), exact["y"])
        assert torch.equal(x.grad, exact["dx"]) and torch.equal(w.grad, exact["dw"]) and torch.equal(b.grad, exact["db"])


# ------------------------------------------------------------------------------------------------ HipLinear: the mutants
@pytest.mark.parametrize("c", T.LINEAR_CASES, ids=ids(T.LINEAR_CASES))
def test_linear_mutants_are_rejected_by_the_bit_comparator(c):
    o, want = T.linear_clean(c)
    got = lambda m: T.linear_stages(c, o, m)[1]
    assert not any(E.rejects(got(None)[k], want[k]) for k in want)
    mut = got("tail_row_zeroed")
    assert E.rejects(mut["dx"], want["dx"]) and int((mut["dx"] != want["dx"]).any(1).sum()) == 1
    mut = got("bias_on_dx")
    assert E.rejects(mut["dx"], want["dx"]) and not E.rejects(mut["dw"], want["dw"])
    mut = got("pad_rows_counted")
    assert E.rejects(mut["dw"], want["dw"]) == (c.pad > 0)          # whole rows (the predictor's 64): nothing is padded
    mut = got("mask_ge")
    if c.relu:
        assert all(E.rejects(mut[k], want[k]) for k in ("dx", "dw", "db")) and not E.rejects(mut["y"], want["y"])
    else:
        assert not any(E.rejects(mut[k], want[k]) for k in want)


def test_clip_margin_grows_with_the_parameters_norm_and_shrinks_with_the_step():
    assert T.clip_rounding_margin(1 << 20, 0.0, 0.5, 1.0) == 23 * T.U
    assert T.clip_rounding_margin(128, 10.0, 0.5, 0.2) > T.clip_rounding_margin(128, 10.0, 1.0, 0.2) > T.clip_rounding_margin(128, 0.0, 1.0, 0.2)
