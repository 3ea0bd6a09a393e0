"""The pack entry points against tests/golden/pack_rows_parent.npz: what pe_proben_pack_calibrated wrote on the log-posterior route
at the commit before the three pack kernels became one (tests/golden/gen_pack_rows.py describes the four cases; DESIGN.md names the
commit).  Bit for bit, by tobytes() on the live rows [b*S, b*S + counts[b]) - the rest of the buffers is uninitialised memory."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TEMPS = (1.3, 0.7, 2.0)
SCALES = (0.25, 1.0, 7.25)
INPUTS = ("boxes", "classes", "class_logits", "prob_score", "scores", "vars", "counts")
OUTPUTS = ("boxes", "scores", "probs", "vars", "classes", "offsets", "counts", "single", "log_probs")      # the order of fusion.pack_rows
PER_IMAGE = ("offsets", "counts", "single")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "pack_rows_parent.npz"))


def _case(z, name):
    nd, B, D, K, max_class = (int(v) for v in z[f"{name}_meta"])
    host = [{k: z[f"{name}_d{d}_{k}"] for k in INPUTS} for d in range(nd)]
    dets = [{k: torch.from_numpy(v).cuda() for k, v in h.items()} for h in host]
    want = {k: z[f"{name}_out_{k}"] for k in OUTPUTS}
    return nd, B, D, K, max_class, host, dets, want


def _live(out, S):
    torch.cuda.synchronize()
    cnt = out[6].cpu().numpy()
    live = (np.arange(S)[None] < cnt[:, None]).reshape(-1)
    return {k: (t.cpu().numpy() if k in PER_IMAGE else t.cpu().numpy()[live]) for k, t in zip(OUTPUTS, out)}


def _same(got, want, keys, what):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k}"


def _kept(host, key, B, D, max_class):
    """The float32 input of every packed row, in packed order: image by image, detector by detector, the first min(counts, D) rows with
    class <= max_class."""
    def rows(h, b):
        c = min(int(h["counts"][b]), D)
        return h[key][b, :c][h["classes"][b, :c] <= max_class]
    return np.concatenate([rows(h, b) for b in range(B) for h in host])


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_every_pack_entry_point_reproduces_the_parents_rows(golden, name):
    from proben_amd import fusion as F
    nd, B, D, K, max_class, host, dets, want = _case(golden, name)
    S, T, scales = nd * D, TEMPS[:nd], SCALES[:nd]
    var64 = _kept(host, "vars", B, D, max_class).astype(np.float64)
    assert int(want["counts"].sum()) == len(var64) > 0
    shared = [k for k in OUTPUTS if k != "vars"]
    # pe_proben_pack_calibrated, log-posterior route: the file
    got = _live(F.pack_rows(dets, max_class, temperatures=T, log_posteriors=True, variance_scales=scales), S)
    _same(got, want, OUTPUTS, "calibrated log-posteriors")
    # ... with all scales 1.0: the unscaled bits
    one = _live(F.pack_rows(dets, max_class, temperatures=T, log_posteriors=True, variance_scales=[1.0] * nd), S)
    _same(one, want, shared, "calibrated, scales 1.0")
    assert one["vars"].tobytes() == var64.tobytes()
    # pe_proben_pack_log_posteriors and pe_proben_pack_logits: every output they share with it; the plain variances
    lp = _live(F.pack_rows(dets, max_class, temperatures=T, log_posteriors=True), S)
    _same(lp, want, shared, "log-posteriors")
    lo = _live(F.pack_rows(dets, max_class, temperatures=T), S)
    _same(lo, want, shared[:-1], "logits")
    assert lp["vars"].tobytes() == var64.tobytes() and lo["vars"].tobytes() == var64.tobytes()
    # pe_proben_pack_detections: the same rows; scores, probabilities and variances the exact widening of its float32 inputs
    pr = _live(F.pack_rows(dets, max_class), S)
    _same(pr, want, ("boxes", "classes") + PER_IMAGE, "probabilities")
    assert pr["vars"].tobytes() == var64.tobytes()
    assert pr["scores"].tobytes() == _kept(host, "scores", B, D, max_class).astype(np.float64).tobytes()
    assert pr["probs"].tobytes() == _kept(host, "prob_score", B, D, max_class).astype(np.float64).tobytes()
    # the calibrated probabilities and logits routes: the route's own bits, and the file's variances
    for kw, ref in ((dict(), pr), (dict(temperatures=T), lo)):
        cal = _live(F.pack_rows(dets, max_class, variance_scales=scales, **kw), S)
        _same(cal, ref, [k for k in OUTPUTS[:-1] if k != "vars"], f"calibrated {sorted(kw)}")
        assert cal["vars"].tobytes() == want["vars"].tobytes()


def test_the_cases_hold_what_they_are_meant_to_hold(golden):
    """The fixture itself: case A's counts, its empty and its single-source image, a dropped class across the chunk boundary, the
    class -1 row (kept, NaN score), the saturated row (finite), the +inf and the NaN logit (NaN probabilities), the NaN variance."""
    nd, B, D, K, max_class, host, _, want = _case(golden, "A")
    counts = sorted(int(c) for h in host for c in h["counts"])
    assert {0, 1, 64, 65, 66}.issubset(counts) and max(counts) > D
    assert want["counts"].tolist()[1] == 0 and want["single"].tolist() == [0, 0, 1] and want["offsets"].tolist() == [0, nd * D, 2 * nd * D]
    assert (host[1]["classes"][0, 62] > max_class) and (host[1]["classes"][0, 64] <= max_class)
    assert int((want["classes"] == -1).sum()) == 1 and np.isnan(want["scores"][want["classes"] == -1]).all()
    assert int(np.isnan(want["probs"]).any(1).sum()) == 2 and int(np.isnan(want["vars"]).sum()) == 1
    sat = np.nonzero((want["probs"] == 1.0).any(1))[0]
    assert len(sat) >= 1 and np.isfinite(want["log_probs"][sat]).all()
    for name, k1 in (("B", 5), ("C", 64), ("D", 65)):
        assert golden[f"{name}_out_log_probs"].shape[1] == k1 and np.isfinite(golden[f"{name}_out_log_probs"]).all()
    assert 1 in golden["B_d0_counts"].tolist()
