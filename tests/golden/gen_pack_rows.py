"""Generate tests/golden/pack_rows_parent.npz: the inputs of four small pack cases and what pe_proben_pack_calibrated wrote for them
on the log-posterior route (temperatures (1.3, 0.7, 2.0), variance scales (0.25, 1.0, 7.25), the first `nd` of each), recorded on
the GPU at the commit BEFORE the three pack kernels were merged into one (DESIGN.md names it).  tests/test_pack_golden_gpu.py holds
every pack entry point to these bits.

    python tests/golden/gen_pack_rows.py [--out FILE]

Only the public call surface is used (fusion.pack_rows).  Of the outputs only the live rows [b*S, b*S + counts[b]) are stored, image
after image: the rest of the buffers is uninitialised memory.  Before writing, the generator checks what the test will check of the
other entry points at this commit (shared outputs equal, variances and the probabilities route the exact float64 widening).

Cases (nd, B, D, K, max_class):
  A (3, 3, 66, 3, 1)  counts 64 / 65 / 66 in image 0 (two chunks of 64, rows of class 2 dropped on both sides of the boundary), image 1
                      empty, image 2 single-source: detector 0 has one row and it is dropped, detector 1 says 70 (> D, clamped to 66),
                      detector 2 has none.  One kept row of class -1 (NaN score on the logits routes), one saturated row (+800 / -800),
                      one row with a +inf logit, one with a NaN logit, one NaN variance.
  B (2, 2, 9, 4, 3)   K + 1 = 5: groups of 8 lanes, 3 of them padding; a detector with exactly one (kept) row.
  C (2, 2, 5, 63, 62) K + 1 = 64: one row per wavefront pass.
  D (2, 2, 5, 64, 63) K + 1 = 65: the serial path.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

TEMPS = (1.3, 0.7, 2.0)
SCALES = (0.25, 1.0, 7.25)
CASES = {"A": (3, 3, 66, 3, 1), "B": (2, 2, 9, 4, 3), "C": (2, 2, 5, 63, 62), "D": (2, 2, 5, 64, 63)}
COUNTS = {"A": [[64, 0, 1], [65, 0, 70], [66, 0, 0]],        # [detector][image]
          "B": [[9, 1], [7, 0]], "C": [[5, 2], [0, 4]], "D": [[5, 2], [0, 4]]}
INPUTS = ("boxes", "classes", "class_logits", "prob_score", "scores", "vars", "counts")
OUTPUTS = ("boxes", "scores", "probs", "vars", "classes", "offsets", "counts", "single", "log_probs")     # the order of pack_rows


def make_inputs(name):
    """One case's detectors as NumPy arrays (every padded row filled: nothing the kernels may not read is special)."""
    nd, B, D, K, max_class = CASES[name]
    rng = np.random.default_rng(20261017 + ord(name))
    dets = []
    for d in range(nd):
        x1, y1 = rng.uniform(0, 500, (B, D)), rng.uniform(0, 400, (B, D))
        bx = np.stack([x1, y1, x1 + rng.uniform(20, 120, (B, D)), y1 + rng.uniform(20, 100, (B, D))], 2).astype(np.float32)
        cls = rng.integers(0, max_class + 2, (B, D)).astype(np.int32)                  # max_class + 1: dropped
        lg = rng.normal(0, 3, (B, D, K + 1)).astype(np.float32)
        var = (10.0 ** rng.uniform(-3, 1, (B, D))).astype(np.float32)
        if name == "A" and d == 0:
            cls[0, 3], cls[0, 5], cls[0, 63] = -1, 1, 2                                # class -1 is kept; the chunk's last row dropped
            lg[0, 5] = [-800.0, 800.0, -800.0, -800.0]
            cls[0, 7], cls[0, 9] = 0, 1
            lg[0, 7, 2] = np.inf
            lg[0, 9, 0] = np.nan
            var[0, 11], cls[0, 11] = np.float32("nan"), 0
            cls[2, 0] = 2                                                              # image 2: its only row is dropped
        if name == "A" and d == 1:
            cls[0, 62:66] = [2, 0, 1, 2]                                               # drops before the boundary, a kept row after it
        if name == "B" and d == 0:
            cls[1, 0] = 2                                                              # the one-row detector's row is kept
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.exp(lg - lg.max(2, keepdims=True))
            p = (e / e.sum(2, keepdims=True)).astype(np.float32)
        sc = np.take_along_axis(p, np.clip(cls, 0, K)[..., None].astype(np.int64), 2)[..., 0].copy()
        dets.append({"boxes": bx, "classes": cls, "class_logits": lg, "prob_score": p[:, :, :K].copy(), "scores": sc, "vars": var,
                     "counts": np.asarray(COUNTS[name][d], np.int32)})
    return dets


def live_rows(out, S):
    """pack_rows' tuple -> dict of NumPy arrays, the per-row ones cut to the live rows of every image."""
    import torch
    torch.cuda.synchronize()
    cnt = out[6].cpu().numpy()
    live = (np.arange(S)[None] < cnt[:, None]).reshape(-1)
    return {k: (t.cpu().numpy() if k in ("offsets", "counts", "single") else t.cpu().numpy()[live]) for k, t in zip(OUTPUTS, out)}


def main():
    import torch
    import proben_amd  # noqa: F401
    from proben_amd import fusion as F
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "pack_rows_parent.npz")
    z = {}
    same = lambda a, b: a.tobytes() == b.tobytes()  # noqa: E731
    for name, (nd, B, D, K, max_class) in CASES.items():
        host = make_inputs(name)
        dets = [{k: torch.from_numpy(v).cuda() for k, v in h.items()} for h in host]
        S, T, sc = nd * D, TEMPS[:nd], SCALES[:nd]
        got = live_rows(F.pack_rows(dets, max_class, temperatures=T, log_posteriors=True, variance_scales=sc), S)
        z[f"{name}_meta"] = np.asarray([nd, B, D, K, max_class], np.int32)
        for d, h in enumerate(host):
            for k in INPUTS:
                z[f"{name}_d{d}_{k}"] = h[k]
        for k, v in got.items():
            z[f"{name}_out_{k}"] = v
        # what the test asks of the other entry points holds at this commit too
        cnt = got["counts"]

        def kept(key):      # the float32 input of every packed row, in packed order
            return np.concatenate([h[key][b, :min(int(h["counts"][b]), D)][h["classes"][b, :min(int(h["counts"][b]), D)] <= max_class]
                                   for b in range(B) for h in host])
        var32 = kept("vars")
        lp = live_rows(F.pack_rows(dets, max_class, temperatures=T, log_posteriors=True), S)
        lo = live_rows(F.pack_rows(dets, max_class, temperatures=T), S)
        pr = live_rows(F.pack_rows(dets, max_class), S)
        one = live_rows(F.pack_rows(dets, max_class, temperatures=T, log_posteriors=True, variance_scales=[1.0] * nd), S)
        ok = all(same(lp[k], got[k]) and same(one[k], got[k]) for k in OUTPUTS if k != "vars")
        ok &= all(same(lo[k], got[k]) for k in OUTPUTS[:-1] if k != "vars")
        ok &= all(same(pr[k], got[k]) for k in ("boxes", "classes", "offsets", "counts", "single"))
        ok &= all(same(x["vars"], var32.astype(np.float64)) for x in (lp, lo, pr, one))
        ok &= same(pr["scores"], kept("scores").astype(np.float64)) and same(pr["probs"], kept("prob_score").astype(np.float64))
        print(f"case {name}: rows per image {cnt.tolist()} single {got['single'].tolist()} NaN scores {int(np.isnan(got['scores']).sum())} "
              f"NaN prob rows {int(np.isnan(got['probs']).any(1).sum())}  other entry points agree: {bool(ok)}", flush=True)
        if not ok:
            raise SystemExit(f"case {name}: the entry points disagree at this commit - not written")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
