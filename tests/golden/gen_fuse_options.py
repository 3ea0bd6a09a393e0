"""Generate tests/golden/fuse_options_parent.npz: two small sets of detector outputs (forward_batch's layout, 2 and 3 detectors) and
what fusion.fuse_detections - and, for three of them, late_fusion.late_fusion - gave for fifteen combinations of the fusion's options,
recorded on the GPU at the commit BEFORE the options moved into options.FusionOptions (DESIGN.md section 20 names it).
tests/test_fuse_options_golden_gpu.py holds the keyword surface, options= and a reused FusionOptions to these bits.

    python tests/golden/gen_fuse_options.py [--out FILE]

Only the public call surface is used, through keywords every entry point has had since the option it names, so the file runs unchanged
on that commit.  Of the per-row outputs only the live rows are stored: [b*S, b*S + counts[b]) of the outputs indexed by fused row,
[b*S, b*S + in_counts[b]) of "cluster" and "row_source", which are indexed by input row; the rest of the buffers is uninitialised.

B = 3 images, D = 12 slots per detector, K = 3 classes:
  image 0  every detector fired: a cluster of two rows (one of them saturated, logits +800 / -800), a cluster of three that holds two
           rows of detector 0, lone rows, and one row of a class above max_class that the pack drops;
  image 1  no rows;
  image 2  detector 1 alone fired (the passthrough path): three rows, two of them overlapping.
The generator refuses to write when a combination merges nothing on image 0 or image 2 is not a passthrough image."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

B, D, K, MAX_CLASS = 3, 12, 3, 2
SETS = (2, 3)
INPUTS = ("boxes", "classes", "class_logits", "prob_score", "scores", "vars", "counts")
PER_INPUT_ROW = ("cluster", "row_source")
TEMPS = (1.3, 0.7, 2.0)
PRIOR = (0.1, 0.3, 0.2, 0.4)
SCALES = (0.25, 1.0, 7.25)
POOL = (0.6, 0.5, 0.8)
CORR = ((0.5, 0.2, 0.15), (0.2, 0.5, 0.25), (0.15, 0.25, 0.5))      # diagonally dominant: every cluster's matrix is positive definite
T, P, V, W, Q, E, C = "temperatures", "class_prior", "variance_scales", "pool_weights", "with_posterior", "presence", "box_correlation"
COMBOS = (("probEn", "v-avg", ()),
          ("probEn", "s-avg", (T,)),
          ("avg", "avg", (V,)),
          ("max", "argmax", (T,)),
          ("probEn-log", "v-avg", ()),
          ("probEn-log", "v-avg", (T, P, V)),
          ("probEn-log", "v-avg", (T, P, V, W)),
          ("probEn-log", "v-avg", (T, P, V, W, Q)),
          ("probEn-log", "v-avg", (T, P, V, Q)),
          ("probEn-log", "v-avg", (E,)),
          ("probEn-log", "v-avg", (E, W, Q)),
          ("probEn-log", "c-avg", (C,)),
          ("probEn-log", "c-avg", (C, W)),
          ("probEn-log", "c-avg", (C, Q)),
          ("probEn-log", "c-avg", (C, E)))
LATE = (0, 7, 14)       # the combinations late_fusion is recorded for as well


def presence_of(nd):
    t = np.random.default_rng(20261019 + nd).normal(0.0, 1.5, (2 ** nd, K + 1))
    t[:, K] = 0.0
    return t


def options(nd, keys):
    """The keyword arguments of one combination for nd detectors."""
    values = {T: list(TEMPS[:nd]), P: list(PRIOR), V: list(SCALES[:nd]), W: list(POOL[:nd]), Q: True, E: presence_of(nd),
              C: np.array(CORR)[:nd, :nd].copy()}
    return {k: values[k] for k in keys}


def make_inputs(nd):
    """nd detectors' outputs as NumPy arrays; every padded slot is filled with rows like the live ones."""
    rng = np.random.default_rng(20261019 * 10 + nd)
    # (anchor x, anchor y, class) of the live rows of [detector][image]; rows of one anchor overlap with IoU > 0.8
    a, b, c, e, f, g = (10, 10, 0), (210, 10, 1), (410, 10, 2), (10, 210, 1), (210, 210, 0), (410, 210, 3)
    live = [[[a, b, b, c, g], [], []],
            [[a, b, e], [], [a, a, b]],
            [[a, f, e], [], []]][:nd]
    dets = []
    for d in range(nd):
        x1, y1 = rng.uniform(0, 500, (B, D)), rng.uniform(300, 400, (B, D))
        bx = np.stack([x1, y1, x1 + rng.uniform(20, 120, (B, D)), y1 + rng.uniform(20, 100, (B, D))], 2)
        cls = rng.integers(0, MAX_CLASS + 1, (B, D)).astype(np.int32)
        for i in range(B):
            for j, (x, y, k) in enumerate(live[d][i]):
                bx[i, j] = np.array([x, y, x + 60.0, y + 50.0]) + rng.uniform(-2.0, 2.0, 4)
                cls[i, j] = k
        lg = rng.normal(0, 2, (B, D, K + 1))
        np.put_along_axis(lg, cls[..., None].astype(np.int64), np.take_along_axis(lg, cls[..., None].astype(np.int64), 2)
                          + rng.uniform(1.0, 6.0, (B, D, 1)), 2)
        if d == 1:
            lg[0, 0] = [800.0, -800.0, -800.0, -800.0]          # the saturated row, in the cluster of two (three with detector 2)
        lg = lg.astype(np.float32)
        e_ = np.exp(lg - lg.max(2, keepdims=True))
        p = (e_ / e_.sum(2, keepdims=True)).astype(np.float32)
        sc = np.take_along_axis(p, cls[..., None].astype(np.int64), 2)[..., 0].copy()
        dets.append({"boxes": bx.astype(np.float32), "classes": cls, "class_logits": lg, "prob_score": p[:, :, :K].copy(), "scores": sc,
                     "vars": (10.0 ** rng.uniform(-1, 0.7, (B, D))).astype(np.float32),
                     "counts": np.asarray([len(rows) for rows in live[d]], np.int32)})
    return dets


def to_device(host):
    import torch
    return [{k: torch.from_numpy(v).cuda() for k, v in h.items()} for h in host]


def j1_of(host):
    """The same detections as prediction-file dicts (late_fusion's input), through JSON like a file that was written and read."""
    out = []
    for h in host:
        rec = {k: [] for k in ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")}
        for b in range(B):
            keep = [j for j in range(int(h["counts"][b])) if int(h["classes"][b, j]) <= MAX_CLASS]
            rec["image"].append(f"f{b}.jpeg")
            rec["image_id"].append(b)
            for key, s in (("boxes", "boxes"), ("scores", "scores"), ("classes", "classes"), ("class_logits", "class_logits"),
                           ("probs", "prob_score")):
                rec[key].append([h[s][b, j].tolist() for j in keep])
            rec["vars"].append([[float(h["vars"][b, j])] for j in keep])
        out.append(json.loads(json.dumps(rec)))
    return out


def live_rows(out):
    """fuse_detections' dict -> {key: ndarray}: per-row tensors cut to their live rows, per-image tensors whole, the stride."""
    import torch
    torch.cuda.synchronize()
    S = int(out["stride"])
    cnt, cin = out["counts"].cpu().numpy(), out["in_counts"].cpu().numpy()
    got = {"stride": np.asarray(S, np.int32)}
    for k, t in out.items():
        if not isinstance(t, torch.Tensor):
            continue
        x = t.cpu().numpy()
        if x.shape[:2] == (B, S):           # "keep" of the ('max', 'argmax') route
            x = x.reshape((B * S,) + x.shape[2:])
        if x.shape[0] == B * S:
            x = x[(np.arange(S)[None] < (cin if k in PER_INPUT_ROW else cnt)[:, None]).reshape(-1)]
        got[k] = x
    return got


def late_rows(results):
    """late_fusion's list -> {"len": entries per image (0: skipped), "<image>_<position>": ndarray}."""
    import torch
    got = {"len": np.asarray([0 if r is None else len(r) for r in results], np.int32)}
    for i, r in enumerate(results):
        for j, x in enumerate(r or ()):
            got[f"{i}_{j}"] = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return got


def case_name(nd, idx):
    return f"n{nd}_c{idx:02d}"


def pack(arrays):
    """{name: ndarray} -> two uint8 arrays: a JSON index [name, dtype, shape, offset] and the arrays' bytes one after another (a zip
    entry per small array would cost more than the array)."""
    index, blob = [], b""
    for k, v in arrays.items():
        index.append([k, v.dtype.str, list(v.shape), len(blob)])
        blob += v.tobytes()
    return np.frombuffer(json.dumps(index).encode(), np.uint8), np.frombuffer(blob, np.uint8)


def unpack(index, blob):
    """pack's inverse: {name: ndarray}."""
    out = {}
    for k, dt, shape, at in json.loads(bytes(index).decode()):
        n = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[k] = np.frombuffer(bytes(blob[at:at + n]), np.dtype(dt)).reshape(shape)
    return out


def main():
    import proben_amd  # noqa: F401
    from proben_amd import fusion as F
    from proben_amd.late_fusion import late_fusion
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "fuse_options_parent.npz")
    z, rec = {}, {}
    for nd in SETS:
        host = make_inputs(nd)
        fired = np.array([[int(h["counts"][b]) > 0 for h in host] for b in range(B)])
        if not (fired[0].all() and not fired[1].any() and fired[2].sum() == 1):
            raise SystemExit(f"nd {nd}: the images are not (all fired, none fired, one fired) - not written")
        for d, h in enumerate(host):
            for k in INPUTS:
                z[f"n{nd}_d{d}_{k}"] = h[k]
        z[f"n{nd}_presence"] = presence_of(nd)
        dets, j1 = to_device(host), j1_of(host)
        for idx, (score, box, keys) in enumerate(COMBOS):
            name = case_name(nd, idx)
            got = live_rows(F.fuse_detections(dets, score, box, max_class=MAX_CLASS, **options(nd, keys)))
            cnt, cin = got["counts"], got["in_counts"]
            sizes = sorted(set(got["members"].tolist())) if "members" in got else None
            print(f"{name}: {score}/{box} {list(keys)}: rows in {cin.tolist()} out {cnt.tolist()} cluster sizes {sizes} "
                  f"NaN scores {int(np.isnan(got['scores']).sum())} keys {sorted(got)}", flush=True)
            if not 0 < cnt[0] < cin[0]:
                raise SystemExit(f"{name}: no cluster of two or more rows on image 0 - not written")
            if not (cnt[1] == 0 and cnt[2] == cin[2] > 0):
                raise SystemExit(f"{name}: image 2 is not passed through row by row - not written")
            if sizes is not None and not {1, 2, 3} <= set(sizes):
                raise SystemExit(f"{name}: clusters of 1, 2 and 3 rows do not all occur - not written")
            for k, v in got.items():
                rec[f"{name}_out_{k}"] = v
            if idx in LATE:
                late = late_rows(late_fusion(j1, [score, box], **options(nd, keys)))
                if late["len"].tolist() != [6 if Q in keys else 3, 0, 6 if Q in keys else 3]:
                    raise SystemExit(f"{name}: late_fusion answered images {late['len'].tolist()} - not written")
                for k, v in late.items():
                    rec[f"{name}_late_{k}"] = v
    z["recorded_index"], z["recorded"] = pack(rec)
    back = unpack(z["recorded_index"], z["recorded"])
    assert all(back[k].dtype == v.dtype and back[k].shape == v.shape and back[k].tobytes() == v.tobytes() for k, v in rec.items())
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
