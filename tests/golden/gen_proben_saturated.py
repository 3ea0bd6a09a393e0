"""Generate tests/golden/proben_saturated.npz by running the REFERENCE's own
``fusion`` (demo/FLIR/demo_probEn.py:189-196) on the inputs where ProbEn's
arithmetic sits on an edge - the ones a trained box head produces and the
Dirichlet rows of gen_proben.py never reach:

  * saturated probabilities: f32 softmax of K+1 logits (foreground margins
    8-25), rows whose float64 sum(p) is below 1, exactly 1 (log 0 = -inf) and
    above 1 (NaN; the smallest such sums the search meets), in clusters of 1, 2
    and >= 8 rows, one NaN member among finite ones; score = max p, class = argmax;
  * scores of exactly 1.0f from two and three detectors;
  * integer boxes at IoU exactly 0.5 under the "+1" area rule, and one float32
    ulp above / below;
  * zero- and negative-area boxes (inter / union = 0 / 0: neither matched nor kept);
  * boxes outside 640 x 512 whose class-band shift overlaps the next class's band;
  * variances of 1e-6 and 1e6 (v-avg), three-detector clusters;
  * the binary form (K = 1, demo_probEn.py:24-30) with scores of exactly 0 and 1.

Run in the build container only:  python tests/golden/gen_proben_saturated.py
The reference sorts with ``scores.argsort()[::-1]`` (unstable, build-dependent
order of ties above 16 elements): ties are kept to images of <= 16 rows, and the
generator refuses to write unless the reference's order equals
oracle.proben.order_desc on every image.  The .npz holds inputs and the
reference's outputs (data only); the output is deterministic.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gen_proben import to_info  # noqa: E402
from ref_harness import load_reference_proben  # noqa: E402

from oracle.proben import order_desc  # noqa: E402

SCORE = ["probEn", "avg", "max"]
BOX = ["v-avg", "s-avg", "avg", "argmax"]
K = 3
F32 = np.float32


def softmax_f32(logits):
    """The box head's softmax in float32 (csrc/boxhead.hip): max-subtract, exp, left-to-right sum over the K+1 columns, divide."""
    x = (logits - logits.max(1, keepdims=True)).astype(F32)
    e = np.exp(x).astype(F32)
    s = np.zeros(len(x), F32)
    for k in range(x.shape[1]):
        s = (s + e[:, k]).astype(F32)
    return (e / s[:, None]).astype(F32)


def saturated_pools(rng):
    """Softmax rows (K foreground columns) by the float64 left-to-right sum of the foreground probabilities: below 1, exactly 1, and the
    smallest sums above 1 found (1 + 2^-52 when the search meets one); plus rows whose max is exactly 1.0f."""
    below, exact, over, one = [], [], [], []
    for _ in range(8):
        n = 1 << 21
        c = rng.integers(0, K, n)
        m = rng.uniform(8.0, 25.0, n)
        lg = np.empty((n, K + 1))
        lg[:, :K] = m[:, None] - rng.uniform(8.0, 25.0, (n, K))
        lg[:, K] = m - rng.uniform(14.0, 20.0, n)
        lg[np.arange(n), c] = m
        p = softmax_f32(lg.astype(F32))[:, :K]
        pd = p.astype(np.float64)
        s = pd[:, 0] + pd[:, 1] + pd[:, 2]
        below.append(p[(s < 1.0) & (s > 1.0 - 1e-6)][:64])
        exact.append(p[s == 1.0])
        over.append(p[(s > 1.0) & (s <= 1.0 + 1e-12)])
        one.append(p[(p.max(1) == F32(1.0)) & (s > 1.0)][:32])
    cat = lambda xs: np.concatenate(xs)  # noqa: E731
    over = cat(over)
    so = over.astype(np.float64).sum(1)
    over = over[np.argsort(so, kind="stable")]
    return cat(below), cat(exact), over[:64], cat(one)


def det(boxes, probs, var=None, score=None, cls=None):
    """One detector's list: f32-valued float64 arrays like the JSON of demo_FLIR_save_predictions.py."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    probs = np.asarray(probs, F32).astype(np.float64)
    assert probs.shape == (len(boxes), K), (probs.shape, len(boxes))
    n = len(boxes)
    var = np.full(n, 1.0) if var is None else np.asarray(var, np.float64)
    return {"bbox": boxes, "score": probs.max(1) if score is None else np.asarray(score, np.float64),
            "class": probs.argmax(1).astype(np.int64) if cls is None else np.asarray(cls, np.int64),
            "prob": probs, "vars": np.asarray(var, F32).astype(np.float64).reshape(n, 1)}


def jitter(rng, base, n, px=2):
    return np.asarray(base, np.float64)[None] + rng.integers(-px, px + 1, (n, 4)).astype(np.float64)


def onehot_probs(rng, pool, cls, n):
    """n rows of `pool` with the saturated column moved to class `cls` (the row's sum, and so its saturation class, are unchanged)."""
    rows = pool[rng.integers(0, len(pool), n)].copy()
    for r in rows:
        j = int(r.argmax())
        r[[j, cls]] = r[[cls, j]]
    return rows


def make_cases(rng):
    below, exact, over, one = saturated_pools(rng)
    assert len(exact) >= 4 and len(over) >= 4 and len(one) >= 6 and len(below) >= 16, (len(exact), len(over), len(one), len(below))
    cases = []
    # ---- saturated clusters: sizes 1, 2, 8+; each of below / exactly 1 / above 1 ----
    for pool in (below, exact, over):
        b1 = det([[20, 20, 80, 90]], onehot_probs(rng, pool, 0, 1))                                     # cluster of 1 (+ a far row)
        b2 = det([[300, 200, 360, 260], [21, 300, 81, 370]], onehot_probs(rng, pool, 1, 2))
        cases.append([b1, b2])
        pa = onehot_probs(rng, pool, 2, 1)
        pb = onehot_probs(rng, pool, 2, 1)
        cases.append([det([[100, 100, 200, 180]], pa), det([[101, 99, 201, 181]], pb)])                  # cluster of 2
        big1 = det(jitter(rng, [200, 150, 320, 260], 5), onehot_probs(rng, pool, 0, 5))                  # cluster of 10
        big2 = det(jitter(rng, [200, 150, 320, 260], 5), onehot_probs(rng, pool, 0, 5))
        cases.append([big1, big2])
    # one NaN member (sum > 1) among finite ones, in a cluster of 9 and in a cluster of 2
    mix = np.concatenate([onehot_probs(rng, below, 1, 7), onehot_probs(rng, over, 1, 1)])
    cases.append([det(jitter(rng, [50, 60, 170, 200], 4), mix[:4]), det(jitter(rng, [50, 60, 170, 200], 4), mix[4:])])
    cases.append([det([[400, 300, 480, 400]], onehot_probs(rng, over, 0, 1)), det([[401, 301, 480, 399]], onehot_probs(rng, below, 0, 1))])
    # an exactly-1 sum (log 0 = -inf) with a NaN row and a finite row in one cluster
    cases.append([det(jitter(rng, [10, 10, 110, 90], 3), np.concatenate([onehot_probs(rng, exact, 2, 1), onehot_probs(rng, below, 2, 2)])),
                  det(jitter(rng, [10, 10, 110, 90], 2), onehot_probs(rng, over, 2, 2))])
    # ---- scores of exactly 1.0f on two and three detectors ----
    cases.append([det(jitter(rng, [100, 100, 200, 200], 3), onehot_probs(rng, one, 0, 3)),
                  det(jitter(rng, [100, 100, 200, 200], 3), onehot_probs(rng, one, 0, 3))])
    cases.append([det(jitter(rng, [300, 50, 420, 170], 2), onehot_probs(rng, one, 1, 2)),
                  det(jitter(rng, [300, 50, 420, 170], 2), onehot_probs(rng, one, 1, 2)),
                  det(jitter(rng, [300, 50, 420, 170], 2), onehot_probs(rng, one, 1, 2))])
    # ---- IoU exactly 0.5 under the "+1" rule: a 10x10 box inside a 10x20 box; one float32 ulp above / below ----
    pa = onehot_probs(rng, below, 0, 6)
    lo, hi = float(np.nextafter(F32(19.0), F32(0))), float(np.nextafter(F32(19.0), F32(100)))
    cases.append([det([[0, 0, 9, 9], [100, 0, 109, 9], [200, 0, 209, 9]], pa[:3], score=[0.9, 0.91, 0.92]),
                  det([[0, 0, 9, 19], [100, 0, 109, lo], [200, 0, 209, hi]], pa[3:], score=[0.8, 0.81, 0.82])])
    # the same at a class-shifted position (class 2: +1280 / +1024), and with the larger box as the pivot
    cases.append([det([[30, 40, 39, 49], [330, 40, 339, 49 + 10]], onehot_probs(rng, below, 2, 2), score=[0.7, 0.95]),
                  det([[30, 40, 39, 59], [330, 40, 339, 49]], onehot_probs(rng, below, 2, 2), score=[0.75, 0.6])])
    # ---- degenerate boxes: zero area ("+1": x2 = x1 - 1) and negative area; 0 / 0 IoUs drop the row ----
    pd_ = onehot_probs(rng, below, 1, 6)
    cases.append([det([[50, 50, 49, 80], [200, 100, 260, 160], [400, 100, 389, 160]], pd_[:3], score=[0.9, 0.8, 0.7]),
                  det([[50, 50, 49, 80], [211, 100, 190, 160], [400, 100, 389, 160]], pd_[3:], score=[0.85, 0.95, 0.6])])
    # ---- class-band shift: a class-0 box beyond 640 x 512 lands on a class-1 box's band; negative coordinates ----
    pc = onehot_probs(rng, below, 0, 2)
    pc1 = onehot_probs(rng, below, 1, 2)
    cases.append([det([[650, 520, 720, 590], [-30, -20, 40, 50]], pc, score=[0.9, 0.8]),
                  det([[10, 8, 80, 78], [-28, -21, 41, 49]], pc1, score=[0.85, 0.7], cls=[1, 0])])
    # ---- variances of 1e-6 and 1e6 (v-avg) ----
    pv = onehot_probs(rng, below, 1, 6)
    cases.append([det(jitter(rng, [100, 200, 180, 300], 6, px=8)[:3], pv[:3], var=[1e-6, 1e6, 1.0]),
                  det(jitter(rng, [100, 200, 180, 300], 6, px=8)[:3], pv[3:], var=[1e6, 1e-6, 1e6])])
    # ---- three-detector clusters, saturated (one of each sum class per detector) ----
    cases.append([det(jitter(rng, [60, 60, 160, 140], 2), np.concatenate([onehot_probs(rng, below, 0, 1), onehot_probs(rng, exact, 2, 1)])),
                  det(jitter(rng, [60, 60, 160, 140], 2), np.concatenate([onehot_probs(rng, over, 0, 1), onehot_probs(rng, below, 0, 1)])),
                  det(jitter(rng, [60, 60, 160, 140], 2), np.concatenate([onehot_probs(rng, one, 0, 1), onehot_probs(rng, below, 0, 1)]))])
    # every row of a case's image sorted by the reference's rule: ties only in images of <= 16 rows, and in a row order for which this
    # NumPy's (unstable) argsort()[::-1] happens to give the oracle's tie rule (main() checks it again before writing)
    for ci, dets in enumerate(cases):
        s = np.concatenate([d["score"] for d in dets])
        assert len(s) <= 16 or len(np.unique(s)) == len(s), len(s)
        for _ in range(500):
            s = np.concatenate([d["score"] for d in dets])
            if np.array_equal(s.argsort()[::-1], order_desc(s)):
                break
            for d in dets:
                perm = rng.permutation(len(d["score"]))
                for k in d:
                    d[k] = d[k][perm]
        else:
            raise SystemExit(f"case {ci}: no row order found whose argsort()[::-1] follows oracle.proben.order_desc on this NumPy")
    return cases


def binary_vectors():
    """Member scores of the K = 1 form, in cluster order (matches first, pivot last): exactly 0 and exactly 1 included."""
    return [np.array(v, np.float64) for v in ([0.5, 1.0], [0.0, 0.5], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0], [0.75, 0.25, 1.0],
                                              [0.9999999403953552, 1.0], [5.960464477539063e-08, 0.0, 0.5])]


def main():
    ref = load_reference_proben()
    rng = np.random.default_rng(20261016)
    cases = make_cases(rng)
    out = {"num_cases": np.int64(len(cases))}
    for ci, dets in enumerate(cases):
        scores = np.concatenate([np.asarray(d["score"], np.float64) for d in dets])
        got = np.asarray(scores).argsort()[::-1]
        if not np.array_equal(got, order_desc(scores)):
            raise SystemExit(f"case {ci}: the reference's argsort()[::-1] differs from oracle.proben.order_desc on this NumPy - not written")
        out[f"c{ci}_ndet"] = np.int64(len(dets))
        for di, d in enumerate(dets):
            for k, v in d.items():
                out[f"c{ci}_d{di}_{k}"] = v
        infos = [to_info(d) for d in dets]
        for sm in SCORE:
            for bm in BOX:
                if sm == "max" and bm == "argmax":
                    continue  # nms_1 route needs torchvision (absent)
                with np.errstate(divide="ignore", invalid="ignore"):
                    b, s, c = ref.fusion([sm, bm], *infos)
                out[f"c{ci}_{sm}_{bm}_boxes"] = np.asarray(b, dtype=np.float64).reshape(-1, 4)
                out[f"c{ci}_{sm}_{bm}_scores"] = s.numpy().astype(np.float32)
                out[f"c{ci}_{sm}_{bm}_classes"] = c.numpy().astype(np.float32)
    vecs = binary_vectors()
    out["binary_in"] = np.concatenate(vecs)
    out["binary_len"] = np.asarray([len(v) for v in vecs], np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["binary_out"] = np.asarray([ref.bayesian_fusion(v) for v in vecs], np.float64)
    path = os.path.join(HERE, "proben_saturated.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
