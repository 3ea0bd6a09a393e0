"""pe_pdq_pair_quality (csrc/pdq.hip) on the GPU, through the C-ABI, against the dense restatement tests/pdq_ref.py:
each of q, fg, bg and label within the bound carried from the sums (pdq_ref.sum_bound, pdq_ref.output_bounds; the per-term allowance
pdq_ref.C_TERM is measured here against 50-digit arithmetic), counts, flags and gt_live exactly, two launches bit for bit; then
pdq.pdq_from_predictions and the command line end to end against the reference pipeline (pdq_ref + SciPy's assignment).

Every case: images of at most 96 x 64, at most 3 images, 4 ground truths and 6 detections per image, K = 3 - but for the one case at
W + H = 4096."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import pdq_ref as R

pytestmark = pytest.mark.gpu

K = 3
TAU = 0.0027
SENTINEL = -777.25
PAD = 8


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def image(H, W, dets, gts, lp=None):
    """dets: (box, var[, the class it is sure of]); gts: (box, class[, crowd])."""
    M = len(dets)
    if lp is None:
        z = np.full((M, K + 1), -50.0)
        for i, d in enumerate(dets):
            z[i, d[2] if len(d) > 2 else 0] = 50.0
        lp = log_softmax(z)
    return dict(H=H, W=W, det_boxes=np.array([d[0] for d in dets], dtype=np.float64).reshape(-1, 4),
                det_vars=np.array([d[1] for d in dets], dtype=np.float64).reshape(-1), det_lp=np.asarray(lp, dtype=np.float64).reshape(M, K + 1),
                gt_boxes=np.array([g[0] for g in gts], dtype=np.float64).reshape(-1, 4), gt_classes=np.array([g[1] for g in gts], dtype=np.int32),
                gt_crowd=np.array([g[2] if len(g) > 2 else 0 for g in gts], dtype=np.int32))


def launch(images, tau=TAU, weights=None):
    """One pe_pdq_pair_quality call over `images` with every output inside PAD sentinels on either side; the pads are checked here.
    Returns (per image {"q", "fg", "bg", "label"} [G_b, M_b] and "gt_live" [G_b], flags [4], the raw output tensors)."""
    from proben_amd import _lib
    cat = lambda k, shape, dt: np.concatenate([np.asarray(im[k], dtype=dt).reshape(shape) for im in images]) if images else np.zeros(shape, dt)  # noqa: E731
    doff = np.concatenate([[0], np.cumsum([len(im["det_vars"]) for im in images])]).astype(np.int32)
    goff = np.concatenate([[0], np.cumsum([len(im["gt_classes"]) for im in images])]).astype(np.int32)
    poff = np.concatenate([[0], np.cumsum(np.diff(goff).astype(np.int64) * np.diff(doff))]).astype(np.int64)
    hw = np.array([[im["H"], im["W"]] for im in images], dtype=np.int32).reshape(-1, 2)
    M, G, B, n = int(doff[-1]), int(goff[-1]), len(images), int(poff[-1])
    t = {"boxes": dev(cat("det_boxes", (-1, 4), np.float64)), "vars": dev(cat("det_vars", (-1,), np.float64)),
         "lp": dev(cat("det_lp", (-1, K + 1), np.float64)), "doff": dev(doff), "gt": dev(cat("gt_boxes", (-1, 4), np.float64)),
         "cls": dev(cat("gt_classes", (-1,), np.int32)), "crowd": dev(cat("gt_crowd", (-1,), np.int32)), "goff": dev(goff), "hw": dev(hw),
         "poff": dev(poff)}
    out = {k: torch.full((n + 2 * PAD,), SENTINEL, dtype=torch.float64, device="cuda") for k in ("q", "fg", "bg", "label")}
    live = torch.full((G + 2 * PAD,), -9, dtype=torch.int32, device="cuda")
    flags = torch.full((4 + 2 * PAD,), -9, dtype=torch.int32, device="cuda")
    at = lambda x, size: ctypes.c_void_p(x.data_ptr() + PAD * size)      # noqa: E731
    p = lambda x: _lib.ptr(x) if x.numel() else None      # noqa: E731
    w = None if weights is None else (ctypes.c_float * 4)(*weights)
    st = _lib.lib().pe_pdq_pair_quality(p(t["boxes"]), p(t["vars"]), p(t["lp"]), p(t["doff"]), p(t["gt"]), p(t["cls"]), p(t["crowd"]), p(t["goff"]),
                                        p(t["hw"]), p(t["poff"]), B, K, M, G, n, int((hw[:, 0] + hw[:, 1]).max()) if B else 0, w, tau,
                                        at(out["q"], 8), at(out["fg"], 8), at(out["bg"], 8), at(out["label"], 8), at(live, 4), at(flags, 4),
                                        _lib.stream())
    _lib.check(st, "pe_pdq_pair_quality")
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    lv, fl = live.cpu().numpy(), flags.cpu().numpy()
    for k, v in host.items():
        assert (v[:PAD] == SENTINEL).all() and (v[n + PAD:] == SENTINEL).all(), f"{k}: a write outside its {n} pairs"
        assert not (v[PAD:n + PAD] == SENTINEL).any(), f"{k}: a pair was left unwritten"
    assert (lv[:PAD] == -9).all() and (lv[G + PAD:] == -9).all() and (fl[:PAD] == -9).all() and (fl[4 + PAD:] == -9).all()
    res = []
    for b, im in enumerate(images):
        Gb, Mb = goff[b + 1] - goff[b], doff[b + 1] - doff[b]
        r = {k: host[k][PAD + poff[b]:PAD + poff[b + 1]].reshape(Gb, Mb) for k in host}
        r["gt_live"] = lv[PAD + goff[b]:PAD + goff[b + 1]]
        res.append(r)
    return res, fl[PAD:PAD + 4].tolist(), host


def compare(images, tau=TAU, weights=None):
    """The kernel against the reference on `images`: every output of every pair within its bound, the rest exactly.  Returns the results
    of both and the largest observed fraction of a bound."""
    got, flags, _ = launch(images, tau, weights)
    want, wflags = R.pair_quality(images, K, tau, weights or (10.0, 10.0, 5.0, 5.0))
    assert flags == wflags, (flags, wflags)          # the counts, and 1 + the LAST index of each kind (an integer maximum: exact)
    worst = 0.0
    for b, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g["gt_live"], w["gt_live"])
        for k in ("q", "fg", "bg", "label"):
            diff, bound = np.abs(g[k] - w[k]), w["bound"][k]
            assert (diff <= bound).all(), f"image {b} {k}: {g[k].ravel().tolist()} against {w[k].ravel().tolist()}, bound {bound.ravel().tolist()}"
            if diff.size:
                worst = max(worst, float((diff / np.where(bound > 0, bound, 1.0)).max()))
    return got, want, flags, worst


def random_images(seed=7):
    """3 images of 96 x 64, 4 ground truths and 6 detections each: boxes around the ground truth and elsewhere, variances over three
    decades (1e-2 .. 1e1), label distributions from random logits."""
    rng = np.random.default_rng(seed)
    images = []
    for b in range(3):
        gts, dets = [], []
        for g in range(4):
            x1, y1 = rng.uniform(0, 70), rng.uniform(0, 45)
            box = [x1, y1, x1 + rng.uniform(4, 25), y1 + rng.uniform(4, 18)]
            gts.append((box, int(rng.integers(0, K))))
            dets.append(((np.array(box) + rng.normal(0, 1.5, 4)).tolist(), 10.0 ** rng.uniform(-2, 1)))
        for _ in range(2):
            x1, y1 = rng.uniform(0, 70), rng.uniform(0, 45)
            dets.append(([x1, y1, x1 + rng.uniform(4, 25), y1 + rng.uniform(4, 18)], 10.0 ** rng.uniform(-2, 1)))
        images.append(image(64, 96, dets, gts, lp=log_softmax(rng.normal(0, 2, (6, K + 1)))))
    return images


def hard_images():
    gts = [([10, 8, 40, 30], 1), ([50, 20, 70, 60], 2)]
    dets = [([10, 8, 40, 30], 0.0, 1), ([50, 20, 70, 60], 0.0, 2), ([14, 8, 44, 30], 0.0, 1), ([50, 24, 70, 64], 0.0, 2)]
    return [image(64, 96, dets, gts)]


def half_edge_images():
    gts = [([10.5, 4.5, 20.5, 9.5], 0), ([30.5, 10.0, 31.5, 11.0], 1)]
    dets = [([10, 4, 21, 10], 0.0, 0), ([10.5, 4.5, 20.5, 9.5], 0.5, 0), ([30, 10, 32, 11], 0.0, 1)]
    return [image(64, 96, dets, gts)]


def outside_images():
    gts = [([-12.3, -5.0, 20.2, 14.7], 0), ([80.4, 50.1, 120.0, 90.0], 1), ([100, 10, 130, 40], 2), ([-30, -30, -1, -2], 0), ([5, 70, 30, 90], 1)]
    dets = [([-10.0, -6.0, 22.0, 15.0], 2.0, 0), ([78.0, 48.0, 125.0, 93.0], 0.7, 1), ([-40, 20, -5, 40], 1.0, 2), ([90, 5, 140, 45], 0.0, 2)]
    return [image(64, 96, dets, gts[:4]), image(64, 96, dets[:2], gts[4:] + gts[:1])]


def size_images():
    gts = [([33.2, 21.3, 34.1, 22.4], 0), ([0, 0, 96, 64], 1), ([-5, -5, 200, 200], 2)]
    dets = [([30, 18, 38, 26], 1.0, 0), ([2, 1, 95, 63], 0.3, 1), ([33, 21, 35, 23], 0.0, 0), ([40, 30, 60, 50], 1e4, 2),
            ([20, 10, 50, 40], 1e-8, 1), ([20.3, 10.7, 50.2, 40.9], 3e-7, 2)]
    return [image(64, 96, dets, gts)]


def empty_images():
    a = random_images(3)
    a[0] = image(64, 96, [], [g for g in zip(a[0]["gt_boxes"].tolist(), a[0]["gt_classes"].tolist())])
    a[2] = image(64, 96, [(b, v) for b, v in zip(a[2]["det_boxes"].tolist(), a[2]["det_vars"].tolist())], [], lp=a[2]["det_lp"])
    return a


def bad_images():
    good = ([10, 8, 40, 30], 0.5, 1)
    dets = [good, ([float("nan"), 8, 40, 30], 0.5, 1), good, ([10, 8, 10, 30], 0.5, 1), ([12, 9, 41, 33], -1e-3, 1), good]
    gts = [([10, 8, 40, 30], 1), ([10, 8, 40, 30], 1, 1), ([10, 8, 40, 30], 3), ([10, 8, 40, 30], -1)]
    more = [([5, 5, 50, 50], float("inf"), 0), ([5, 5, float("inf"), 50], 1.0, 0), ([5, 50, 50, 5], 1.0, 0), ([5, 5, 50, 50], float("nan"), 0)]
    return [image(64, 96, dets, gts), image(64, 96, more, [([5, 5, 50, 50], 0), ([5, float("nan"), 50, 50], 0)])]


CASES = {"random": random_images, "hard": hard_images, "half_edges": half_edge_images, "outside": outside_images, "sizes": size_images,
         "empty": empty_images, "bad": bad_images}


@pytest.fixture(scope="module")
def reference():
    """name -> (images, the reference's results and flags), computed once."""
    return {}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_quality_against_the_reference(name):
    images = CASES[name]()
    got, want, flags, worst = compare(images)
    print(f"{name}: largest difference of an output {worst:.3f} of its bound; flags {flags}")
    if name == "hard":
        # hard boxes on integer coordinates equal to the ground truth, logits +-50: q is 1.0 exactly; four pixels off: the log eps terms
        g = got[0]
        assert g["q"][0, 0] == 1.0 and g["q"][1, 1] == 1.0 and g["fg"][0, 0] == 1.0 and g["bg"][0, 0] == 1.0 and g["label"][0, 0] == 1.0
        n, off = 30 * 22, 4 * 22
        fg = math.exp(off * math.log(1e-14) / n)
        assert abs(g["fg"][0, 2] - fg) <= 1e-12 * fg and abs(g["bg"][0, 2] - fg) <= 1e-12 * fg and abs(g["q"][0, 2] - fg) <= 1e-12 * fg
        assert 0 < g["q"][0, 1] < 1e-30          # another class (Q_L = exp(-100)), no pixel in common
    if name == "half_edges":
        # x1g = 10.5 includes pixel 10, x2g = 20.5 excludes pixel 20: the hard box [10, 21] x [4, 10] claims 11 x 6, the ground truth 10 x 5
        g = got[0]
        assert g["fg"][0, 0] == 1.0
        bg = math.exp((11 * 6 - 10 * 5) * math.log(1e-14) / 50)
        assert abs(g["bg"][0, 0] - bg) <= 1e-12 * bg
        assert g["gt_live"].tolist() == [1, 1] and g["fg"][1, 2] == 1.0          # the 1 x 1 box [30.5, 31.5) x [10, 11): pixel (10, 30)
    if name == "outside":
        assert got[0]["gt_live"].tolist() == [1, 1, 0, 0] and got[1]["gt_live"].tolist() == [0, 1] and flags[2] == 3
        assert flags[3] == 5 and (got[0]["q"][2:] == 0).all() and (got[0]["q"][:2] > 0).all()
    if name == "sizes":
        assert got[0]["gt_live"].tolist() == [1, 1, 1] and flags == [0, 0, 0, 0]
    if name == "empty":
        assert got[0]["q"].shape == (4, 0) and got[2]["q"].shape == (0, 6) and got[1]["q"].shape == (4, 6) and (got[1]["q"] > 0).all()
    if name == "bad":
        g = got[0]
        assert flags[0] == 3 + 4 and flags[1] == 6 + 4 and flags[2] == 3 + 1 and flags[3] == 6
        assert g["gt_live"].tolist() == [1, 0, 0, 0] and got[1]["gt_live"].tolist() == [1, 0]
        for k in ("q", "fg", "bg", "label"):
            assert (g[k][:, [1, 3, 4]] == 0).all() and (g[k][1:] == 0).all() and (got[1][k] == 0).all()
        assert g["q"][0, 0] == g["q"][0, 2] == g["q"][0, 5] > 0.3          # the neighbours of the excluded rows are untouched


def test_table_limit_one_detection_one_ground_truth():
    """W + H = 4096, the most the tables hold (64 KiB of them beside the reduction's 4 KiB: the kernel asks for the larger LDS)."""
    images = [image(96, 4000, [([1500.3, 20.2, 1620.8, 70.9], 1.5, 2)], [([1498.0, 18.0, 1625.0, 75.0], 2)])]
    got, want, flags, worst = compare(images)
    print(f"W + H = 4096: largest difference of an output {worst:.3f} of its bound; q = {got[0]['q'][0, 0]:.6f}")
    assert flags == [0, 0, 0, 0] and 0.0 < got[0]["q"][0, 0] < 1.0


def test_other_box_weights_and_support():
    images = random_images(5)[:1]
    _, _, _, w1 = compare(images, tau=0.0, weights=(10.0, 10.0, 5.0, 5.0))
    _, _, _, w2 = compare(images, tau=0.2, weights=(4.0, 6.0, 2.0, 3.0))
    print(f"tau 0 and tau 0.2 with other box weights: largest difference {max(w1, w2):.3f} of its bound")


def test_two_launches_are_bit_identical():
    images = random_images() + size_images()
    a, b = launch(images)[2], launch(images)[2]
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_term_error_against_fifty_digits():
    """The per-term allowance of the bound: the largest error, in units of 2^-53 relative, of a foreground or background term of the
    kernel (pe_test_pdq_terms: the kernel's own device functions) against mpmath at 50 digits, over pixels of the cases above - every
    third column and row of every soft detection.  pdq_ref.C_TERM is twice the figure recorded in DESIGN.md section 30 and must be at
    least twice what is measured here."""
    import mpmath as mp
    from proben_amd import _lib
    mp.mp.dps = 50
    ax, bx, ay, by = [], [], [], []
    for name in ("random", "half_edges", "outside", "sizes"):
        for im in CASES[name]():
            for box, var in zip(im["det_boxes"], im["det_vars"]):
                if R.excluded(box, var) or var == 0:
                    continue
                sx, sy = R.sigmas(box, var)
                a, b = R.axis_arguments(box[0], box[2], sx, im["W"])
                c, d = R.axis_arguments(box[1], box[3], sy, im["H"])
                uu, vv = np.meshgrid(np.arange(0, im["W"], 3), np.arange(0, im["H"], 3))
                ax.append(a[uu.ravel()]); bx.append(b[uu.ravel()]); ay.append(c[vv.ravel()]); by.append(d[vv.ravel()])
    ax, bx, ay, by = (np.concatenate(x) for x in (ax, bx, ay, by))
    n = ax.size
    out_fg, out_bg = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    L = _lib.test_hooks()
    args = [dev(x) for x in (ax, bx, ay, by)]          # held until the results are back
    st = L.pe_test_pdq_terms(*[_lib.ptr(x) for x in args], n, _lib.ptr(out_fg), _lib.ptr(out_bg), _lib.stream())
    _lib.check(st, "pe_test_pdq_terms")
    fg, bg = out_fg.cpu().numpy(), out_bg.cpu().numpy()
    half, root2, eps = mp.mpf(0.5), mp.sqrt(2), mp.mpf(1e-14)
    cache = {}

    def side(a, b):
        key = (a, b)
        if key not in cache:
            pa = half * mp.erfc(-mp.mpf(a) / root2)
            cache[key] = (pa * half * mp.erfc(-mp.mpf(b) / root2), half * mp.erfc(mp.mpf(a) / root2) + pa * half * mp.erfc(mp.mpf(b) / root2))
        return cache[key]

    worst, at = 0.0, None
    for i in range(n):
        (pxi, qxi), (pyi, qyi) = side(ax[i], bx[i]), side(ay[i], by[i])
        P, Q = pxi * pyi, qxi + pxi * qyi
        tf = mp.log1p(-Q) if P > half else mp.log(max(P, eps))
        tb = mp.log1p(-P) if Q > half else mp.log(max(Q, eps))
        for got, exact in ((fg[i], tf), (bg[i], tb)):
            if abs(exact) < mp.mpf(1e-300):
                continue                      # next to the subnormal range a relative error says nothing
            e = float(abs(mp.mpf(float(got)) - exact) / (abs(exact) * mp.mpf(R.U)))
            if e > worst:
                worst, at = e, (float(ax[i]), float(bx[i]), float(ay[i]), float(by[i]), float(got))
    print(f"largest error of a term over {n} pixels: {worst:.3f} x 2^-53 relative at (ax, bx, ay, by, term) = {at}; C_TERM = {R.C_TERM}")
    assert 2 * worst <= R.C_TERM


# ---- end to end

def dataset(tmp_path):
    """A FLIR val folder (annotations only) of 3 images of 96 x 64 and two prediction files over it."""
    rng = np.random.default_rng(21)
    root = tmp_path / "val"
    root.mkdir()
    images, anns, preds = [], [], [{k: [] for k in ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")} for _ in range(2)]
    for i in range(3):
        images.append({"id": 10 + i, "file_name": f"thermal_8_bit/FLIR_{i:05d}.jpeg", "height": 64, "width": 96})
        boxes = []
        for g in range(3):
            x, y, w, h = 4 + 30 * g, 6 + 10 * ((g + i) % 3), 12 + 3 * g, 10 + 2 * i
            boxes.append(([x, y, x + w, y + h], (g + i) % 3))
            anns.append({"id": len(anns) + 1, "image_id": 10 + i, "category_id": 1 + (g + i) % 3, "bbox": [x, y, w, h], "area": w * h,
                         "iscrowd": 1 if (i, g) == (2, 2) else 0})
        for f, (noise, var) in enumerate(((1.0, 0.8), (2.5, 0.2))):
            rows = [(np.array(b) + rng.normal(0, noise, 4), c) for b, c in boxes] + [(np.array([60.0, 40, 80, 58]) + rng.normal(0, 2, 4), 0)]
            logits = rng.normal(0, 1, (len(rows), K + 1)).astype(np.float32)
            for r, (_, c) in enumerate(rows):
                if r == 1:
                    logits[r], logits[r, c] = 0.0, 0.6          # one row at p = 0.38: between the two thresholds
                else:
                    logits[r, c] += 3.0
            p = np.exp(log_softmax(logits))
            cls = [c for _, c in rows]
            pr = preds[f]
            pr["image"].append(images[-1]["file_name"]); pr["image_id"].append(10 + i)
            pr["boxes"].append([b.tolist() for b, _ in rows]); pr["classes"].append(cls)
            pr["scores"].append([float(p[r, c]) for r, c in enumerate(cls)]); pr["class_logits"].append(logits.tolist())
            pr["probs"].append(p[:, :K].tolist()); pr["vars"].append([[var * (1 + 0.1 * r)] for r in range(len(rows))])
    cats = [{"id": 1, "name": "person"}, {"id": 2, "name": "bicycle"}, {"id": 3, "name": "car"}]
    json.dump({"images": images, "annotations": anns, "categories": cats}, open(root / "FLIR_thermal_RGBT_pairs_val.json", "w"))
    files = []
    for f, name in enumerate(("val_thermal_only_predictions.json", "val_early_fusion_predictions.json")):
        files.append(str(tmp_path / name))
        json.dump(preds[f], open(files[-1], "w"))
    return root, files, preds


def reference_images(records, pred, T, s):
    """The reference's image dicts for a prediction dict, with the label distributions the product computes (calibration.log_posterior_rows)."""
    from proben_amd import calibration
    out = []
    for i, r in enumerate(records):
        n = len(pred["boxes"][i])
        lp = calibration.log_posterior_rows(pred["class_logits"][i], T) if n else np.zeros((0, K + 1))
        cls = np.asarray(pred["classes"][i], dtype=np.int64)
        gts = [([a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]], a["category_id"], a["iscrowd"])
               for a in r["annotations"]]
        im = image(r["height"], r["width"], [(b, v[0] * s) for b, v in zip(pred["boxes"][i], pred["vars"][i])], gts, lp=lp)
        im["scores"] = np.exp(lp[np.arange(n), cls])
        out.append(im)
    return out


def test_pdq_from_predictions_against_the_reference_pipeline(tmp_path):
    from proben_amd import pdq
    from proben_amd.data import load_coco_json
    root, files, preds = dataset(tmp_path)
    records = load_coco_json(str(root / "FLIR_thermal_RGBT_pairs_val.json"), str(root / "thermal_8_bit"))
    worst = {}
    for pred, T, s in ((preds[0], 1.0, 1.0), (preds[1], 1.7, 2.5)):
        run = pdq.pdq_from_predictions(records, pred, T, s, score_thresh=(0.5, 0.2))
        assert run["score_thresh"] == [0.2, 0.5] and run["image_ids"] == [10, 11, 12] and run["num_classes"] == K
        images = reference_images(records, pred, T, s)
        # the reference sees every row; the product launched the rows at or above the smallest threshold: the same assignment problem
        for ti, th in enumerate(run["score_thresh"]):
            rec, bound, value = R.pdq(images, K, TAU, th)
            got = run["per_image"][ti]
            np.testing.assert_array_equal(got[:, 1:4], rec[:, 1:4])
            n = max(rec[:, 1:4].sum(), 1)
            assert abs(run["summary"][ti]["pdq"] - value) <= bound[0] / n + 2 * R.U * value
            # every column of the records within its carried bound; an image's record adds at most 3 pairs, two roundings on either
            # side, each relative to at most the image's total: 4 U of the column's total
            for col in (0, 4, 5, 6, 7):
                diff, allowed = np.abs(got[:, col] - rec[:, col]).sum(), bound[col] + 4 * R.U * rec[:, col].sum()
                assert diff <= allowed, (th, pdq.RECORD[col], diff, allowed)
                worst[pdq.RECORD[col]] = max(worst.get(pdq.RECORD[col], 0.0), diff / allowed)
            assert rec[:, 1].sum() >= 3
        assert run["flags"]["ignored_ground_truths"] == 1 and run["flags"]["excluded_detections"] == 0 and run["live_ground_truths"] == 8
        assert run["detections"][0] > run["detections"][1] and run["flags"]["unscored_rows"] == 0
    print("records against the reference pipeline, largest difference of a column as a fraction of its bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_command_line_two_files(tmp_path, capsys):
    from proben_amd.cli import pdq as cli
    root, files, preds = dataset(tmp_path)
    cal = tmp_path / "calibration.json"
    json.dump({"detectors": {"thermal_only": 1.3, "early_fusion": 0.8}, "variance_scales": {"thermal_only": 1.5, "early_fusion": 0.6}}, open(cal, "w"))
    out = tmp_path / "report.json"
    cli.main(["--dataset_path", str(root), "--predictions", files[0], files[1], "--calibration", str(cal), "--score_thresh", "0.5,0.2",
              "--replicates", "300", "--seed", "4", "--out", str(out)])
    text = capsys.readouterr().out
    rep = json.load(open(out))
    assert "PDQ" in text and "val_early_fusion_predictions.json - val_thermal_only_predictions.json" in text
    assert rep["a"]["temperature"] == 1.3 and rep["b"]["variance_scale"] == 0.6 and rep["score_thresh"] == [0.2, 0.5]
    for key in "ab":
        assert rep[key]["flags"]["ignored_ground_truths"] == 1 and len(rep[key]["thresholds"]) == 2
        for row in rep[key]["thresholds"]:
            assert 0.0 < row["pdq"]["point"] < 1.0 and row["pdq"]["lo"] <= row["pdq"]["hi"]
            assert row["tp"] + row["fp"] + row["fn"] == row["detections"] + rep[key]["live_ground_truths"] - row["tp"]
    for ti, row in enumerate(rep["paired"]):
        d = row["pdq"]
        assert d["point"] == rep["b"]["thresholds"][ti]["pdq"]["point"] - rep["a"]["thresholds"][ti]["pdq"]["point"]
        assert d["lo"] <= d["point"] <= d["hi"] and 0.0 <= d["p"] <= 1.0


def test_perfect_hard_boxes_score_one_and_a_temperature_costs():
    """Detections equal to the ground truth, hard boxes, logits +-50: PDQ is 1.0 exactly.  At a temperature of 4 the same file scores
    strictly less - every box, score order and class unchanged: a change AP cannot see."""
    from proben_amd import pdq
    records, pred = [], {k: [] for k in ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")}
    for i in range(3):
        boxes = [[4 + 20 * g, 6 + 5 * i, 16 + 20 * g, 30 + 5 * i] for g in range(3)]
        cls = [(g + i) % K for g in range(3)]
        records.append({"file_name": f"{i}.jpeg", "height": 64, "width": 96, "image_id": i, "annotations": [
            {"bbox": [b[0], b[1], b[2] - b[0], b[3] - b[1]], "category_id": c, "iscrowd": 0} for b, c in zip(boxes, cls)]})
        logits = np.full((3, K + 1), -50.0)
        logits[np.arange(3), cls] = 50.0
        pred["image"].append(f"{i}.jpeg"); pred["image_id"].append(i); pred["boxes"].append(boxes); pred["classes"].append(cls)
        pred["scores"].append([1.0] * 3); pred["class_logits"].append(logits.tolist()); pred["probs"].append(np.eye(K + 1)[cls][:, :K].tolist())
        pred["vars"].append([[0.0]] * 3)
    one = pdq.pdq_from_predictions(records, pred)
    assert one["summary"][0]["pdq"] == 1.0 and one["summary"][0]["tp"] == 9 and one["summary"][0]["fp"] == 0 and one["summary"][0]["fn"] == 0
    assert (one["per_image"][0][:, 0] == 3.0).all()
    warm = pdq.pdq_from_predictions(records, pred, temperature=4.0)
    assert warm["summary"][0]["pdq"] < 1.0 and warm["summary"][0]["tp"] == 9 and warm["summary"][0]["spatial"] == 1.0
    # a file of a conventional method (no logits, no probabilities, the schema's placeholder variance): the spread and hard boxes
    plain = dict(pred, class_logits=[[[] for _ in range(3)]] * 3, probs=[[[] for _ in range(3)]] * 3, vars=[[[1.0]] * 3] * 3, scores=[[0.8] * 3] * 3)
    conv = pdq.pdq_from_predictions(records, plain)
    assert conv["summary"][0]["spatial"] == 1.0 and abs(conv["summary"][0]["pdq"] - math.sqrt(0.8)) <= 8 * R.U
