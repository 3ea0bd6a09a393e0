"""The inputs the probEn-log GPU tests share, each built once from a fixed seed and left unchanged, and the one fuse_batch launcher over
them: three image builders (anchor images: tests/test_posterior_gpu.py; spec rows: tests/test_presence_gpu.py; grid images:
tests/test_pool_gpu.py, test_boxcorr_gpu.py), the saturated rows of tests/test_proben_logp_gpu.py, the synthetic detectors' rows and
logit rows of tests/test_calibration_gpu.py, and the synthetic FLIR folders of the driver tests.  torch is imported inside the
functions that need it."""
import json
import os

import numpy as np

from fuse_ref import log_softmax, seq_sum


def to_dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- anchor images ------------------------------------------------------------------------------------------------------------------

# anchors 70 x 62 apart hold boxes of 60 x 50 jittered by <= 2 px: members of one anchor overlap with IoU > 0.8, anchors never meet
ANCHORS = [(4 + 70 * ix, 4 + 62 * iy) for iy in range(8) for ix in range(9)]


def anchor_image(rng, K1, sizes):
    """One image's rows (shuffled): an anchor per entry of `sizes`, that many rows of one class on it, from detectors 0 / 1 at random.
    Log-posteriors are float64 log_softmax of logits with margins from flat to saturated (up to ~40)."""
    K = K1 - 1
    n = sum(sizes)
    boxes, cls = np.empty((n, 4)), np.empty(n, np.int32)
    r = 0
    for a, size in zip(rng.permutation(len(ANCHORS))[:len(sizes)], sizes):
        x, y = ANCHORS[a]
        boxes[r:r + size] = np.array([x, y, x + 60.0, y + 50.0]) + rng.uniform(-2.0, 2.0, (size, 4))
        cls[r:r + size] = rng.integers(0, K)
        r += size
    lg = rng.normal(0.0, 3.0, (n, K1))
    lg[np.arange(n), cls] += rng.uniform(2.0, 12.0, n) * rng.choice([1.0, 3.0], n)
    lp = log_softmax(lg)
    perm = rng.permutation(n)
    boxes, cls, lp = boxes[perm], cls[perm], lp[perm]
    return {"boxes": boxes, "classes": cls, "lp": lp, "scores": np.exp(lp[np.arange(n), cls]), "vars": rng.uniform(0.5, 4.0, n),
            "src": rng.integers(0, 2, n).astype(np.int32)}


def _sizes(total):
    out, k = [], 0
    while sum(out) < total:
        out.append(min(1 + k % 6, total - sum(out)))          # clusters of 1 .. 6 rows
        k += 1
    return out


_ANCHOR_SETS = {}


def anchor_image_set(K1):
    """Images of 1, 2, 64 and 65 rows (65 crosses the 64-row word of the bit matrices), one of 0 rows, one passed through (5 rows) and
    one of 70 rows for the launches whose bound is 65 (counts == -1).  Computed once per K + 1 and left unchanged."""
    if K1 not in _ANCHOR_SETS:
        rng = np.random.default_rng(1000 + K1)
        imgs = [anchor_image(rng, K1, [1]), anchor_image(rng, K1, [2]), anchor_image(rng, K1, _sizes(64)), anchor_image(rng, K1, _sizes(65)),
                anchor_image(rng, K1, []), anchor_image(rng, K1, [2, 1, 2]), anchor_image(rng, K1, _sizes(70))]
        _ANCHOR_SETS[K1] = (imgs, [0, 0, 0, 0, 0, 1, 0])
    return _ANCHOR_SETS[K1]


# ---- spec rows ----------------------------------------------------------------------------------------------------------------------

SEQ_ROWS = {2: 1000, 4: 1000, 63: 250}         # a bound at which the bit matrices no longer fit the LDS: the sequential walk
BITS_ROWS = 12


def spec_rows(rng, K1, spec):
    """spec: [(anchor x, anchor y, class, source)]; boxes 60 x 50 jittered by <= 2 px on their anchor (rows of one anchor
    overlap with IoU > 0.8, anchors 100 px apart never meet).  Scores are the row's own p[class]."""
    n = len(spec)
    boxes = np.array([[x, y, x + 60.0, y + 50.0] for x, y, _, _ in spec]) + rng.uniform(-2.0, 2.0, (n, 4))
    cls = np.array([c for _, _, c, _ in spec], np.int32)
    lg = rng.normal(0.0, 2.0, (n, K1))
    lg[np.arange(n), cls] += rng.uniform(1.0, 6.0, n)
    lp = log_softmax(lg)
    return {"boxes": boxes, "classes": cls, "lp": lp, "scores": np.exp(lp[np.arange(n), cls]), "vars": rng.uniform(0.5, 4.0, n),
            "src": np.array([s for _, _, _, s in spec], np.int32)}


_SPEC_SETS = {}


def spec_image_set(K1, D):
    """The batch of the presence tests: (0) one row; (1) rows of one detector with the passthrough flag set, two of them overlapping
    above the gate; (2) rows of every detector: a cluster of three that holds two rows of detector 0, a cluster of two, a lone row of
    each detector; (3) a row whose NaN coordinate removes it; (4) more rows than any bound used (count -1); (5) a row with source D in a
    cluster of two, a lone row with source D and a lone row with source -1.  Computed once per (K + 1, D) and left unchanged."""
    if (K1, D) not in _SPEC_SETS:
        rng = np.random.default_rng(100 * K1 + D)
        K = K1 - 1
        c = lambda: int(rng.integers(0, K))  # noqa: E731
        c0, c1 = c(), c()
        imgs = [spec_rows(rng, K1, [(10, 10, c(), D - 1)]),
                spec_rows(rng, K1, [(10, 10, c0, 1), (10, 10, c0, 1), (210, 10, c(), 1), (410, 10, c(), 1)]),
                spec_rows(rng, K1, [(10, 10, c0, 0), (10, 10, c0, 0), (10, 10, c0, 1), (110, 10, c1, D - 1), (110, 10, c1, 0)] +
                          [(10 + 100 * d, 210, c(), d) for d in range(D)]),
                spec_rows(rng, K1, [(10, 10, c0, 0), (10, 10, c0, 1)]),
                spec_rows(rng, K1, [(10 + (i % 6) * 100, 10 + (i // 6 % 4) * 100, 0, i % D) for i in range(SEQ_ROWS[K1] + 3)]),
                spec_rows(rng, K1, [(10, 10, c0, 0), (10, 10, c0, D), (210, 10, c(), D), (410, 10, c(), -1)])]
        nan = imgs[3]
        lo = int(np.argmin(nan["scores"]))
        nan["boxes"][lo, 0] = np.nan                    # the lower-scored row: its IoU with the pivot is NaN, it leaves without a cluster
        table = rng.normal(0.0, 1.5, (2 ** D, K1))
        table[:, K] = 0.0                               # the fit's gauge; row 0 stays random: nothing may read it
        _SPEC_SETS[(K1, D)] = (imgs, [0, 1, 0, 0, 0, 0], table)
    return _SPEC_SETS[(K1, D)]


# ---- grid images --------------------------------------------------------------------------------------------------------------------

GRID = [(10 + 40 * ix, 10 + 40 * iy) for iy in range(12) for ix in range(15)]      # 180 far-apart 20 x 20 anchors inside 640 x 512


def grid_image(rng, sizes, k1, D, n_single=0, nan_row=False):
    """One image: a cluster of each size in `sizes` (+ n_single single rows) at distinct anchors, class 0, sources cycling from a random
    start, log-posteriors of random float32 logits, score = the row's own p[0] - plus, optionally, a low-score row with NaN coordinates."""
    sizes = list(sizes) + [1] * n_single
    anchors = rng.permutation(len(GRID))[:len(sizes)]
    box, src = [], []
    for a, m in zip(anchors, sizes):
        x, y = GRID[a]
        for t in range(m):
            box.append(np.array([x, y, x + 20, y + 20], np.float64) + rng.integers(-1, 2, 4))
            src.append((t + a) % D)
    n = len(box)
    box = np.asarray(box, np.float64).reshape(-1, 4)
    lp = log_softmax(rng.normal(0, 3, (n, k1)).astype(np.float32))
    score = np.exp(lp[:, 0])
    if nan_row:
        box = np.concatenate([box, [[np.nan] * 4]])
        lp = np.concatenate([lp, log_softmax(rng.normal(0, 3, (1, k1)))])
        score = np.append(score, score.min() * 0.5)
        src.append(0)
    perm = rng.permutation(len(score))
    return {"boxes": box[perm], "scores": score[perm], "lp": lp[perm], "src": np.asarray(src, np.int32)[perm],
            "vars": rng.uniform(0.5, 3.0, len(score)), "classes": np.zeros(len(score), np.int32)}


def batch(images):
    cat = lambda k: np.concatenate([im[k] for im in images])  # noqa: E731
    offs = np.concatenate([[0], np.cumsum([len(im["scores"]) for im in images])]).astype(np.int32)
    return (to_dev(cat("boxes").reshape(-1, 4)), to_dev(cat("scores")), to_dev(cat("vars")), to_dev(cat("classes")), to_dev(offs), to_dev(cat("src")),
            to_dev(cat("lp").reshape(-1, images[0]["lp"].shape[1]))), offs


# ---- the launcher ---------------------------------------------------------------------------------------------------------------------

def launch(imgs, passthrough, box, max_rows, table, prior=None, pool=None, with_posterior=True, **kw):
    """fuse_batch in score_fusion "probEn-log" over images of the three builders, every output on the host, and the offsets.  pool = the
    weight per detector or None; row_source goes along when the pool weights, the table or src=True ask for it."""
    import torch
    from proben_amd import fusion as F
    cat = lambda k, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate([i[k] for i in imgs]).astype(dt))).cuda()  # noqa: E731
    offs = torch.tensor(np.cumsum([0] + [len(i["scores"]) for i in imgs]), dtype=torch.int32).cuda()
    out = F.fuse_batch(cat("boxes", np.float64), cat("scores", np.float64), None, cat("vars", np.float64), cat("classes", np.int32), offs,
                       "probEn-log", box, max_rows=max_rows, log_probs=cat("lp", np.float64), class_prior=prior,
                       passthrough=None if passthrough is None else torch.tensor(passthrough, dtype=torch.int32).cuda(),
                       pool_weights=pool, row_source=cat("src", np.int32) if (pool is not None or table is not None or kw.get("src")) else None,
                       with_posterior=with_posterior, presence=table)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, offs.cpu().numpy()


def image_rows(out, offs, i):
    cnt = int(out["counts"][i])
    sl = slice(offs[i], offs[i] + cnt)
    return (out["keep"][sl].cpu().numpy(), out["boxes"][sl].cpu().numpy(), out["scores"][sl].cpu().numpy(), out["classes"][sl].cpu().numpy())


# ---- reference-style dicts and saturated rows -------------------------------------------------------------------------------------------

def log_full(p):
    """log([p, 1 - sum p]) in float64, the background formed as oracle.proben.fuse_score forms it (left-to-right sum)."""
    p = np.asarray(p, np.float64).reshape(len(p), -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.concatenate([p, (1.0 - seq_sum(list(p.T)))[:, None]], 1))


def fuse_logp(infos_per_image, lps_per_image, box, max_rows=None, class_prior=None):
    """fuse_batch in the log-posterior mode over images given as lists of reference-style dicts + one [n, K+1] log-posterior array per image."""
    import torch
    from proben_amd import fusion as F
    b, s, p, v, c, offs = F.pack_infos(infos_per_image)
    K1 = lps_per_image[0].shape[1]
    lp = torch.from_numpy(np.concatenate(lps_per_image).reshape(-1, K1)).cuda()
    out = F.fuse_batch(b, s, None, v, c, offs, "probEn-log", box, max_rows=max_rows, log_probs=lp, class_prior=class_prior)
    return out, offs.cpu().numpy()


def load_case(z, ci):
    return [{"img_name": "x", "bbox": z[f"c{ci}_d{di}_bbox"], "score": z[f"c{ci}_d{di}_score"], "class": z[f"c{ci}_d{di}_class"],
             "prob": z[f"c{ci}_d{di}_prob"], "vars": z[f"c{ci}_d{di}_vars"]} for di in range(int(z[f"c{ci}_ndet"]))]


K = 3
POS = [(60 + 190 * ix, 40 + 160 * iy) for iy in range(3) for ix in range(3)]      # nine far-apart anchors inside 640 x 512


def _softmax_f32(logits):
    """The box head's float32 softmax (max-subtract, exp, left-to-right sum over the K + 1 columns, divide): the recipe of
    tests/golden/gen_proben_saturated.py restated."""
    x = (logits - logits.max(1, keepdims=True)).astype(np.float32)
    e = np.exp(x).astype(np.float32)
    s = np.zeros(len(x), np.float32)
    for k in range(x.shape[1]):
        s = (s + e[:, k]).astype(np.float32)
    return (e / s[:, None]).astype(np.float32)


def _saturated_logits(rng, n):
    """Foreground margins 8-25, background 14-20 below the top (gen_proben_saturated.saturated_pools' recipe)."""
    c = rng.integers(0, K, n)
    m = rng.uniform(8.0, 25.0, n)
    lg = np.empty((n, K + 1))
    lg[:, :K] = m[:, None] - rng.uniform(8.0, 25.0, (n, K))
    lg[:, K] = m - rng.uniform(14.0, 20.0, n)
    lg[np.arange(n), c] = m
    return lg.astype(np.float32), c


_SAT = {}


def saturated_images():
    """48 images, two and three detectors alternating, each with clusters of 1, 2, 8 and 12 rows of one class at far-apart anchors.
    Per image: infos with the float32 prob_score route's numbers (prob / score = the float32 softmax, as the JSON carries them), the rows'
    logits, and the members of every cluster for the checks.  Rows are drawn so that all three float64 sums of the float32
    probabilities occur: below, exactly and above 1."""
    if _SAT:
        return _SAT
    rng = np.random.default_rng(20261016)
    # sums of exactly 1 are rare (a few per 2^21 rows): 2^24 rows are searched for them, the first 2^17 serve the two other kinds
    pool, pcls = [], []
    for chunk in range(8):
        lg, c = _saturated_logits(rng, 1 << 21)
        p = _softmax_f32(lg)[:, :K].astype(np.float64)
        hit = (p[:, 0] + p[:, 1] + p[:, 2]) == 1.0
        hit[:1 << 17] |= chunk == 0
        pool.append(lg[hit])
        pcls.append(c[hit])
    pool, pcls = np.concatenate(pool), np.concatenate(pcls)
    p32 = _softmax_f32(pool)[:, :K].astype(np.float64)
    s = p32[:, 0] + p32[:, 1] + p32[:, 2]
    kinds = {"below": np.nonzero(s < 1.0)[0], "exact": np.nonzero(s == 1.0)[0], "over": np.nonzero(s > 1.0)[0]}
    assert len(kinds["below"]) >= 1000 and len(kinds["over"]) >= 1000 and len(kinds["exact"]) >= 8, {k: len(v) for k, v in kinds.items()}
    images = []
    for b in range(48):
        kdet = 2 + b % 2
        dets = [{"bbox": [], "rows": []} for _ in range(kdet)]
        anchors = rng.permutation(len(POS))
        for a, size in zip(anchors, [1, 2, 8, 12, 2, 1, 9]):
            kind = ["below", "exact", "over", "mixed"][int(rng.integers(0, 4))]
            # a cluster has one class; the few exactly-1 rows keep theirs (moving a column would change the float32 sum)
            cls = int(pcls[kinds["exact"][rng.integers(0, len(kinds["exact"]))]]) if kind in ("exact", "mixed") else int(rng.integers(0, K))
            x, y = POS[a]
            for t in range(size):
                src = kinds[kind if kind != "mixed" else ["below", "exact", "over"][t % 3]]
                src = src[pcls[src] == cls]
                r = int(src[rng.integers(0, len(src))])
                d = dets[(t + a) % kdet]
                d["bbox"].append([x, y, x + 100, y + 80] + rng.integers(-2, 3, 4))
                d["rows"].append(r)
        infos, logits = [], []
        for d in dets:
            r = np.asarray(d["rows"], int)
            pr = _softmax_f32(pool[r])[:, :K].astype(np.float64) if len(r) else np.zeros((0, K))
            infos.append({"img_name": f"s{b}", "bbox": np.asarray(d["bbox"], np.float64).reshape(-1, 4), "score": pr.max(1) if len(r) else np.zeros(0),
                          "class": pcls[r].astype(np.int64), "prob": pr, "vars": rng.uniform(0.5, 3.0, (len(r), 1))})
            logits.append(pool[r].reshape(-1, K + 1))
        images.append((infos, np.concatenate(logits)))
    _SAT["images"] = images
    allp = np.concatenate([np.concatenate([d["prob"] for d in infos]) for infos, _ in images])
    ss = allp[:, 0] + allp[:, 1] + allp[:, 2]
    _SAT["sum_kinds"] = (int((ss < 1).sum()), int((ss == 1).sum()), int((ss > 1).sum()))
    return _SAT


def calibrated_infos(T=(1.0, 1.0, 1.0)):
    """The images with the rows the log-posterior route sees: prob / score = calibrated_probs of the logits (float64, on the device), plus
    the log-posteriors of calibration.log_posteriors - the inputs of pe_proben_fuse_batch_logp, taken as given by the restatement."""
    import torch
    from proben_amd.calibration import calibrated_probs, log_posteriors
    out = []
    for infos, logits in saturated_images()["images"]:
        new, lps, k = [], [], 0
        for d, t in zip(infos, T):
            n = len(d["score"])
            lg = torch.from_numpy(logits[k:k + n]).cuda()
            k += n
            if n == 0:
                new.append(d)
                continue
            p, _ = calibrated_probs(lg, t)
            p = p.cpu().numpy()
            new.append(dict(d, prob=p, score=p[np.arange(n), d["class"]]))
            lps.append(log_posteriors(lg, t).cpu().numpy())
        out.append((new, np.concatenate(lps)))
    return out


# ---- detector rows ----------------------------------------------------------------------------------------------------------------------

def logit_rows(rng, n, K):
    """[n, K+1] float32 logits on a 2^-12 grid spanning +-60; a fifth of the rows have an exact tie at the top, a tenth are flat."""
    lg = np.round(rng.uniform(-60.0, 60.0, (n, K + 1)) * 4096.0) / 4096.0
    narrow = rng.random(n) < 0.5                      # half the rows within a few units of their top, like a head's rows
    lg[narrow] = lg[narrow, :1] - np.round(rng.uniform(0.0, 6.0, (int(narrow.sum()), K + 1)) * 4096.0) / 4096.0
    t = rng.integers(0, K, n)
    top = lg.max(1)
    lg[np.arange(n), t] = top
    tie = rng.random(n) < 0.2
    t2 = (t + 1 + rng.integers(0, max(K - 1, 1), n)) % K
    lg[tie, t2[tie]] = top[tie]
    flat = rng.random(n) < 0.1
    lg[flat] = lg[flat, :1]
    return lg.astype(np.float32)


_DETS = {}


def detector_rows(K):
    """Two product detectors (R50, synthetic weights, K classes) on 8 synthetic frames: their forward_batch dicts."""
    if K not in _DETS:
        import torch
        import proben_amd
        from proben_amd.synthetic import synthetic_images
        frames = synthetic_images(8, height=256, width=320, seed=5)
        dets = []
        for seed in (1, 2):
            cfg = proben_amd.get_cfg()
            cfg.MODEL.RESNETS.DEPTH = 50
            cfg.MODEL.ROI_HEADS.NUM_CLASSES = K
            cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST = 0.5 if K > 1 else 0.05
            cfg.MODEL.ROI_BOX_HEAD.OUTPUT_LOGITS = True
            cfg.MODEL.ROI_HEADS.ENABLE_GAUSSIANNLLOSS = True
            cfg.MODEL.WEIGHTS = f"synthetic://{seed}"
            m = proben_amd.DefaultPredictor(cfg).model
            dets.append(m.forward_batch([torch.from_numpy(f).cuda() for f in frames], out_sizes=[(256, 320)] * 8, resize_to=(800, 1000)))
        torch.cuda.synchronize()
        assert all(int(d["counts"].sum()) > 0 for d in dets), "the synthetic detectors found nothing"
        _DETS[K] = dets
    return _DETS[K]


# ---- synthetic FLIR folders -------------------------------------------------------------------------------------------------------------

def write_flir(root, n, H, W, rgb_hw):
    """FLIR val layout (the tests/test_boundary_gpu.py pattern) with RGB frames of their own size."""
    from PIL import Image
    from proben_amd.synthetic import synthetic_images
    (root / "thermal_8_bit").mkdir(parents=True)
    (root / "RGB").mkdir()
    th, rgb = synthetic_images(n, H, W, seed=31), synthetic_images(n, rgb_hw[0], rgb_hw[1], seed=32)
    images, anns = [], []
    for i in range(n):
        Image.fromarray(th[i]).save(root / "thermal_8_bit" / f"FLIR_{i:05d}.jpeg", quality=95)
        Image.fromarray(rgb[i]).save(root / "RGB" / f"FLIR_{i:05d}.jpg", quality=95)
        images.append({"id": 10 + i, "file_name": f"thermal_8_bit/FLIR_{i:05d}.jpeg", "height": H, "width": W})
        anns.append({"id": i + 1, "image_id": 10 + i, "category_id": 1 + i % 3, "bbox": [20, 30, 60, 80], "area": 4800, "iscrowd": 0})
    json.dump({"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}, {"id": 2, "name": "bicycle"},
                                                                      {"id": 3, "name": "car"}]},
              open(root / "FLIR_thermal_RGBT_pairs_val.json", "w"))


def weights(tmp, method, seed):
    import torch
    from proben_amd.synthetic import synthetic_state_dict
    nin = {"thermal_only": 3, "early_fusion": 4, "middle_fusion": 6}[method]
    p = tmp / f"r50_{method}.pth"
    if not p.exists():
        torch.save(synthetic_state_dict(50, 3, nin, seed=seed), p)
    return str(p)


def dependent_files(tmp_path, n_img=16):
    """A FLIR val folder of n_img images and two prediction files over it, written by hand: per image 4 objects on a grid of disjoint
    30 x 35 boxes; detector 0 sees logits z0 ~ N(0, 2^2) per object, detector 1 a noisy copy z0 + N(0, 1) with detector 0's class (rows
    cluster within a class only), both with boxes within a pixel of the object's; the object's class is drawn from softmax(z0) and an
    object drawn as background gets no annotation.  Detector 0 adds one detection per image that nothing overlaps: a cluster of one.
    Returns (root, files, per image: the objects' labels in [0, 3])."""
    root = tmp_path / "val"
    write_flir(root, n_img, 96, 120, (96, 120))
    val = root / "FLIR_thermal_RGBT_pairs_val.json"
    ds = json.load(open(val))
    rng = np.random.default_rng(5)
    grid = [(5.0, 5.0), (45.0, 5.0), (5.0, 55.0), (45.0, 55.0)]
    preds = [{k: [] for k in ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")} for _ in range(2)]
    anns, labels = [], []
    for im in ds["images"]:
        z0 = rng.normal(0, 2, (4, 4)).astype(np.float32)
        p0 = np.exp(log_softmax(z0))
        lab = [int(rng.choice(4, p=p / p.sum())) for p in p0]
        labels.append(lab)
        for (x, y), l in zip(grid, lab):
            if l < 3:
                anns.append({"id": len(anns) + 1, "image_id": im["id"], "category_id": l + 1, "bbox": [x, y, 30.0, 35.0], "area": 1050.0, "iscrowd": 0})
        cls = z0[:, :3].argmax(1)
        for d, p in enumerate(preds):
            z = z0 if d == 0 else (z0 + rng.normal(0, 1, z0.shape)).astype(np.float32)
            bx = [[x + e[0], y + e[1], x + 30 + e[2], y + 35 + e[3]] for (x, y), e in zip(grid, rng.uniform(-1, 1, (4, 4)))]
            c = cls.tolist()
            if d == 0:
                z = np.concatenate([z, rng.normal(0, 2, (1, 4)).astype(np.float32)])
                bx.append([85.0, 5.0, 115.0, 40.0])
                c.append(int(z[4, :3].argmax()))
            pr = np.exp(log_softmax(z))
            p["image"].append(os.path.basename(im["file_name"]))
            p["image_id"].append(im["id"])
            p["boxes"].append(bx)
            p["classes"].append(c)
            p["class_logits"].append(z.tolist())
            p["probs"].append(pr[:, :3].tolist())
            p["scores"].append([float(pr[i, k]) for i, k in enumerate(c)])
            p["vars"].append([[0.01]] * len(bx))
    ds["annotations"] = anns
    json.dump(ds, open(val, "w"))
    pdir = tmp_path / "pred"
    pdir.mkdir()
    files = []
    for m, p in zip(("thermal_only", "early_fusion"), preds):
        files.append(str(pdir / f"val_{m}_predictions.json"))
        json.dump(p, open(files[-1], "w"))
    return root, files, preds, labels
