"""Helpers of tests/test_lamr_bootstrap_{cpu,gpu}.py: the seeded 9-image KAIST case both files share, the explicit
duplicated dataset a bootstrap replicate stands for, the evaluator's figures on it, and a plain NumPy restatement of the rule.  Not a
test module."""
import copy
import functools

import numpy as np

DAY = 5                     # the case's day / night boundary: images 0 - 4 are day, 5 - 8 night
N_IMAGES = 9
CELLS = ((0, 9), (0, 5), (5, 9))      # all / day / night


def _gt(anns, img, box, occlusion=0, ignore=0):
    anns.append({"id": len(anns), "image_id": img, "category_id": 1, "bbox": [float(v) for v in box], "height": float(box[3]),
                 "occlusion": occlusion, "ignore": ignore})
    return anns[-1]


def _random_box(rng):
    w, h = rng.uniform(30, 50), rng.uniform(60, 120)
    return [float(round(rng.uniform(5, 330 - w), 2)), float(round(rng.uniform(5, 500 - h), 2)), float(round(w, 2)), float(round(h, 2))]


@functools.lru_cache(maxsize=None)
def case():
    """(annotation dict, result rows A, result rows B, mult [6, 9]).  Image ids 0 - 8, day_frames = 5:
      0  day    3 pedestrians, 28 seeded rows + a hand-placed true positive at 0.97
      1  day    2 pedestrians and an ignore region; 24 seeded rows, a true positive at 0.97 (ties with image 0's: tp / tp across two
                images) and a detection inside the ignore region (matched to it: neither tp nor fp)
      2  day    no ground truth, no detection: evaluateImg is None
      3  day    ground truth all ignored (one too small, one heavily occluded); 12 rows, one on the occluded box
      4  day    1 pedestrian, no detection
      5  night  2 pedestrians, 26 rows
      6  night  2 pedestrians, 24 rows, listed in the file NOT by descending score, three of them below the expanded height range:
                the published row lookup and fix_row_index differ here
      7  night  no ground truth; 18 rows, two of them tied in score (fp / fp inside one image), and the night range's top score (0.999):
                the night cell's first counted detection is an fp, 1 / N > 0.01, so the "-1 reads the last point" rule fires
      8  night  1 pedestrian; 5 rows, all below the expanded height range (55 / 1.25)
    Every image's rows are listed together; all but image 6's by descending score.  A seeded row is a jittered copy of one of the image's
    pedestrians (two of three rows; later copies of one pedestrian are duplicates, i.e. false positives) or a random box.
    File B is A without the jittered copies: of A's true positives only the two hand-placed ones of images 0 and 1 are left.
    The vectors: identity; zeros and threes (image 7 three times: its top fp straddles a reference); every night image with ground truth
    dropped (NP = 0); only day images without a detection kept (MR = 1 on all and day; the night range is empty, N = 0); image 0 at 255;
    one multinomial draw."""
    rng = np.random.default_rng(28)
    anns = []
    peds = {0: 3, 1: 2, 4: 1, 5: 2, 6: 2, 8: 1}
    for img, n in peds.items():
        for g in range(n):
            _gt(anns, img, [10 + 105 * g + float(rng.integers(0, 20)), 40 + float(rng.integers(0, 200)), 40, 60 + float(rng.integers(0, 60))])
    region = _gt(anns, 1, [400, 100, 100, 200], ignore=1)
    _gt(anns, 3, [50, 50, 30, 40])                                   # height 40 < 55
    occluded = _gt(anns, 3, [200, 100, 40, 90], occlusion=2)
    counts = {0: 28, 1: 24, 3: 12, 5: 26, 6: 24, 7: 18}
    total = sum(counts.values())
    scores = iter(((rng.permutation(total) + 1) / (total + 2.0) * 0.95).tolist())       # distinct, below the hand-placed ones
    rows, copies = {i: [] for i in range(N_IMAGES)}, set()
    for img, n in counts.items():
        gts = [a for a in anns if a["image_id"] == img and not a["ignore"] and a["occlusion"] == 0 and a["height"] >= 55]
        for j in range(n):
            if gts and j % 3 != 2:
                g = np.array(gts[j % len(gts)]["bbox"])
                box = (g + rng.normal(0, 0.05, 4) * np.array([g[2], g[3], g[2], g[3]])).round(2).tolist()
            else:
                box = _random_box(rng)
            row = {"image_id": img, "category_id": 1, "bbox": [float(v) for v in box], "score": float(next(scores))}
            if gts and j % 3 != 2:
                copies.add(id(row))
            rows[img].append(row)
    hand = lambda img, box, score: rows[img].append({"image_id": img, "category_id": 1, "bbox": [float(v) for v in box], "score": score})      # noqa: E731
    for img in (0, 1):                                               # the tp / tp tie across two images
        hand(img, next(a for a in anns if a["image_id"] == img)["bbox"], 0.97)
    hand(1, [region["bbox"][0] + 20, region["bbox"][1] + 50, 40, 80], 0.6)          # inside the ignore region
    hand(3, occluded["bbox"], 0.7)                                   # on an ignored pedestrian
    hand(7, [500, 300, 40, 80], 0.999)                               # the night range's top score: an fp
    rows[7][3]["score"] = rows[7][9]["score"]                        # fp / fp inside one image
    for j in (4, 11, 17):
        rows[6][j]["bbox"][3] = 30.0                                 # below 55 / 1.25
    for j in range(5):
        hand(8, [20 + 50 * j, 100, 20, 30 + j], 0.5 + 0.05 * j)
    results = []
    for img in range(N_IMAGES):
        results += rows[img] if img == 6 else sorted(rows[img], key=lambda r: -r["score"])
    results_b = [dict(r) for r in results if id(r) not in copies]
    results = [dict(r) for r in results]
    annotation = {"images": [{"id": i, "im_name": f"set{6 + (i >= DAY) * 3:02d}/V000/I{i:05d}", "height": 512, "width": 640} for i in range(N_IMAGES)],
                  "annotations": anns, "categories": [{"id": 1, "name": "person"}]}
    from proben_amd.bootstrap import resample_multiplicities
    mult = np.array([[1] * 9, [1, 0, 1, 3, 1, 1, 0, 3, 1], [1, 2, 1, 1, 0, 0, 0, 2, 0], [0, 0, 1, 0, 2, 0, 0, 0, 0],
                     [255, 1, 1, 1, 1, 1, 1, 1, 1], resample_multiplicities(9, 2, 28)[1].tolist()], dtype=np.int64)
    mult.setflags(write=False)
    return annotation, results, results_b, mult


def kept(row):
    """Inside the expanded height range of the Reasonable setup: the rows that make an entry of the exported list."""
    return row["bbox"][3] >= 55 / 1.25


def truncated_results(n_entries):
    """The shortest prefix of file A's rows with n_entries kept rows: the exported list then has n_entries entries."""
    results, n = case()[1], 0
    for k, r in enumerate(results):
        if n == n_entries:
            return [dict(x) for x in results[:k]]
        n += kept(r)
    assert n == n_entries, (n, n_entries)
    return [dict(x) for x in results]


def truncated_matches(n_entries, fix_row_index=False):
    from proben_amd.lamr_bootstrap import export_lamr_matches
    m = export_lamr_matches(case()[0], truncated_results(n_entries), 0, fix_row_index)
    assert len(m["list_img"]) == n_entries, (len(m["list_img"]), n_entries)
    return m


def duplicated_dataset(annotation, results, mult):
    """(annotation', results') with mult[i] adjacent copies of image i (i = position in the sorted image ids): image id * 1000 + copy
    keeps the image order with the copies adjacent; annotation ids are renumbered; every copy's result rows are contiguous and in the
    original order (the file lists an image's rows together, so the published `id - first kept id` lookup reads the same rows)."""
    ids = sorted(im["id"] for im in annotation["images"])
    assert len(mult) == len(ids)
    by_id = {im["id"]: im for im in annotation["images"]}
    images, anns, res = [], [], []
    for i, m in zip(ids, mult):
        for c in range(int(m)):
            images.append(dict(by_id[i], id=i * 1000 + c))
            anns += [dict(a, image_id=i * 1000 + c) for a in annotation["annotations"] if a["image_id"] == i]
            res += [dict(r, image_id=i * 1000 + c) for r in results if r["image_id"] == i]
    for k, a in enumerate(anns):
        a["id"] = k
    return {"images": images, "annotations": anns, "categories": copy.deepcopy(annotation["categories"])}, res


def evaluator_figures(annotation, results, img_ids, fix_row_index=False, id_setup=0):
    """KAISTPedEval itself over img_ids, read the way evaluate() and demo_LAMR_KAIST read it: (MR, the nine miss rates, recall_all) as
    float64 - MR and the miss rates -1 and recall_all -1 where accumulate leaves the cell at -1 (no non-ignored ground truth),
    recall_all nan where there is ground truth and no counted detection (yy is empty)."""
    from proben_amd.evalKAIST.evaluation_script import KAIST, KAISTPedEval
    gt = KAIST()
    gt.dataset = annotation
    gt._index()
    ev = KAISTPedEval(gt, gt.loadRes(results), "bbox")
    ev.params.fixRowIndex = bool(fix_row_index)
    ev.params.imgIds = list(img_ids)
    ev.evaluate(id_setup)
    ev.accumulate()
    mr = ev.summarize(id_setup)
    tp = ev.eval["TP"][0, :, 0, 0]
    if (tp == -1).all():
        assert mr == -1.0
        return np.float64(-1.0), np.full(len(tp), -1.0), np.float64(-1.0)
    yy = ev.eval["yy"]
    return np.float64(mr), 1 - tp, np.float64(1 - yy[0][-1] if yy and len(yy[0]) else np.nan)


@functools.lru_cache(maxsize=None)
def duplicated_figures(v, cell, fix_row_index=False, n_entries=None):
    """The exact expectation of vector v of the case on cell (index into CELLS): the evaluator on the duplicated dataset, restricted to
    the copies of the cell's images.  n_entries: on the truncated result rows.  Shared, read-only."""
    annotation, results, _, mult = case()
    if n_entries is not None:
        results = truncated_results(n_entries)
    ann2, res2 = duplicated_dataset(annotation, results, mult[v])
    lo, hi = CELLS[cell]
    ids = [im["id"] for im in ann2["images"] if lo <= im["id"] // 1000 < hi]
    mr, mrs, rec = evaluator_figures(ann2, res2, ids, fix_row_index)
    mrs.setflags(write=False)
    return mr, mrs, rec


def numpy_rule(list_img, list_flags, npig, m, cell, thr):
    """DESIGN.md section 28's rule, literally, for one multiplicity vector and one cell (lo, hi).  Returns the integers the kernel
    returns - tp_at i64 [R], totals (N, NP, TP_tot, FP_tot), valid - and, for the tests of the case's corners, pos [R], fired [R] (the
    "-1 reads the last point" rule applied) and straddle (an fp of weight >= 2 with some but not all copies below a reference)."""
    lo, hi = cell
    I, R = len(npig), len(thr)
    assert 0 <= lo <= hi <= I
    m = np.asarray(m, dtype=np.int64)
    img = np.asarray(list_img, dtype=np.int64)
    matched, ignored = (np.asarray(list_flags) & 1) != 0, (np.asarray(list_flags) & 2) != 0
    inside = (img >= lo) & (img < hi) & ~ignored
    w = np.where(inside, m[np.clip(img, 0, I - 1)], 0)
    N, NP = int(m[lo:hi].sum()), int((m[lo:hi] * npig[lo:hi]).sum())
    wf = np.where(matched, 0, w)
    F = np.cumsum(wf) - wf
    TP, FP = int(np.where(matched, w, 0).sum()), int(wf.sum())
    tp_at, pos, straddle = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64), False
    with np.errstate(divide="ignore", invalid="ignore"):
        below = lambda f: np.float64(f) / np.float64(N) <= thr                  # noqa: E731  the evaluator's division and comparison, all R at once
        for j in range(len(img)):
            if w[j] == 0:
                continue
            if matched[j]:
                b = below(F[j])
                tp_at += w[j] * b
                pos += w[j] * b
            else:
                n_below = sum(below(F[j] + k).astype(np.int64) for k in range(1, int(w[j]) + 1))
                pos += n_below
                straddle |= bool(((n_below > 0) & (n_below < w[j])).any())
    fired = np.zeros(R, dtype=bool)
    if TP + FP > 0:
        fired = pos == 0
        tp_at[fired] = TP
    if NP == 0:
        tp_at[:] = 0
    return {"tp_at": tp_at, "totals": np.array([N, NP, TP, FP], dtype=np.int64), "valid": int(NP != 0), "pos": pos, "fired": fired & (NP != 0),
            "straddle": straddle}


def rule_run(matches, mult, cells=CELLS):
    """numpy_rule over every vector and cell, in lamr_bootstrap's output layout (plus the corner flags)."""
    thr = np.asarray(matches["evaluator"].params.fppiThrs, dtype=np.float64)
    rec = [[numpy_rule(matches["list_img"], matches["list_flags"], matches["npig"], m, c, thr) for c in cells] for m in mult]
    stack = lambda k: np.array([[r[k] for r in row] for row in rec])      # noqa: E731
    return {"tp_at": stack("tp_at").astype(np.int64), "totals": stack("totals").astype(np.int64), "valid": stack("valid").astype(np.int32),
            "fired": stack("fired"), "straddle": stack("straddle"), "pos": stack("pos")}
