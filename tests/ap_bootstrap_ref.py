"""Helpers of tests/test_ap_bootstrap_{cpu,gpu}.py: the explicit duplicated dataset a bootstrap replicate stands
for, a NumPy restatement of the weighted accumulate rule, and the seeded case both test files share.  Not a test module."""
import copy
import functools

import numpy as np

SUMMARY_CELLS = ((0, 2), (1, 2), (2, 2), (3, 2), (0, 0), (0, 1))      # (area range, maxDets index): what summarize() reads


def duplicated_dataset(gt_json, results, mult):
    """(gt_json', results') with mult[i] adjacent copies of image i (i = position in the sorted image ids): image id * 1000 + copy
    keeps the image order with the copies adjacent, annotation ids are renumbered from 1, a copy's detections keep their file order."""
    ids = sorted(im["id"] for im in gt_json["images"])
    assert len(mult) == len(ids)
    m = dict(zip(ids, (int(x) for x in mult)))
    by_id = {im["id"]: im for im in gt_json["images"]}
    images, anns, res = [], [], []
    for i in ids:
        for c in range(m[i]):
            images.append(dict(by_id[i], id=i * 1000 + c))
    for a in gt_json["annotations"]:
        for c in range(m[a["image_id"]]):
            anns.append(dict(a, image_id=a["image_id"] * 1000 + c, id=len(anns) + 1))
    for r in results:
        for c in range(m[r["image_id"]]):
            res.append(dict(r, image_id=r["image_id"] * 1000 + c))
    return {"images": images, "annotations": anns, "categories": copy.deepcopy(gt_json["categories"])}, res


def numpy_records(ev):
    """What pe_cocoeval_bbox_matches exports, built from COCOevalBBox(impl="numpy")._eval_img: (list_off, list_img, list_rank,
    list_flags [A, L], npig [K, A, I])."""
    K, A, I, T = len(ev.cat_ids), len(ev.area_rng), len(ev.img_ids), len(ev.iou_thrs)
    off, img, rank, flags, npig = [0], [], [], [[] for _ in range(A)], np.zeros((K, A, I), dtype=np.int32)
    for k, cat in enumerate(ev.cat_ids):
        per = [(i, ev._eval_img(iid, cat)) for i, iid in enumerate(ev.img_ids)]
        per = [(i, e) for i, e in per if e is not None]
        scores = np.concatenate([e[0]["dt_scores"] for _, e in per] + [np.zeros(0)])
        order = np.argsort(-scores, kind="mergesort")
        img += np.concatenate([np.full(len(e[0]["dt_scores"]), i) for i, e in per] + [np.zeros(0)]).astype(int)[order].tolist()
        rank += np.concatenate([np.arange(len(e[0]["dt_scores"])) for _, e in per] + [np.zeros(0)]).astype(int)[order].tolist()
        bits = (1 << np.arange(T)).astype(np.int64)[:, None]
        for a in range(A):
            m = np.concatenate([e[a]["dtm"] != 0 for _, e in per] + [np.zeros((T, 0), bool)], axis=1)[:, order]
            g = np.concatenate([e[a]["dt_ig"] for _, e in per] + [np.zeros((T, 0), bool)], axis=1)[:, order]
            flags[a] += ((m * bits).sum(0) | ((g * bits).sum(0) << 16)).tolist()
            for i, e in per:
                npig[k, a, i] = np.count_nonzero(~e[a]["gt_ig"])
        off.append(len(img))
    return (np.array(off, np.int64), np.array(img, np.int32), np.array(rank, np.uint8),
            np.array(flags, np.uint32).reshape(A, len(img)), npig)


def weighted_accumulate(records, mult, rec_thrs, T, max_dets, only=None):
    """The rule of DESIGN.md section 27 in NumPy, over every (category, area range, maxDet): precision [T, R, K, A, M] and recall
    [T, K, A, M] as COCOevalBBox.accumulate lays them out, for the replicate that holds image i mult[i] times.  `only`: the
    (area range, maxDets index) pairs to fill; the others stay -1."""
    list_off, list_img, list_rank, list_flags, npig = records
    K, A, _ = npig.shape
    R, M = len(rec_thrs), len(max_dets)
    mult = np.asarray(mult, dtype=np.int64)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        sl = slice(int(list_off[k]), int(list_off[k + 1]))
        for a in range(A):
            NP = int((mult * npig[k, a]).sum())
            if NP == 0:
                continue
            for m, md in enumerate(max_dets):
                if only is not None and (a, m) not in only:
                    continue
                w = np.where(list_rank[sl] < md, mult[list_img[sl]], 0)
                for t in range(T):
                    matched = (list_flags[a, sl] >> t) & 1 != 0
                    ignored = (list_flags[a, sl] >> (16 + t)) & 1 != 0
                    tp = np.cumsum(w * (matched & ~ignored)).astype(np.float64)
                    fp = np.cumsum(w * (~matched & ~ignored)).astype(np.float64)
                    nd = len(tp)
                    rc = tp / NP
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    idx = np.searchsorted(rc, rec_thrs, side="left")
                    q = np.zeros(R)
                    q[idx < nd] = pr[idx[idx < nd]]
                    precision[t, :, k, a, m] = q
    return precision, recall


def _xywh(rng, n, side_lo, side_hi):
    w, h = rng.uniform(side_lo, side_hi, n), rng.uniform(side_lo, side_hi, n)
    return np.stack([rng.uniform(0, 600 - w), rng.uniform(0, 480 - h), w, h], 1)


@functools.lru_cache(maxsize=None)
def case():
    """(gt_json, results, mult [5, 7]).  7 images (ids 1..7), 2 categories (ids 1, 2):
      * image 4 has ground truth and no detection; image 7 has detections and no ground truth; image 2 holds a crowd box of category 1;
      * category 1 has ground truth in every area range; category 2 has none that is large (NP = 0: -1) ;
      * category 1's list has 129 entries (two 64-lane chunk seams), category 2's 65 (one);
      * image 1 has 40 detections of category 1: maxDet = 10 (and 1) cut;
      * equal scores across images 1 and 2 (category 1) and inside image 7 (category 1).  The pair inside image 7 agrees in its
        flags at every threshold (two unmatched boxes of the medium range): a duplicated image repeats its tie group as a whole
        (x y x y), the weighted list weighs entry by entry (xx yy) - the same table only when x and y count alike (section 27).
    The vectors: all ones; a zero and a three; zero on every image with ground truth of category 1; a single image; one resample."""
    from proben_amd.bootstrap import resample_multiplicities
    rng = np.random.default_rng(27)
    sides = {"small": (8, 30), "medium": (36, 90), "large": (100, 200)}
    gt_plan = {1: {1: ["small", "medium", "large"], 2: ["medium", "crowd", "small"], 3: ["large", "medium"], 4: ["small", "large"]},
               2: {3: ["small", "medium"], 5: ["medium", "medium"], 6: ["small"]}}
    anns = []
    for cat, per in gt_plan.items():
        for iid, kinds in per.items():
            for kind in kinds:
                b = _xywh(rng, 1, *sides["medium" if kind == "crowd" else kind])[0].round(2).tolist()
                anns.append({"id": len(anns) + 1, "image_id": iid, "category_id": cat, "bbox": b, "area": b[2] * b[3], "iscrowd": int(kind == "crowd")})
    gt_json = {"images": [{"id": i, "height": 512, "width": 640, "file_name": f"{i}.jpeg"} for i in range(1, 8)], "annotations": anns,
               "categories": [{"id": 1, "name": "person"}, {"id": 2, "name": "car"}]}
    det_plan = {1: {1: 40, 2: 30, 3: 25, 5: 14, 6: 10, 7: 10}, 2: {1: 5, 3: 20, 5: 15, 6: 15, 7: 10}}
    results = []
    for cat, per in det_plan.items():
        total = sum(per.values())
        scores = iter(((rng.permutation(total) + 1) / (total + 1.0)).tolist())          # distinct; the ties are set below
        for iid, n in per.items():
            gts = [a for a in anns if a["image_id"] == iid and a["category_id"] == cat]
            for j in range(n):
                if gts and j % 3 != 2:      # a jittered copy of a ground-truth box: a match at some thresholds, a duplicate at others
                    g = np.array(gts[j % len(gts)]["bbox"])
                    b = g + rng.normal(0, 0.06, 4) * np.array([g[2], g[3], g[2], g[3]])
                else:
                    b = _xywh(rng, 1, 8, 200)[0]
                results.append({"image_id": iid, "category_id": cat, "bbox": b.round(2).tolist(), "score": next(scores)})
    pick = lambda iid, cat: [r for r in results if r["image_id"] == iid and r["category_id"] == cat]      # noqa: E731
    pick(2, 1)[3]["score"] = pick(1, 1)[7]["score"]                   # equal across two images
    x, y = pick(7, 1)[2], pick(7, 1)[5]                               # equal inside one image: two medium boxes nothing overlaps
    y["score"] = x["score"]
    x["bbox"], y["bbox"] = [10.0, 10.0, 50.0, 50.0], [300.0, 300.0, 60.0, 40.0]
    assert sum(per_n for per_n in det_plan[1].values()) == 129 and sum(det_plan[2].values()) == 65
    mult = np.array([[1] * 7, [1, 0, 3, 1, 1, 1, 1], [0, 0, 0, 0, 2, 1, 2], [0, 0, 3, 0, 0, 0, 0],
                     resample_multiplicities(7, 2, 27)[1].tolist()], dtype=np.int64)
    return gt_json, results, mult


def COCOevalBBox_on(gt_json, results):
    """The NumPy evaluator run to the end on a dataset."""
    from proben_amd.evaluation import COCOevalBBox
    ev = COCOevalBBox(gt_json, results, impl="numpy")
    ev.evaluate()
    ev.accumulate()
    ev.summarize(printer=None)
    return ev


@functools.lru_cache(maxsize=None)
def duplicated_eval(v):
    """The exact expectation of vector v of the case: COCOevalBBox(impl="numpy") on the duplicated dataset, summarized.  Shared, read-only."""
    gt_json, results, mult = case()
    ev = COCOevalBBox_on(*duplicated_dataset(gt_json, results, mult[v]))
    for arr in (ev.eval["precision"], ev.eval["recall"], ev.stats):
        arr.setflags(write=False)
    return ev


@functools.lru_cache(maxsize=None)
def paired_case():
    """(gt_json, results_a, results_b) on 64 synthetic images (proben_amd.synthetic.synth_detections rows, no detector run): file A is
    a detector's rows, the ground truth is every second of them (so half of A's rows are true positives at every threshold, at
    scores no different from the others'), file B is A with the score of every category-1 row that is a ground-truth box times 0.2:
    category 1's true positives sink below its false positives."""
    from proben_amd.synthetic import synth_detections
    xywh = lambda b: [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])]      # noqa: E731
    anns, a, b = [], [], []
    for i, (d1,) in enumerate(synth_detections(64, 5, kdet=1, nmax=24, K=3), 1):
        for j, (box, s, c) in enumerate(zip(d1["bbox"], d1["score"], d1["class"])):
            row = {"image_id": i, "category_id": int(c) + 1, "bbox": xywh(box), "score": float(s)}
            a.append(row)
            if j % 2 == 0:
                anns.append({"id": len(anns) + 1, "image_id": i, "category_id": row["category_id"], "bbox": row["bbox"],
                             "area": row["bbox"][2] * row["bbox"][3], "iscrowd": 0})
            b.append(dict(row, score=row["score"] * 0.2) if j % 2 == 0 and c == 0 else dict(row))
    gt_json = {"images": [{"id": i, "height": 512, "width": 640, "file_name": f"{i}.jpeg"} for i in range(1, 65)], "annotations": anns,
               "categories": [{"id": c, "name": n} for c, n in ((1, "person"), (2, "bicycle"), (3, "car"))]}
    return gt_json, a, b


def cells_of(table, K):
    """[T, R, K, A, M] or [T, K, A, M] -> [K * 6, T(, R)]: the evaluated cells in the kernel's order."""
    return np.stack([table[..., k, a, m] for k in range(K) for a, m in SUMMARY_CELLS])
