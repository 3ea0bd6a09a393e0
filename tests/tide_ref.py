"""Helpers of tests/test_tide_{cpu,gpu}.py: the TIDE rule restated in plain NumPy float64 loops, steps A to E, from
the dataset dicts up.  It imports nothing of the product: the typing, the claims, the variants and their lists are all built here a
second time.  Not a test module.

The rule (restated from Bolya et al., ECCV 2020, for this project's evaluator; the priority Loc, Cls, Dupe, Bkg, Both is the project's):
  order   per image the kept detections (per category the top 100 by stable descending score) by descending score, NaN last, ties by
          category index, then rank; ground truths in annotation order
  A       cocoeval.py:236-313 at t_f with every non-crowd ground truth counted, category by category
  B       own / other = largest plain IoU over the non-crowd ground truths of the own / the other classes, lowest index on a tie
          Loc t_b <= own < t_f | Cls other >= t_f | Dupe own >= t_f | Bkg other < t_b | Both
  C       missed = non-crowd, unmatched in A, partner of no Loc and no Cls error
  D       two walks in order (Loc, Cls): an error claims its partner if A left it unmatched and nobody of the walk holds it
  E       the nine variants as flags and ground-truth counts over the evaluator's lists (variant 1 adds the claimed Cls errors to
          their partner's list)
"""
import numpy as np

TP, CLS, LOC, BOTH, DUPE, BKG, IGNORED = range(7)
VARIANTS = ("base", "Cls", "Loc", "Both", "Dupe", "Bkg", "Miss", "FP", "FN")
GT_MATCHED, GT_LOC, GT_CLS, GT_MISSED = 1, 2, 4, 8
CAP = 100


def _overlap(d, g):
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    return np.float64(0.0) if (w <= 0 or h <= 0) else w * h


def _eval_iou(d, g, crowd):
    inter = _overlap(d, g)
    return inter / (d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - inter)


def _plain_iou(d, g):
    inter = _overlap(d, g)
    return inter / (d[2] * d[3] + g[2] * g[3] - inter) if inter > 0 else np.float64(0.0)


def eval_iou(d, g, crowd):
    """bbIou as the evaluator uses it: unguarded."""
    with np.errstate(all="ignore"):
        return _eval_iou(np.asarray(d, dtype=np.float64), np.asarray(g, dtype=np.float64), crowd)


def plain_iou(d, g):
    with np.errstate(all="ignore"):
        return _plain_iou(np.asarray(d, dtype=np.float64), np.asarray(g, dtype=np.float64))


def classify_image(det_box, det_cat, gt_box, gt_cat, gt_crowd, t_f=0.5, t_b=0.1):
    """Steps A to D for one image whose detections are already in the total order.  int arrays "match", "type", "partner", "claim" [D]
    and "gt" [G] (bits), all indices local to the image."""
    with np.errstate(all="ignore"):
        return _classify_image(np.asarray(det_box, dtype=np.float64).reshape(-1, 4), det_cat, np.asarray(gt_box, dtype=np.float64).reshape(-1, 4),
                               gt_cat, gt_crowd, t_f, t_b)


def _classify_image(det_box, det_cat, gt_box, gt_cat, gt_crowd, t_f, t_b):
    D, G = len(det_cat), len(gt_cat)
    match, typ, partner, claim = -np.ones(D, int), np.full(D, BKG), -np.ones(D, int), np.zeros(D, int)
    taken = np.zeros(G, bool)
    thr = min(t_f, 1 - 1e-10)
    for k in sorted(set(int(c) for c in det_cat)):                                   # A
        gts = sorted((g for g in range(G) if gt_cat[g] == k), key=lambda g: bool(gt_crowd[g]))      # stable: the regular ones first
        for d in range(D):
            if det_cat[d] != k:
                continue
            best, m = thr, -1
            for pos, g in enumerate(gts):
                if taken[g] and not gt_crowd[g]:
                    continue
                if m > -1 and not gt_crowd[gts[m]] and gt_crowd[g]:
                    break
                v = _eval_iou(det_box[d], gt_box[g], gt_crowd[g])
                if v < best:
                    continue
                best, m = v, pos
            if m > -1:
                match[d], taken[gts[m]] = gts[m], True
                typ[d] = IGNORED if gt_crowd[gts[m]] else TP
    for d in range(D):                                                                # B
        if match[d] >= 0:
            continue
        own, own_g, other, other_g = 0.0, -1, 0.0, -1
        for g in range(G):
            if gt_crowd[g]:
                continue
            v = _plain_iou(det_box[d], gt_box[g])
            if not v >= 0:
                continue
            if gt_cat[g] == det_cat[d]:
                if own_g < 0 or v > own:
                    own, own_g = v, g
            elif other_g < 0 or v > other:
                other, other_g = v, g
        if t_b <= own < t_f:
            typ[d], partner[d] = LOC, own_g
        elif other >= t_f:
            typ[d], partner[d] = CLS, other_g
        elif own >= t_f:
            typ[d], partner[d] = DUPE, own_g
        elif other < t_b:
            typ[d] = BKG
        else:
            typ[d] = BOTH
    gt = np.zeros(G, int)                                                             # C
    for g in range(G):
        loc = any(typ[d] == LOC and partner[d] == g for d in range(D))
        cls = any(typ[d] == CLS and partner[d] == g for d in range(D))
        gt[g] = GT_MATCHED * bool(taken[g]) + GT_LOC * loc + GT_CLS * cls + GT_MISSED * (not gt_crowd[g] and not taken[g] and not loc and not cls)
    for kind in (LOC, CLS):                                                           # D
        held = set()
        for d in range(D):
            if typ[d] == kind and partner[d] >= 0 and not taken[partner[d]] and partner[d] not in held:
                held.add(int(partner[d]))
                claim[d] = 1
    return {"match": match, "type": typ, "partner": partner, "claim": claim, "gt": gt}


def _score_key(s):
    return (1, 0.0) if s != s else (0, -s)


def dataset(gt_json, results):
    """The kept detections and the ground truths of a dataset as flat records, per image in the rule's orders.  "dets": dicts with img,
    cat (dense indices), rank, score, box, row (into results), image-major in the total order; "gts": dicts with img, cat, box, crowd,
    ann (into the annotations), image-major in annotation order."""
    img_ids = sorted({im["id"] for im in gt_json["images"]})
    cat_ids = sorted({c["id"] for c in gt_json["categories"]})
    img_ix, cat_ix = {v: i for i, v in enumerate(img_ids)}, {v: i for i, v in enumerate(cat_ids)}
    cells = {}
    for row, r in enumerate(results):
        if r["category_id"] in cat_ix:
            cells.setdefault((img_ix[r["image_id"]], cat_ix[r["category_id"]]), []).append(row)
    dets = []
    for (i, k), rows in cells.items():
        rows = sorted(rows, key=lambda r: _score_key(results[r]["score"]))[:CAP]      # sorted() is stable: file order inside a tie
        dets += [{"img": i, "cat": k, "rank": n, "score": float(results[r]["score"]), "box": [float(x) for x in results[r]["bbox"]], "row": r}
                 for n, r in enumerate(rows)]
    dets.sort(key=lambda e: (e["img"],) + _score_key(e["score"]) + (e["cat"], e["rank"]))
    gts = [{"img": img_ix[a["image_id"]], "cat": cat_ix[a["category_id"]], "box": [float(x) for x in a["bbox"]],
            "crowd": int(a.get("iscrowd", 0)) != 0, "ann": n}
           for n, a in enumerate(gt_json.get("annotations", [])) if a["category_id"] in cat_ix and a["image_id"] in img_ix]
    gts.sort(key=lambda g: g["img"])
    return {"dets": dets, "gts": gts, "I": len(img_ids), "K": len(cat_ids)}


def classify(ds, t_f=0.5, t_b=0.1):
    """Steps A to D over a dataset(): every detection record gains type / match / partner (indices into ds["gts"], -1) / claim, every
    ground-truth record gains bits."""
    for i in range(ds["I"]):
        di = [n for n, e in enumerate(ds["dets"]) if e["img"] == i]
        gi = [n for n, g in enumerate(ds["gts"]) if g["img"] == i]
        out = classify_image([ds["dets"][n]["box"] for n in di], [ds["dets"][n]["cat"] for n in di], [ds["gts"][n]["box"] for n in gi],
                             [ds["gts"][n]["cat"] for n in gi], [ds["gts"][n]["crowd"] for n in gi], t_f, t_b)
        for j, n in enumerate(di):
            ds["dets"][n].update(type=int(out["type"][j]), claim=int(out["claim"][j]),
                                 match=gi[out["match"][j]] if out["match"][j] >= 0 else -1,
                                 partner=gi[out["partner"][j]] if out["partner"][j] >= 0 else -1)
        for j, n in enumerate(gi):
            ds["gts"][n]["bits"] = int(out["gt"][j])
    return ds


def counts(ds):
    """(per type and class [7, K], missed [K], unmatched non-crowd [K], confusion of the Cls errors [K, K])."""
    K = ds["K"]
    types, missed, unmatched, conf = np.zeros((7, K), int), np.zeros(K, int), np.zeros(K, int), np.zeros((K, K), int)
    for e in ds["dets"]:
        types[e["type"], e["cat"]] += 1
        if e["type"] == CLS:
            conf[e["cat"], ds["gts"][e["partner"]]["cat"]] += 1
    for g in ds["gts"]:
        missed[g["cat"]] += bool(g["bits"] & GT_MISSED)
        unmatched[g["cat"]] += (not g["crowd"]) and not g["bits"] & GT_MATCHED
    return types, missed, unmatched, conf


def variant_records(ds):
    """Step E: (list_off, list_img, list_rank, list_flags [9, n], npig [K, 9, I]) in the form ap_bootstrap_ref.weighted_accumulate takes,
    T = 1 (bit 0 matched, bit 16 ignored), the variant on the area-range axis; plus, per list row, the detection record behind it and
    whether it is a moved copy."""
    K, I, V = ds["K"], ds["I"], len(VARIANTS)
    off, img, rank, flags, recs, moved = [0], [], [], [], [], []
    for k in range(K):
        own = sorted((e for e in ds["dets"] if e["cat"] == k), key=lambda e: (e["img"], e["rank"]))
        own.sort(key=lambda e: _score_key(e["score"]))                                 # stable, as accumulate's mergesort
        extra = [e for e in ds["dets"] if e["type"] == CLS and e["claim"] and ds["gts"][e["partner"]]["cat"] == k]      # image order, then total order
        rows = sorted([(e, False) for e in own] + [(e, True) for e in extra], key=lambda p: _score_key(p[0]["score"]))
        for e, mv in rows:
            f = []
            for v in range(V):
                matched, ignored = e["type"] in (TP, IGNORED), e["type"] == IGNORED
                if mv:
                    matched, ignored = v == 1, v != 1
                elif v == 1:
                    ignored |= e["type"] == CLS
                elif v == 2 and e["type"] == LOC:
                    matched, ignored = bool(e["claim"]), not e["claim"]
                elif v in (3, 4, 5):
                    ignored |= e["type"] == v
                elif v == 7:
                    ignored |= CLS <= e["type"] <= BKG
                f.append(int(matched) | int(ignored) << 16)
            flags.append(f)
            img.append(e["img"])
            rank.append(0 if mv else e["rank"])
            recs.append(e)
            moved.append(mv)
        off.append(len(img))
    npig = np.zeros((K, V, I), np.int32)
    for g in ds["gts"]:
        if g["crowd"]:
            continue
        for v in range(V):
            gone = (v == 6 and g["bits"] & GT_MISSED) or (v == 8 and not g["bits"] & GT_MATCHED)
            npig[g["cat"], v, g["img"]] += not gone
    records = (np.array(off, np.int64), np.array(img, np.int32), np.array(rank, np.uint8),
               np.array(flags, np.uint32).reshape(len(img), V).T.copy(), npig)
    return records, recs, moved


def psum_table(records, mult, rec_thrs):
    """(psum [K, 9], valid [K, 9], precision [R, K, 9]) of one replicate under the weighted accumulate rule of section 27: psum is the
    cell's R precisions added in order."""
    from ap_bootstrap_ref import weighted_accumulate
    p, _ = weighted_accumulate(records, mult, rec_thrs, 1, [CAP])
    p = p[0, :, :, :, 0]
    valid = p[0] > -1
    s = np.zeros(p.shape[1:])
    for r in range(p.shape[0]):
        s = s + p[r]
    return np.where(valid, s, 0.0), valid, p


def ap50(psum, valid, R):
    """[9]: the mean over the valid categories of psum / R, added in category order; -1 without one."""
    tot, n = np.zeros(psum.shape[1]), np.zeros(psum.shape[1], int)
    for k in range(psum.shape[0]):
        tot = tot + np.where(valid[k], psum[k] / R, 0.0)
        n += valid[k]
    return np.where(n > 0, tot / np.maximum(n, 1), -1.0)


def edited_dataset(gt_json, results, ds, v):
    """The dataset variant v in (3, 4, 5, 6, 7, 8) stands for: exactly those detections deleted from the results, or exactly those
    annotations deleted from the ground truth."""
    drop_rows = {e["row"] for e in ds["dets"] if (v in (3, 4, 5) and e["type"] == v) or (v == 7 and CLS <= e["type"] <= BKG)}
    drop_anns = {g["ann"] for g in ds["gts"] if not g["crowd"] and ((v == 6 and g["bits"] & GT_MISSED) or (v == 8 and not g["bits"] & GT_MATCHED))}
    gt2 = dict(gt_json, annotations=[a for n, a in enumerate(gt_json["annotations"]) if n not in drop_anns])
    return gt2, [r for n, r in enumerate(results) if n not in drop_rows]


A, B_, C10, C20, C100, C101 = [0, 0, 10, 10], [50, 50, 10, 10], [0, 0, 10, 10], [0, 0, 10, 20], [0, 0, 10, 100], [0, 0, 10, 101]
# (name, detections, ground truths, types, partners, claims, ground-truth bits)
HAND = [
    ("IoU exactly 0.5 with a taken ground truth is Dupe", [(C20, 0), (C10, 0)], [(C20, 0, 0)], [TP, DUPE], [-1, 0], [0, 0], [GT_MATCHED]),
    ("IoU exactly 0.5 with a free one is TP", [(C10, 0)], [(C20, 0, 0)], [TP], [-1], [0], [GT_MATCHED]),
    ("exactly 0.1 with its own class is Loc, and its partner is not missed", [(C10, 0)], [(C100, 0, 0)], [LOC], [0], [1], [GT_LOC]),
    ("0.1 with another class only is Both, and the ground truth is missed", [(C10, 0)], [(C100, 1, 0)], [BOTH], [-1], [0], [GT_MISSED]),
    ("just under 0.1 is Bkg, whichever class", [(C10, 0), (C10, 1)], [(C101, 1, 0)], [BKG, BKG], [-1, -1], [0, 0], [GT_MISSED]),
    ("own in [0.1, 0.5) with other >= 0.5 is Loc", [(C10, 0)], [(C100, 0, 0), (C10, 1, 0)], [LOC], [0], [1], [GT_LOC, GT_MISSED]),
    ("own >= 0.5 taken with other >= 0.5 is Cls", [(C10, 0), (C10, 0)], [(C10, 0, 0), (C20, 1, 0)], [TP, CLS], [-1, 1], [0, 1],
     [GT_MATCHED, GT_CLS]),
    ("two Loc errors on one free ground truth: the first claims", [(C10, 0), (C10, 0)], [(C100, 0, 0)], [LOC, LOC], [0, 0], [1, 0], [GT_LOC]),
    ("a Loc error on a matched ground truth is removed", [(C20, 0), ([0, 0, 10, 5], 0)], [(C20, 0, 0)], [TP, LOC], [-1, 0], [0, 0],
     [GT_MATCHED | GT_LOC]),
    ("a crowd ground truth neither types nor misses", [(C10, 1), (B_, 0)], [(C100, 0, 1)], [BKG, BKG], [-1, -1], [0, 0], [0]),
    ("a detection on a crowd ground truth is ignored, again and again", [(C10, 0), (C10, 0)], [(C100, 0, 1)], [IGNORED, IGNORED], [-1, -1],
     [0, 0], [GT_MATCHED]),
    ("the later ground truth wins an IoU tie in A, the lowest index in B", [(C10, 0), (C10, 0), (C10, 0)], [(C20, 0, 0), (C20, 0, 0)],
     [TP, TP, DUPE], [-1, -1, 0], [0, 0, 0], [GT_MATCHED, GT_MATCHED]),
    ("Loc is tested before Cls: own 0.1 beats other 1.0, and the second claim fails", [(C10, 1), (C10, 0), (C10, 0)],
     [(C10, 1, 0), (C100, 0, 0)], [TP, LOC, LOC], [-1, 1, 1], [0, 1, 0], [GT_MATCHED, GT_LOC]),
    ("a Cls error whose partner is taken is removed", [(C10, 1), (C10, 0)], [(C10, 1, 0)], [TP, CLS], [-1, 0], [0, 0],
     [GT_MATCHED | GT_CLS]),
    ("two Cls errors on one free ground truth: the first claims", [(C10, 0), (C10, 0)], [(C20, 1, 0)], [CLS, CLS], [0, 0], [1, 0], [GT_CLS]),
    ("two Cls errors on a taken ground truth are both removed", [(C10, 0), (C10, 0), (C10, 1)], [(C20, 1, 0), (C100, 1, 0)],
     [CLS, CLS, TP], [0, 0, -1], [0, 0, 0], [GT_MATCHED | GT_CLS, GT_MISSED]),
    ("a NaN IoU lets every later candidate through, as the evaluator's comparison does", [([5, 5, 0, 0], 0)], [([5, 5, 0, 0], 0, 0), (C10, 0, 0)],
     [TP], [-1], [0], [GT_MISSED, GT_MATCHED]),
    ("no ground truth at all", [(C10, 0)], [], [BKG], [-1], [0], []),
]


def random_case(seed, K=3, images=6, crowd=True, ties=True):
    """A seeded set on an integer grid: K classes, crowd boxes, score ties inside and across categories, an empty image, IoU ties and
    the 0.5 / 0.1 seams (boxes with integer corners from a small range)."""
    rng = np.random.default_rng(seed)
    anns, results = [], []
    box = lambda: [float(rng.integers(0, 12)), float(rng.integers(0, 12)), float(rng.integers(1, 4) * 5), float(rng.integers(1, 4) * 5)]      # noqa: E731
    for i in range(1, images + 1):
        if i == 3:
            continue                                        # an image with neither ground truth nor detections
        for _ in range(int(rng.integers(0 if i != 2 else 3, 7))):
            b = box()
            anns.append({"id": len(anns) + 1, "image_id": i, "category_id": int(rng.integers(1, K + 1)), "bbox": b, "area": b[2] * b[3],
                         "iscrowd": int(crowd and rng.random() < 0.15)})
        mine = [a for a in anns if a["image_id"] == i]
        for _ in range(int(rng.integers(0 if i != 2 else 5, 25))):
            if mine and rng.random() < 0.6:
                a = mine[int(rng.integers(len(mine)))]
                b = list(a["bbox"])
                if rng.random() < 0.5:
                    b[int(rng.integers(2, 4))] *= float(rng.choice([0.5, 2.0, 1.0]))
                if rng.random() < 0.3:
                    b[0] += float(rng.integers(-3, 4))
                cat = a["category_id"] if rng.random() < 0.7 else int(rng.integers(1, K + 1))
            else:
                b, cat = box(), int(rng.integers(1, K + 1))
            score = float(rng.integers(1, 12)) / 12.0 if ties else float(rng.random())
            results.append({"image_id": i, "category_id": cat, "bbox": b, "score": score})
    gt_json = {"images": [{"id": i, "height": 64, "width": 64, "file_name": f"{i}.jpeg"} for i in range(1, images + 1)], "annotations": anns,
               "categories": [{"id": c, "name": f"c{c}"} for c in range(1, K + 1)]}
    return gt_json, results
