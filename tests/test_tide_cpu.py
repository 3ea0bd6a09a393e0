"""TIDE without a GPU: the NumPy restatement tests/tide_ref.py on cases worked by hand, against the evaluator's
exported flags, against COCOevalBBox(impl="numpy") on the edited datasets, on a planted set; the host layers of proben_amd.tide fed
with the restatement's typing; the argument checks of pe_tide_classify and the CLI's parser."""
import ctypes

import numpy as np
import pytest

import ap_bootstrap_ref as R
import tide_ref as T

A, C10, C20, C100, C101, HAND = T.A, T.C10, T.C20, T.C100, T.C101, T.HAND


def one(dets, gts, **kw):
    """classify_image over [(box, cat)] in the total order and [(box, cat, crowd)]."""
    return T.classify_image([d[0] for d in dets], [d[1] for d in dets], [g[0] for g in gts], [g[1] for g in gts], [g[2] for g in gts], **kw)


def test_the_seam_boxes_are_exact():
    assert T.plain_iou(C10, C20) == 0.5 and T.plain_iou(C10, C100) == 0.1 and T.plain_iou(C10, C101) < 0.1
    assert T.eval_iou(C10, C20, False) == 0.5 and T.eval_iou(C10, C100, True) == 1.0


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_cases_worked_by_hand(case):
    _, dets, gts, types, partners, claims, bits = case
    out = one(dets, gts)
    assert out["type"].tolist() == types and out["partner"].tolist() == partners and out["claim"].tolist() == claims
    assert out["gt"].tolist() == bits
    assert [m >= 0 for m in out["match"]] == [t in (T.TP, T.IGNORED) for t in types]


def test_the_later_ground_truth_holds_the_first_match():
    assert one([(C10, 0)], [(C20, 0, 0), (C20, 0, 0)])["match"].tolist() == [1]


def test_order_nan_last_and_ties_by_category_then_rank():
    gt_json = {"images": [{"id": 1}], "annotations": [], "categories": [{"id": 1}, {"id": 2}]}
    res = [{"image_id": 1, "category_id": c, "bbox": A, "score": s} for c, s in ((2, .5), (1, float("nan")), (1, .5), (2, .9), (1, .5), (2, float("nan")))]
    ds = T.dataset(gt_json, res)
    assert [e["row"] for e in ds["dets"]] == [3, 2, 4, 0, 1, 5]
    assert [e["rank"] for e in ds["dets"]] == [0, 0, 1, 1, 2, 2]


SETS = {"case": lambda: R.case()[:2], "seeded": lambda: T.random_case(2), "seeded-2": lambda: T.random_case(24, K=2, images=5)}
_cache = {}


def typed(name):
    """(gt_json, results, classified dataset, (records, recs, moved)) of a named set: computed once, shared, read-only."""
    if name not in _cache:
        gt_json, results = SETS[name]()
        ds = T.classify(T.dataset(gt_json, results))
        _cache[name] = (gt_json, results, ds, T.variant_records(ds))
    return _cache[name]


def product_side(name):
    """proben_amd.tide's host layers over the same set, its kernel replaced by the restatement's typing."""
    from proben_amd import tide
    from proben_amd.bootstrap import export_matches
    gt_json, results, ds, _ = typed(name)
    m = export_matches(gt_json, results)
    lay = tide.layout(m)
    raw = {k: [] for k in ("match", "type", "partner", "claim", "gt")}
    for i in range(ds["I"]):
        d, g = slice(*lay["det_off"][i:i + 2]), slice(*lay["gt_off"][i:i + 2])
        out = T.classify_image(lay["det_box"][d], lay["det_cat"][d], lay["gt_box"][g], lay["gt_cat"][g], lay["gt_crowd"][g])
        for k in raw:
            raw[k].append(out[k])
    raw = {k: np.concatenate(v).astype(np.int32) for k, v in raw.items()}
    return m, lay, tide.assemble(m, lay, raw)


@pytest.mark.parametrize("name", ["case", "seeded"])
def test_base_flags_are_the_evaluators(name):
    """The restatement's lists and variant-0 flags are export_matches' at area range 0, threshold 0 (T = 1: bit 0 and bit 16)."""
    from proben_amd.bootstrap import export_matches
    gt_json, results, ds, (records, recs, moved) = typed(name)
    m = export_matches(gt_json, results)
    keep = ~np.array(moved, bool)
    assert (np.diff(records[0]) - np.diff(m["list_off"]) == np.bincount([ds["gts"][e["partner"]]["cat"] for e, mv in zip(recs, moved) if mv],
                                                                         minlength=ds["K"])).all()
    assert records[1][keep].tobytes() == m["list_img"].tobytes() and records[2][keep].tobytes() == m["list_rank"].tobytes()
    want = (m["list_flags"][0] & 1) | (m["list_flags"][0] & (1 << 16))
    assert records[3][0][keep].tobytes() == want.astype(np.uint32).tobytes()
    assert (records[4][:, 0, :] == m["npig"][:, 0, :]).all()
    assert 0 < (want & 1).sum() < len(want)
    if name == "seeded":
        assert any(g["crowd"] for g in ds["gts"]) and any(m_ for m_ in moved) and (want >> 16).any()


@pytest.mark.parametrize("name", ["case", "seeded", "seeded-2"])
@pytest.mark.parametrize("v", [3, 4, 5, 6, 7, 8])
def test_removal_variants_are_the_evaluator_on_the_edited_dataset(name, v):
    """An unmatched detection holds no ground truth and an unmatched ground truth was never chosen, so deleting either changes no other
    match: the variant's precision column is COCOevalBBox(impl="numpy") at IoU 0.5 / all / 100 on the edited dataset, bit for bit."""
    gt_json, results, ds, (records, _, _) = typed(name)
    ev = R.COCOevalBBox_on(*T.edited_dataset(gt_json, results, ds, v))
    _, _, p = T.psum_table(records, np.ones(ds["I"], int), ev.rec_thrs)
    want = ev.eval["precision"][0, :, :, 0, 2]
    assert p[:, :, v].tobytes() == want.tobytes()
    assert (want > -1).any()


@pytest.mark.parametrize("name", ["case", "seeded", "seeded-2"])
def test_variant_zero_is_the_evaluator(name):
    gt_json, results, ds, (records, _, _) = typed(name)
    ev = R.COCOevalBBox_on(gt_json, results)
    psum, valid, p = T.psum_table(records, np.ones(ds["I"], int), ev.rec_thrs)
    assert p[:, :, 0].tobytes() == ev.eval["precision"][0, :, :, 0, 2].tobytes()
    N = int(valid[:, 0].sum()) * len(ev.rec_thrs)
    assert abs(T.ap50(psum, valid, len(ev.rec_thrs))[0] - ev.stats[1]) <= 2 * N * 2.0 ** -53


@pytest.mark.parametrize("seed", range(6))
def test_every_repair_gains_and_the_totals_bound_their_parts(seed):
    gt_json, results = T.random_case(100 + seed, K=2 + seed % 3, images=4 + seed % 3, ties=seed % 2 == 0)
    ds = T.classify(T.dataset(gt_json, results))
    records, _, _ = T.variant_records(ds)
    rec_thrs = np.linspace(0, 1, 101)
    psum, valid, _ = T.psum_table(records, np.ones(ds["I"], int), rec_thrs)
    ap = T.ap50(psum, valid, 101)
    d = dict(zip(T.VARIANTS, ap - ap[0]))
    print(seed, d)
    assert ap[0] > -1 and all(d[v] >= 0 for v in T.VARIANTS)
    assert all(d["FP"] >= d[v] for v in ("Both", "Dupe", "Bkg")) and d["FN"] >= d["Miss"]


def planted():
    """Objects 100 apart on a grid, 3 classes; per object one fate.  Returns (gt_json, results, planted counts, planted confusion)."""
    fates = ["swap"] * 4 + ["shift"] * 5 + ["dupe"] * 3 + ["drop"] * 2 + ["both"] * 2 + ["hit"] * 9
    rng = np.random.default_rng(32)
    rng.shuffle(fates)
    anns, res, conf = [], [], np.zeros((3, 3), int)
    for n, fate in enumerate(fates):
        img, cat = 1 + n % 4, 1 + n % 3
        x, y = 100.0 * (n % 6), 100.0 * (n // 6)
        anns.append({"id": n + 1, "image_id": img, "category_id": cat, "bbox": [x, y, 20.0, 20.0], "area": 400.0, "iscrowd": 0})
        other = 1 + (cat + n // 3 % 2) % 3          # one of the two other classes
        det = lambda b, c: res.append({"image_id": img, "category_id": c, "bbox": b, "score": float(rng.uniform(0.1, 0.9))})      # noqa: E731
        if fate in ("hit", "dupe"):
            det([x, y, 20.0, 20.0], cat)
        if fate == "dupe":
            det([x, y, 20.0, 20.0], cat)
        if fate == "swap":
            det([x, y, 20.0, 20.0], other)
            conf[other - 1, cat - 1] += 1
        if fate == "shift":
            det([x + 10.0, y, 20.0, 20.0], cat)          # IoU 1/3
        if fate == "both":
            det([x + 10.0, y, 20.0, 20.0], other)
    for n in range(6):                                     # strays
        res.append({"image_id": 1 + n % 4, "category_id": 1 + n % 3, "bbox": [50.0 + 100.0 * n, 850.0, 20.0, 20.0], "score": 0.5})
    gt_json = {"images": [{"id": i, "height": 1000, "width": 1000, "file_name": f"{i}.jpeg"} for i in range(1, 5)], "annotations": anns,
               "categories": [{"id": c, "name": f"c{c}"} for c in (1, 2, 3)]}
    want = {T.TP: 12, T.CLS: 4, T.LOC: 5, T.BOTH: 2, T.DUPE: 3, T.BKG: 6, T.IGNORED: 0, "missed": 4, "unmatched": 4 + 4 + 5}
    return gt_json, res, want, conf


def test_planted_errors_are_counted_exactly():
    gt_json, res, want, conf = planted()
    types, missed, unmatched, got_conf = T.counts(T.classify(T.dataset(gt_json, res)))
    assert {t: int(types[t].sum()) for t in range(7)} == {t: want[t] for t in range(7)}
    assert missed.sum() == want["missed"] and unmatched.sum() == want["unmatched"]
    assert (got_conf == conf).all() and conf.sum() == 4 and (np.diag(conf) == 0).all()


@pytest.mark.parametrize("name", ["case", "seeded"])
def test_host_layers_over_the_restatements_typing(name):
    """layout() orders the entries as the restatement does; assemble() and variant_lists() over the restatement's typing give the
    restatement's counts and its lists, byte for byte."""
    from proben_amd import tide
    _, _, ds, (records, _, moved) = typed(name)
    m, lay, cl = product_side(name)
    assert lay["det_box"].tolist() == [e["box"] for e in ds["dets"]] and lay["det_cat"].tolist() == [e["cat"] for e in ds["dets"]]
    assert lay["gt_box"].tolist() == [g["box"] for g in ds["gts"]]
    types, missed, unmatched, conf = T.counts(ds)
    c = cl["counts"]
    assert (c["types"] == types).all() and (c["missed"] == missed).all() and (c["unmatched"] == unmatched).all() and (c["confusion"] == conf).all()
    lists = tide.variant_lists(cl)
    for key, want in zip(("list_off", "list_img", "list_rank", "list_flags", "npig"), records):
        assert lists[key].dtype == want.dtype and lists[key].tobytes() == want.tobytes(), key
    assert lists["moved"].tolist() == list(moved) and lists["sizes"] == (ds["I"], ds["K"], 9, 1)


def test_argument_checks_answer_without_a_gpu():
    import proben_amd
    L = proben_amd._lib.lib()
    err = lambda: L.pe_last_error().decode()      # noqa: E731
    off = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    P = 4096                                       # stands for a device pointer: no check may read it
    call = lambda do, go, B=1, K=3, M=2, G=2, tf=0.5, tb=0.1, ws=P, box=P: L.pe_tide_classify(box, P, do, P, P, P, go, B, K, M, G, tf, tb, ws, P, P, P, P, P, None)      # noqa: E731
    assert L.pe_tide_classify(None, None, None, None, None, None, None, 0, 3, 0, 0, 0.5, 0.1, None, None, None, None, None, None, None) == 0
    assert call(None, off(0, 2)) == -1 and "null pointer" in err()
    assert call(off(0, 2), off(0, 2), ws=None) == -1 and "null pointer" in err()
    assert call(off(0, 2), off(0, 2), box=None) == -1 and "null pointer" in err()
    for tf, tb in ((0.5, 0.5), (0.5, -0.1), (1.5, 0.1), (0.5, float("nan")), (float("nan"), 0.1)):
        assert call(off(0, 2), off(0, 2), tf=tf, tb=tb) == -1 and "0 <= t_b < t_f <= 1" in err()
    assert call(off(0, 3, 2), off(0, 1, 2), B=2) == -1 and "not monotone" in err()
    assert call(off(1, 2), off(0, 2)) == -1 and "start at 0" in err()
    assert call(off(0, 2), off(0, 2), K=0) == -1 and "bad sizes" in err()
    assert call(off(0, 2), off(0, 2), K=81) == -2 and "80" in err()
    assert call(off(0, 2), off(0, 1025), G=1025) == -2 and "1024" in err()
    assert call(off(0, 8001), off(0, 2), M=8001) == -2 and "8000" in err()


def test_python_checks_answer_without_a_gpu():
    from proben_amd import tide
    gt_json, results = T.random_case(2)
    with pytest.raises(ValueError, match="background_iou"):
        tide.classify(gt_json, results, background_iou=0.5)
    with pytest.raises(ValueError, match="confidence"):
        tide.tide(gt_json, results, confidence=1.0)
    with pytest.raises(ValueError, match="replicates"):
        tide.tide(gt_json, results, replicates=1)
    with pytest.raises(ValueError, match="does not have"):
        tide.tide(gt_json, results + [dict(results[0], image_id=99)])
    with pytest.raises(ValueError, match="images \\+ 1"):
        tide.classify_arrays(np.zeros((0, 4)), [], [0], [], [], [], [0, 0], 3)
    huge = [dict(a, area=1e11) for a in gt_json["annotations"]]
    with pytest.raises(ValueError, match="outside the evaluator's range"):
        tide.classify(dict(gt_json, annotations=huge), results)


def test_cli_parser_and_table():
    from proben_amd.cli import tide as cli
    a = cli.parse(["--dataset_path", "d", "--predictions", "a.json", "b.json", "--background_iou", "0.2", "--replicates", "50", "--seed", "3"])
    assert (a.background_iou, a.replicates, a.seed, a.confidence, a.out, a.device) == (0.2, 50, 3, 0.95, None, "cuda")
    assert cli.parse(["--dataset_path", "d", "--predictions", "a.json"]).background_iou == 0.1
    for bad in (["--background_iou", "0.5"], ["--replicates", "1"], ["--confidence", "1"], ["--predictions", "a", "b", "c"]):
        with pytest.raises(SystemExit):
            cli.parse(["--dataset_path", "d", "--predictions", "a.json"] + bad)
    rec = {"point": 0.01, "lo": 0.0, "hi": 0.02, "se": 0.005, "replicates": 49}
    side = {"AP50": dict(rec, point=0.6), "repairs": {r: dict(rec, count=3) for r in T.VARIANTS[1:]}}
    text = cli.table({"confidence": 0.95, "a": side, "b": side, "paired": {r: dict(rec, p=0.04) for r in T.VARIANTS[1:]}}, ["a.json", "b.json"])
    assert all("d" + r in text for r in T.VARIANTS[1:]) and "AP50" in text and "p 0.0400" in text and text.count("dMiss") == 3
