"""pe_tide_classify (csrc/tide.hip) on the GPU against the NumPy restatement tests/tide_ref.py, array for array;
the nine variants through pe_ap_bootstrap against the evaluator on the edited (and duplicated) datasets, bit for bit; the report of
tide() in its one-file and paired modes; the CLI on a FLIR-layout folder."""
import functools
import json

import numpy as np
import pytest

import ap_bootstrap_ref as R
import tide_ref as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KEYS = ("match", "type", "partner", "claim", "gt")


@functools.lru_cache(maxsize=None)
def image(D, G, K, seed):
    """One image on an integer grid: boxes with corners and sides from a small range (IoU ties and the exact 0.5 / 0.1 seams occur),
    a tenth of the ground truths crowd, the detections in an arbitrary (given) total order.  With its restated typing; read-only."""
    rng = np.random.default_rng(seed)
    span = 14 + G // 3                                  # the more ground truths, the wider the field: some detections stay alone
    box = lambda n: np.stack([rng.integers(0, span, n), rng.integers(0, span, n), rng.choice([5, 10, 20], n), rng.choice([5, 10, 20, 50], n)], 1).astype(np.float64)      # noqa: E731
    img = {"det_box": box(D), "det_cat": rng.integers(0, K, D).astype(np.int32), "gt_box": box(G), "gt_cat": rng.integers(0, K, G).astype(np.int32),
           "gt_crowd": (rng.random(G) < 0.1).astype(np.uint8)}
    n = min(D, G) // 2                                  # half of the detections sit on a ground truth, or on a scaled copy of one
    img["det_box"][:n] = img["gt_box"][:n]
    img["det_box"][: n // 2, 3] *= 0.5
    img["det_cat"][:n] = np.where(rng.random(n) < 0.7, img["gt_cat"][:n], img["det_cat"][:n])
    img["det_box"][n:n + n // 4] = img["det_box"][:n // 4]          # and an eighth repeats an earlier detection
    img["det_cat"][n:n + n // 4] = img["det_cat"][:n // 4]
    img["want"] = T.classify_image(img["det_box"], img["det_cat"], img["gt_box"], img["gt_cat"], img["gt_crowd"])
    for v in list(img.values()) + list(img["want"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return img


def launch(images, K, **kw):
    """The images as one launch; the outputs split per image."""
    from proben_amd.tide import classify_arrays
    cat = lambda key, dt, shape: np.concatenate([im[key].reshape(shape) for im in images] + [np.zeros((0,) + shape[1:], dt)]).astype(dt)      # noqa: E731
    d_off = np.cumsum([0] + [len(im["det_cat"]) for im in images])
    g_off = np.cumsum([0] + [len(im["gt_cat"]) for im in images])
    out = classify_arrays(cat("det_box", np.float64, (-1, 4)), cat("det_cat", np.int32, (-1,)), d_off, cat("gt_box", np.float64, (-1, 4)),
                          cat("gt_cat", np.int32, (-1,)), cat("gt_crowd", np.uint8, (-1,)), g_off, K, **kw)
    return [{k: out[k][(g_off if k == "gt" else d_off)[i]:(g_off if k == "gt" else d_off)[i + 1]] for k in KEYS} for i in range(len(images))]


# (detections, ground truths, classes): every lane-count seam of both axes, the 3 x 100 image, the ground-truth limit, K = 1, 3, 80
SHAPES = [(0, 0, 1), (1, 1, 1), (63, 63, 3), (64, 64, 3), (65, 65, 3), (300, 1024, 3), (0, 64, 3), (65, 0, 3), (64, 1, 80), (300, 65, 80), (63, 64, 1)]


@pytest.mark.parametrize("D,G,K", SHAPES)
def test_classify_equals_the_restatement(D, G, K):
    """Three images with the middle one empty; every output array equal.  The image alone gives the bytes it gives inside the batch,
    twice in a row."""
    first, empty, last = image(D, G, K, 1000 + D + G + K), image(0, 0, K, 0), image(7, 5, K, 7)
    got = launch([first, empty, last], K)
    for im, g in zip((first, empty, last), got):
        for k in KEYS:
            assert g[k].dtype == np.int32 and g[k].tolist() == im["want"][k].tolist(), k
    for _ in range(2):
        alone = launch([first], K)[0]
        for k in KEYS:
            assert alone[k].tobytes() == got[0][k].tobytes(), k
    if D >= 63 and G >= 63:
        seen = set(first["want"]["type"].tolist())
        assert {T.TP, T.LOC, T.DUPE, T.IGNORED} <= seen and (K == 1 or T.CLS in seen) and (D < 300 or len(seen) == 7), seen
        assert first["want"]["claim"].any() and (first["want"]["gt"] & T.GT_MISSED).any()


def test_hand_cases_in_one_launch():
    images = [{"det_box": np.array([d[0] for d in dets], np.float64).reshape(-1, 4), "det_cat": np.array([d[1] for d in dets], np.int32),
               "gt_box": np.array([g[0] for g in gts], np.float64).reshape(-1, 4), "gt_cat": np.array([g[1] for g in gts], np.int32),
               "gt_crowd": np.array([g[2] for g in gts], np.uint8)} for _, dets, gts, *_ in T.HAND]
    for (name, _, _, types, partners, claims, bits), got in zip(T.HAND, launch(images, 2)):
        assert (got["type"].tolist(), got["partner"].tolist(), got["claim"].tolist(), got["gt"].tolist()) == (types, partners, claims, bits), name


def test_other_thresholds_and_the_limits():
    from proben_amd._lib import HipLibraryError
    im = image(65, 65, 3, 9)
    for t_f, t_b in ((0.75, 0.25), (0.5, 0.0), (1.0, 0.5)):
        got = launch([im], 3, t_f=t_f, t_b=t_b)[0]
        want = T.classify_image(im["det_box"], im["det_cat"], im["gt_box"], im["gt_cat"], im["gt_crowd"], t_f, t_b)
        for k in KEYS:
            assert got[k].tolist() == want[k].tolist(), (t_f, t_b, k)
    big = {"det_box": np.zeros((1, 4)), "det_cat": np.zeros(1, np.int32), "gt_box": np.ones((1025, 4)), "gt_cat": np.zeros(1025, np.int32),
           "gt_crowd": np.zeros(1025, np.uint8)}
    with pytest.raises(HipLibraryError, match="1024"):
        launch([im, big], 3)


# ---- the variants through pe_ap_bootstrap, on the case of tests/ap_bootstrap_ref.py ----

@pytest.fixture(scope="module")
def case_run():
    """(classified restatement, its records, the product's typing, its lists, price() over the five vectors with the full table)."""
    from proben_amd import tide
    gt_json, results, mult = R.case()
    ds = T.classify(T.dataset(gt_json, results))
    cl = tide.classify(gt_json, results)
    lists = tide.variant_lists(cl)
    return ds, T.variant_records(ds)[0], cl, lists, tide.price(lists, mult, full_table=True)


def native(gt_json, results):
    from proben_amd.evaluation import COCOevalBBox
    ev = COCOevalBBox(gt_json, results, impl="native")
    ev.evaluate()
    ev.accumulate()
    ev.summarize(printer=None)
    return ev


def test_typing_and_lists_of_the_case_are_the_restatements(case_run):
    ds, records, cl, lists, _ = case_run
    types, missed, unmatched, conf = T.counts(ds)
    c = cl["counts"]
    assert (c["types"] == types).all() and (c["missed"] == missed).all() and (c["unmatched"] == unmatched).all() and (c["confusion"] == conf).all()
    for key, want in zip(("list_off", "list_img", "list_rank", "list_flags", "npig"), records):
        assert lists[key].tobytes() == want.tobytes(), key
    base = cl["matches"]["list_flags"][0]
    keep = ~lists["moved"]
    assert lists["list_flags"][0][keep].tobytes() == ((base & 1) | (base & (1 << 16))).astype(np.uint32).tobytes()


@pytest.mark.parametrize("vec", range(5))
def test_variants_are_the_evaluator_on_the_edited_duplicated_dataset(case_run, vec):
    """Row vec of the case's multiplicities (row 0: every image once).  Variant 0 is the native evaluator's AP50 column on the duplicated
    dataset, variants 3 to 8 the evaluator's on the edited dataset, duplicated, bit for bit; every variant (1 and 2 too) is the
    restatement's weighted accumulate bit for bit; the means are within 2 N u of summarize()'s stats[1] (N doubles added in another order
    than NumPy's pairwise sum)."""
    ds, records, _, _, run = case_run
    gt_json, results, mult = R.case()
    rec_thrs = np.linspace(0, 1, 101)
    psum, valid, p = T.psum_table(records, mult[vec], rec_thrs)
    assert run["precision"][vec].tobytes() == np.ascontiguousarray(p.transpose(1, 2, 0)).tobytes()
    assert run["psum"][vec].tobytes() == psum.tobytes() and (run["valid"][vec] == valid).all()
    assert run["ap"][vec].tobytes() == T.ap50(psum, valid, 101).tobytes()
    for v in (0, 3, 4, 5, 6, 7, 8):
        edited = (gt_json, results) if v == 0 else T.edited_dataset(gt_json, results, ds, v)
        ev = native(*R.duplicated_dataset(*edited, mult[vec]))
        want = ev.eval["precision"][0, :, :, 0, 2]                          # [R, K]
        assert np.ascontiguousarray(run["precision"][vec][:, v, :].T).tobytes() == want.tobytes(), v
        N = int(run["valid"][vec][:, v].sum()) * 101
        print(f"vector {vec} variant {v}: {run['ap'][vec, v]!r} vs {ev.stats[1]!r}, N = {N}")
        assert N > 0 and abs(run["ap"][vec, v] - ev.stats[1]) <= 2 * N * U
    if vec == 0:
        assert run["precision"][0][:, 0, :].T.tobytes() == native(gt_json, results).eval["precision"][0, :, :, 0, 2].tobytes()


# ---- the report ----

@functools.lru_cache(maxsize=None)
def reports():
    from proben_amd.tide import tide
    gt_json, a, b = R.paired_case()
    kw = dict(replicates=60, seed=1)
    return tide(gt_json, a, b, **kw), tide(gt_json, a, **kw), tide(gt_json, b, **kw), tide(gt_json, a, a, **kw)


def test_two_files_are_the_one_file_runs_and_the_paired_differences():
    from proben_amd import tide
    from proben_amd.bootstrap import paired, resample_multiplicities
    two, one_a, one_b, same = reports()
    dump = lambda x: json.dumps(x, sort_keys=True)      # noqa: E731  (NaN == NaN in the dump)
    assert dump(two["a"]) == dump(one_a["a"]) and dump(two["b"]) == dump(one_b["a"]) and "paired" not in one_a
    gt_json, a, b = R.paired_case()
    mult = resample_multiplicities(64, 60, 1)
    gains = [tide._gains(tide.price(tide.variant_lists(tide.classify(gt_json, res)), mult)["ap"]) for res in (a, b)]
    for i, r in enumerate(two["repairs"]):
        assert dump(two["paired"][r]) == dump(paired(gains[0][1:, i], gains[1][1:, i], gains[0][0, i], gains[1][0, i], np.isnan, 0.95)), r
        assert two["a"]["repairs"][r]["point"] == gains[0][0, i] and two["a"]["repairs"][r]["point"] >= 0
    for r, rec in same["paired"].items():
        assert rec["point"] == 0.0 and rec["lo"] == 0.0 and rec["hi"] == 0.0 and rec["p"] == 1.0, (r, rec)


def test_report_schema_and_the_evaluators_ap50():
    two, one_a, _, _ = reports()
    gt_json, a, _ = R.paired_case()
    ev = native(gt_json, a)
    N = 3 * 101
    assert abs(one_a["a"]["AP50"]["point"] - ev.stats[1]) <= 2 * N * U
    assert two["repairs"] == list(T.VARIANTS[1:]) and two["categories"] == [1, 2, 3] and two["threshold"] == 0.5 and two["background_iou"] == 0.1
    side = two["a"]
    assert set(side) == {"AP50", "repairs", "counts", "mixed_score_ties"} and set(side["repairs"]) == set(T.VARIANTS[1:])
    for rec in side["repairs"].values():
        assert set(rec) == {"count", "point", "lo", "hi", "se", "replicates"} and rec["replicates"] == 59 and rec["lo"] <= rec["hi"]
    ds = T.classify(T.dataset(gt_json, a))
    types, missed, unmatched, conf = T.counts(ds)
    assert side["counts"]["types"] == {name: types[t].tolist() for t, name in enumerate(two["types"])}
    assert side["counts"]["confusion"] == conf.tolist() and side["counts"]["missed"] == missed.tolist()
    assert side["repairs"]["FP"]["count"] == int(types[1:6].sum()) and side["repairs"]["FN"]["count"] == int(unmatched.sum())
    json.dumps(two)


def test_cli_prints_repairs_and_paired_rows(tmp_path, capsys):
    from fuse_inputs import dependent_files
    from proben_amd.cli import tide as cli
    root, files, _, _ = dependent_files(tmp_path)
    one = cli.main(["--dataset_path", str(root), "--predictions", files[0], "--replicates", "50"])
    out = capsys.readouterr().out
    assert "paired" not in one and "AP50" in out and all("d" + r in out for r in T.VARIANTS[1:]) and " p " not in out
    assert one["a"]["AP50"]["lo"] <= one["a"]["AP50"]["point"] <= one["a"]["AP50"]["hi"] and one["a"]["AP50"]["point"] > 0
    report = tmp_path / "report.json"
    two = cli.main(["--dataset_path", str(root), "--predictions", files[0], files[1], "--replicates", "50", "--seed", "3", "--background_iou", "0.2",
                    "--out", str(report)])
    out = capsys.readouterr().out
    assert "paired" in two and " p " in out and report.exists() and two["seed"] == 3 and two["background_iou"] == 0.2
    assert two["a"]["AP50"]["point"] == one["a"]["AP50"]["point"]
    assert json.load(open(report))["repairs"] == list(T.VARIANTS[1:])
