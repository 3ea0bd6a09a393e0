"""The bootstrap's host side, without a GPU: the exported match lists against the NumPy evaluator's records,
the weighted accumulate rule against the evaluator on the explicitly duplicated dataset (bit for bit: this pins the equivalence
argument), the resampler, the argument checks of both entry points and the CLI's."""
import ctypes
import json

import numpy as np
import pytest

import ap_bootstrap_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.lib()


@pytest.fixture(scope="module")
def matches(lib):
    from proben_amd.bootstrap import export_matches
    gt_json, results, _ = R.case()
    return export_matches(gt_json, results)


def test_case_has_what_it_is_meant_to_have(matches):
    gt_json, results, mult = R.case()
    assert len(gt_json["images"]) == 7 and len(gt_json["categories"]) == 2 and mult.shape == (5, 7)
    off, npig = matches["list_off"], matches["npig"]
    assert off.tolist() == [0, 129, 194]
    assert (npig[0].sum(1) > 0).all() and npig[1, 3].sum() == 0 and (npig[1, :3].sum(1) > 0).all()      # every range; category 2 has no large box
    dets = {i: [r for r in results if r["image_id"] == i] for i in range(1, 8)}
    gts = {i: [a for a in gt_json["annotations"] if a["image_id"] == i] for i in range(1, 8)}
    assert not dets[4] and gts[4] and dets[7] and not gts[7] and sum(a["iscrowd"] for a in gt_json["annotations"]) == 1
    assert (mult[2][[i - 1 for i in range(1, 8) if any(a["category_id"] == 1 for a in gts[i])]] == 0).all() and mult[2].sum() > 0
    assert 0 in mult[1] and 3 in mult[1] and np.count_nonzero(mult[3]) == 1 and (mult[0] == 1).all()
    s1 = [r["score"] for r in dets[1] if r["category_id"] == 1]
    s2 = [r["score"] for r in dets[2] if r["category_id"] == 1]
    s7 = [r["score"] for r in dets[7] if r["category_id"] == 1]
    assert set(s1) & set(s2) and len(set(s7)) == len(s7) - 1 and len(s1) > 10


def test_exported_matches_are_the_numpy_evaluators_records(matches):
    from proben_amd.evaluation import COCOevalBBox
    gt_json, results, _ = R.case()
    want = R.numpy_records(COCOevalBBox(gt_json, results, impl="numpy"))
    for name, w in zip(("list_off", "list_img", "list_rank", "list_flags", "npig"), want):
        got = matches[name]
        assert got.dtype == w.dtype and got.shape == w.shape, name
        np.testing.assert_array_equal(got, w, err_msg=name)
    assert (matches["list_flags"] != 0).any() and (matches["list_flags"] >> 16).any()


@pytest.mark.parametrize("v", range(5))
def test_weighted_rule_equals_the_evaluator_on_the_duplicated_dataset(matches, v):
    _, _, mult = R.case()
    ev = matches["evaluator"]
    want = R.duplicated_eval(v)
    records = tuple(matches[k] for k in ("list_off", "list_img", "list_rank", "list_flags", "npig"))
    precision, recall = R.weighted_accumulate(records, mult[v], ev.rec_thrs, len(ev.iou_thrs), ev.max_dets)
    assert precision.tobytes() == want.eval["precision"].tobytes()
    assert recall.tobytes() == want.eval["recall"].tobytes()
    if v == 2:        # no ground truth of category 1 is left: its cells are -1
        assert (precision[:, :, 0] == -1).all() and (precision[:, :, 1, 0] > -1).all()
    assert (precision[:, :, 1, 3] == -1).all()


def test_mixed_score_ties_are_counted(matches):
    """The case meets section 27's condition (its tie inside image 7 is between two unmatched boxes).  A tie between a match and an
    unmatched box inside one image does not, and is counted: there the weighted list (xx yy) and the duplicated image (xy xy) differ."""
    import copy
    from proben_amd.bootstrap import export_matches, mixed_score_ties
    assert mixed_score_ties(matches) == 0
    gt_json, results, _ = R.case()
    gt = next(a for a in gt_json["annotations"] if a["image_id"] == 1 and a["category_id"] == 1 and not a["iscrowd"])
    res = copy.deepcopy(results) + [{"image_id": 1, "category_id": 1, "bbox": list(gt["bbox"]), "score": 2.0},
                                    {"image_id": 1, "category_id": 1, "bbox": [600.0, 470.0, 30.0, 30.0], "score": 2.0}]
    m = export_matches(gt_json, res)
    assert mixed_score_ties(m) == 1
    records = tuple(m[k] for k in ("list_off", "list_img", "list_rank", "list_flags", "npig"))
    ev = m["evaluator"]
    for mult, same in (([1] * 7, True), ([2, 1, 1, 1, 1, 1, 1], False)):
        want = R.COCOevalBBox_on(*R.duplicated_dataset(gt_json, res, mult))
        got = R.weighted_accumulate(records, mult, ev.rec_thrs, len(ev.iou_thrs), ev.max_dets)[0]
        assert (got.tobytes() == want.eval["precision"].tobytes()) == same


def test_identity_vector_is_the_native_evaluator(matches):
    from proben_amd.evaluation import COCOevalBBox
    gt_json, results, mult = R.case()
    ev = COCOevalBBox(gt_json, results)
    ev.evaluate()
    ev.accumulate()
    records = tuple(matches[k] for k in ("list_off", "list_img", "list_rank", "list_flags", "npig"))
    precision, recall = R.weighted_accumulate(records, mult[0], ev.rec_thrs, len(ev.iou_thrs), ev.max_dets)
    assert precision.tobytes() == ev.eval["precision"].tobytes() and recall.tobytes() == ev.eval["recall"].tobytes()


def test_resample_multiplicities():
    from proben_amd.bootstrap import resample_multiplicities
    m = resample_multiplicities(1366, 50, 3)
    assert m.shape == (50, 1366) and m.dtype == np.int64 and (m >= 0).all()
    assert (m.sum(1) == 1366).all() and (m[0] == 1).all() and not (m[1] == 1).all()
    assert m.tobytes() == resample_multiplicities(1366, 50, 3).tobytes()
    assert m.tobytes() != resample_multiplicities(1366, 50, 4).tobytes()
    assert resample_multiplicities(5, 1, 0).tolist() == [[1] * 5]
    with pytest.raises(ValueError):
        resample_multiplicities(0, 5, 0)


def test_argument_checks_answer_without_a_gpu(lib, matches):
    from proben_amd.bootstrap import ap_bootstrap
    ev = matches["evaluator"]
    err = lambda: lib.pe_last_error().decode()      # noqa: E731
    args = ev._native_arrays()
    outs = [matches[k].copy() for k in ("list_off", "list_img", "list_rank", "list_flags", "npig")]
    call = lambda a: lib.pe_cocoeval_bbox_matches(*[x.ctypes.data_as(ctypes.c_void_p) if isinstance(x, np.ndarray) else x for x in a])      # noqa: E731
    assert call(args + outs) == 0
    t17 = list(args)
    t17[14], t17[15] = np.linspace(0.1, 0.9, 17), 17
    assert call(t17 + outs) == -2 and "17" in err()                       # PE_ERR_UNSUPPORTED
    assert call(args + [outs[0], None] + outs[2:]) == -1 and "null pointer" in err()
    assert call(args + [None] + outs[1:]) == -1
    # pe_ap_bootstrap: (list_off, list_img, list_rank, list_flags, stride, npig, mult, B, I, K, A, T, rec_thrs, R, cells, C, psum, recall, valid, precision, stream)
    p = 4096      # never dereferenced: the checks come before any GPU call
    ok = [p, p, p, p, 194, p, p, 5, 7, 2, 4, 10, p, 101, p, 12, p, p, p, None, None]
    bad = lambda **kw: lib.pe_ap_bootstrap(*[kw.get(i, x) for i, x in zip("off img rank flags stride npig mult B I K A T thr R cells C psum recall valid prec stream".split(), ok)])      # noqa: E731
    assert bad(T=17) == -2 and "T 17" in err()
    assert bad(R=129) == -2 and bad(I=32769) == -2 and bad(stride=2 ** 31 // 255 + 1) == -2
    assert bad(img=None) == -1 and "list_img" in err()
    assert bad(mult=None) == -1 and bad(T=0) == -1 and bad(I=0) == -1 and bad(B=-1) == -1
    assert bad(B=0) == 0                                                  # nothing to do
    _, _, mult = R.case()
    for wrong in (mult + 255, -mult - 1, mult[:, :6], mult.astype(np.float64)):
        with pytest.raises(ValueError):
            ap_bootstrap(matches, wrong, device="cuda")                   # refused before the device is touched


def test_cli_parsing_and_mismatched_image_sets(tmp_path):
    from proben_amd.bootstrap import bootstrap_ap, check_same_images
    from proben_amd.cli import bootstrap_ap as cli
    a = cli.parse(["--dataset_path", "D", "--predictions", "A.json"])
    assert (a.replicates, a.seed, a.confidence, a.out, a.predictions) == (2000, 0, 0.95, None, ["A.json"])
    a = cli.parse(["--dataset_path", "D", "--predictions", "A.json", "B.json", "--replicates", "100", "--seed", "5", "--confidence", "0.9",
                   "--out", "r.json"])
    assert (a.replicates, a.seed, a.confidence, a.out, a.predictions) == (100, 5, 0.9, "r.json", ["A.json", "B.json"])
    for bad in (["--predictions", "A", "B", "C"], ["--predictions", "A", "--replicates", "1"], ["--predictions", "A", "--confidence", "1.0"], []):
        with pytest.raises(SystemExit):
            cli.parse(["--dataset_path", "D"] + bad)
    check_same_images([1, 2, 3], [3, 2, 1])
    with pytest.raises(ValueError, match="same images"):
        check_same_images([1, 2, 3], [1, 2])
    gt_json, results, _ = R.case()
    keys = ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")
    files = []
    for name, ids in (("a", [1, 2, 3]), ("b", [1, 2, 4]), ("c", [1, 2, 99])):
        pred = {k: [[] for _ in ids] for k in keys}
        pred["image_id"], pred["image"] = ids, [f"{i}.jpeg" for i in ids]
        files.append(str(tmp_path / f"{name}.json"))
        json.dump(pred, open(files[-1], "w"))
    assert cli.load(gt_json, files[:1]) == [[]]
    with pytest.raises(ValueError, match="same images"):
        cli.load(gt_json, files[:2])
    with pytest.raises(ValueError, match="does not have"):
        cli.load(gt_json, files[2:])
    with pytest.raises(ValueError, match="does not have"):
        bootstrap_ap(gt_json, results + [dict(results[0], image_id=99)], replicates=10)


def test_paired_perturbation_moves_ap_under_the_numpy_rule(lib):
    """The perturbation of ap_bootstrap_ref.paired_case was chosen here, on the NumPy restatement, before the kernel saw it: over 100
    resamples the paired AP difference B - A is below 0 in every one, so its percentile interval excludes 0 (the GPU test asserts
    the same of the kernel over more resamples)."""
    from proben_amd.bootstrap import export_matches, resample_multiplicities
    gt_json, a, b = R.paired_case()
    mult = resample_multiplicities(64, 101, 0)[1:]
    ap = []
    for res in (a, b):
        m = export_matches(gt_json, res)
        ev = m["evaluator"]
        rec = tuple(m[k] for k in ("list_off", "list_img", "list_rank", "list_flags", "npig"))
        ap.append([np.mean(p[p > -1]) for p in (R.weighted_accumulate(rec, v, ev.rec_thrs, len(ev.iou_thrs), ev.max_dets, only={(0, 2)})[0][:, :, :, 0, 2]
                                                for v in mult)])
    d = np.array(ap[1]) - np.array(ap[0])
    print("AP a", np.mean(ap[0]), "AP b", np.mean(ap[1]), "difference: max", d.max(), "97.5 %", np.quantile(d, 0.975))
    assert np.quantile(d, 0.975) < 0 and d.max() < 0


def test_prediction_file_rows_take_the_evaluators_whitelist_and_conversion():
    from proben_amd.evaluation import prediction_file_results
    gt_json, _, _ = R.case()
    pred = {"image_id": [3, 5], "boxes": [[[10.0, 20.0, 50.0, 80.0], [1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 8.0, 8.0]], []],
            "scores": [[0.9, 0.8, 0.7], []], "classes": [[0, 3, 1], []]}
    rows = prediction_file_results(pred, gt_json)
    assert rows == [{"image_id": 3, "category_id": 1, "bbox": [10.0, 20.0, 40.0, 60.0], "score": pytest.approx(0.9, rel=1e-7)},
                    {"image_id": 3, "category_id": 2, "bbox": [0.0, 0.0, 8.0, 8.0], "score": pytest.approx(0.7, rel=1e-7)}]
