"""The LAMR bootstrap's host side, without a GPU: the NumPy restatement of the rule on the exported list against
KAISTPedEval on the explicitly duplicated dataset (bit for bit: this pins the equivalence argument), the corners the case is meant to
hold, the mixed-tie condition, the paired perturbation, the stratified resampler, and the argument checks of pe_lamr_bootstrap."""
import numpy as np
import pytest

import lamr_bootstrap_ref as R


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    import proben_amd
    return proben_amd._lib.lib()


@pytest.fixture(scope="module", params=[False, True], ids=["published_row_lookup", "fix_row_index"])
def exported(request):
    """(fix_row_index, matches, the NumPy rule over the six vectors and three cells)."""
    import proben_amd  # noqa: F401
    from proben_amd.lamr_bootstrap import export_lamr_matches
    annotation, results, _, mult = R.case()
    m = export_lamr_matches(annotation, results, 0, request.param)
    return request.param, m, R.rule_run(m, mult)


def test_export_is_the_evaluators_list(exported):
    from proben_amd.lamr_bootstrap import lamr_cells, mixed_score_ties
    fix, m, _ = exported
    annotation, results, _, mult = R.case()
    assert len(annotation["images"]) == 9 and mult.shape == (6, 9) and 130 <= len(results) <= 150
    assert m["img_ids"] == list(range(9)) and m["npig"].tolist() == [3, 2, 0, 0, 1, 2, 2, 0, 1] and m["npig"].dtype == np.int32
    assert m["list_img"].dtype == np.int32 and m["list_flags"].dtype == np.uint8
    assert len(m["list_img"]) == sum(R.kept(r) for r in results) >= 129           # two 64-entry chunk seams
    assert (np.diff(m["list_score"]) <= 0).all()
    ev = m["evaluator"]
    assert ev.evalImgs[2] is None and sum(e is None for e in ev.evalImgs) == 1   # no ground truth, no detection
    assert len(ev.evalImgs[3]["gtIgnore"]) == 2 and ev.evalImgs[3]["gtIgnore"].all()          # ground truth all ignored
    assert len(ev.evalImgs[8]["dtScores"]) == 0 and sum(r["image_id"] == 8 for r in results) == 5      # all outside the expanded height range
    assert len(ev.evalImgs[4]["dtScores"]) == 0 and not ev.evalImgs[4]["gtIgnore"].any()
    assert ev.evalImgs[1]["dtIgnore"].any() and ev.evalImgs[3]["dtIgnore"].any() and (m["list_flags"] == 3).sum() == 2      # matched to an ignore region
    assert lamr_cells(9, R.DAY).tolist() == [list(c) for c in R.CELLS] and lamr_cells(3).tolist() == [[0, 3], [0, 3], [3, 3]]
    assert mixed_score_ties(m) == 0
    # the ties: tp / tp across images 0 and 1, fp / fp inside image 7
    s, li, f = m["list_score"], m["list_img"], m["list_flags"]
    tie = np.flatnonzero(s[1:] == s[:-1])
    pairs = {(int(li[j]), int(li[j + 1]), int(f[j]), int(f[j + 1])) for j in tie}
    assert (0, 1, 1, 1) in pairs and (7, 7, 0, 0) in pairs
    # the night range's first counted detection is an fp
    night = np.flatnonzero((li >= R.DAY) & (f & 2 == 0))
    assert li[night[0]] == 7 and f[night[0]] == 0


def test_the_case_holds_its_corners(exported):
    """A refactor of the case must not quietly lose them: the "-1 reads the last point" rule fires, an fp of weight >= 2 straddles a
    reference, NP = 0 and N = 0 occur, MR = 1 occurs, the upper references are crossed."""
    from proben_amd.lamr_bootstrap import figures
    _, m, run = exported
    fired, totals = run["fired"], run["totals"]
    assert fired[0, 2, 0] and not fired[0, 2, -1] and not fired[0, 1].any()      # identity, night: the low references; day: its first point is a tp
    assert run["straddle"][1, 2] and not run["straddle"][0].any()                # weight 3 on image 7
    assert run["valid"][2].tolist() == [1, 1, 0] and totals[2, 2, 0] > 0 and totals[2, 2, 1] == 0       # NP = 0 with images left
    assert run["valid"][3].tolist() == [1, 1, 0] and totals[3, 2].tolist() == [0, 0, 0, 0]              # N = 0
    assert totals[3, 0, 1] > 0 and totals[3, 0, 2] + totals[3, 0, 3] == 0 and (run["tp_at"][3] == 0).all()
    assert figures(run["tp_at"][3, 0], *totals[3, 0, 1:])[0] == 1.0
    assert totals[4, 0, 0] == 263 and totals[4, 0, 3] > 255                      # image 0 at 255
    assert (totals[0, :, 3] > totals[0, :, 0]).all()                             # more fps than images: FPPI = 1 is crossed
    assert (run["pos"][0] < (totals[0, :, 2] + totals[0, :, 3])[:, None]).all()
    # the rule does make use of every reference: the nine miss rates of the identity are not all alike
    assert len(set(run["tp_at"][0, 0].tolist())) > 2


@pytest.mark.parametrize("v", range(6))
def test_numpy_rule_equals_the_evaluator_on_the_duplicated_dataset(exported, v):
    from proben_amd.lamr_bootstrap import figures
    fix, m, run = exported
    for c in range(3):
        mr, mrs, rec = figures(run["tp_at"][v, c], *(int(x) for x in run["totals"][v, c, 1:]))
        want_mr, want_mrs, want_rec = R.duplicated_figures(v, c, fix)
        print(f"vector {v} cell {c}: MR {mr!r} vs {want_mr!r}, recall {rec!r} vs {want_rec!r}, totals {run['totals'][v, c].tolist()}")
        assert np.float64(mr).tobytes() == want_mr.tobytes(), (c, mr, want_mr)
        assert np.asarray(mrs, dtype=np.float64).tobytes() == want_mrs.tobytes(), (c, mrs, want_mrs)
        assert np.float64(rec).tobytes() == want_rec.tobytes(), (c, rec, want_rec)


def test_identity_is_evaluate_itself(exported, tmp_path, capsys):
    """Row 0 is the dataset: the three figures evaluate() prints at DAY_FRAMES = 1455 are the cells of lamr_cells(9) - everything is day."""
    import json
    from proben_amd.evalKAIST.evaluation_script import evaluate
    from proben_amd.lamr_bootstrap import figures, lamr_cells, point_estimates, subset_evaluators
    fix, m, _ = exported
    annotation, results, _, mult = R.case()
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(annotation))
    res = evaluate(str(path), results, fix_row_index=fix)
    capsys.readouterr()
    thr = m["evaluator"].params.fppiThrs
    for sub, cell in zip(("all", "day", "night"), lamr_cells(9).tolist()):
        r = R.numpy_rule(m["list_img"], m["list_flags"], m["npig"], mult[0], cell, thr)
        mr = figures(r["tp_at"], *(int(x) for x in r["totals"][1:]))[0]
        assert mr == res[sub].summarize(0), sub
    for sub_ev, c in zip(subset_evaluators(m, R.CELLS), range(3)):
        want = R.duplicated_figures(0, c, fix)
        got = point_estimates(sub_ev, 0)
        assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]


def test_mixed_score_ties_are_counted():
    """A tp and an fp that tie in score inside one image: drawn twice, the weighted list (tp tp fp fp) and the duplicated image
    (tp fp tp fp) differ at the references below 1 / N, and mixed_score_ties counts the pair."""
    import proben_amd  # noqa: F401
    from proben_amd.lamr_bootstrap import export_lamr_matches, figures, mixed_score_ties
    annotation, results, _, _ = R.case()
    gt = next(a for a in annotation["annotations"] if a["image_id"] == 0)
    res = [{"image_id": 0, "category_id": 1, "bbox": list(gt["bbox"]), "score": 2.0},
           {"image_id": 0, "category_id": 1, "bbox": [560.0, 380.0, 40.0, 80.0], "score": 2.0}] + [dict(r) for r in results]
    m = export_lamr_matches(annotation, res, 0, True)
    assert mixed_score_ties(m) == 1
    thr = m["evaluator"].params.fppiThrs
    for mult, same in (([1] * 9, True), ([2] + [1] * 8, False)):
        r = R.numpy_rule(m["list_img"], m["list_flags"], m["npig"], mult, (0, 9), thr)
        got = figures(r["tp_at"], *(int(x) for x in r["totals"][1:]))
        ann2, res2 = R.duplicated_dataset(annotation, res, mult)
        want = R.evaluator_figures(ann2, res2, [im["id"] for im in ann2["images"]], True)
        assert (got[1].tobytes() == want[1].tobytes()) == same, (mult, got, want)


def test_paired_perturbation_moves_mr_under_the_numpy_rule():
    """File B (A without its jittered copies of the pedestrians: two true positives are left) was chosen here, on the NumPy rule, before the
    kernel saw it: over 400 seeded resamples the 95 % percentile interval of the paired MR difference B - A on `all` excludes 0."""
    import proben_amd  # noqa: F401
    from proben_amd.bootstrap import resample_multiplicities
    from proben_amd.lamr_bootstrap import export_lamr_matches, figures
    annotation, a, b, _ = R.case()
    mult = resample_multiplicities(9, 401, 1)[1:]
    mr = []
    for res in (a, b):
        m = export_lamr_matches(annotation, res, 0, False)
        thr = m["evaluator"].params.fppiThrs
        runs = [R.numpy_rule(m["list_img"], m["list_flags"], m["npig"], v, (0, 9), thr) for v in mult]
        mr.append(np.array([figures(r["tp_at"], *(int(x) for x in r["totals"][1:]))[0] for r in runs]))
    ok = (mr[0] > -1) & (mr[1] > -1)
    d = (mr[1] - mr[0])[ok]
    lo, hi = np.quantile(d, 0.025), np.quantile(d, 0.975)
    print("MR a", mr[0][ok].mean(), "MR b", mr[1][ok].mean(), "difference: interval", lo, hi, "defined", int(ok.sum()))
    assert lo > 0 and ok.sum() > 390


def test_resample_multiplicities_stratified():
    import proben_amd  # noqa: F401
    from proben_amd.lamr_bootstrap import lamr_cells, resample_multiplicities_stratified
    bounds = lamr_cells(2252)[1:]
    m = resample_multiplicities_stratified(bounds, 40, 3)
    assert m.shape == (40, 2252) and m.dtype == np.int64 and (m >= 0).all() and (m[0] == 1).all() and not (m[1] == 1).all()
    assert (m[:, :1455].sum(1) == 1455).all() and (m[:, 1455:].sum(1) == 797).all()
    assert m.tobytes() == resample_multiplicities_stratified(bounds, 40, 3).tobytes()
    assert m.tobytes() != resample_multiplicities_stratified(bounds, 40, 4).tobytes()
    one = resample_multiplicities_stratified(lamr_cells(9, 20)[1:], 5, 0)           # an empty night stratum
    assert one.shape == (5, 9) and (one.sum(1) == 9).all()
    assert resample_multiplicities_stratified([(0, 4), (4, 9)], 1, 0).tolist() == [[1] * 9]
    for bad in ([], [(1, 4)], [(0, 4), (5, 9)], [(0, 4), (4, 3)], [(0, 0)]):
        with pytest.raises(ValueError):
            resample_multiplicities_stratified(bad, 5, 0)


def test_argument_checks_answer_without_a_gpu(lib):
    """Every limit and null-pointer case of include/proben_hip.h, by status and message, before any device work."""
    from proben_amd.lamr_bootstrap import export_lamr_matches, lamr_bootstrap
    err = lambda: lib.pe_last_error().decode()      # noqa: E731
    p = 4096      # never dereferenced: the checks come before any GPU call
    names = "img flags n npig mult B I thr R cells C tp_at totals valid stream".split()
    ok = [p, p, 134, p, p, 6, 9, p, 9, p, 3, p, p, p, None]
    bad = lambda **kw: lib.pe_lamr_bootstrap(*[kw.get(k, x) for k, x in zip(names, ok)])      # noqa: E731
    assert bad(C=17) == -2 and "C 17 > 16" in err()                        # PE_ERR_UNSUPPORTED
    assert bad(R=17) == -2 and "R 17 > 16" in err()
    assert bad(I=32769) == -2 and "I 32769 > 32768" in err()
    assert bad(n=(2 ** 31 - 1) // 255 + 1) == -2 and "n_list" in err()
    assert bad(B=2 ** 30, C=2) == -2 and "B * C" in err()
    assert bad(B=0) == 0 and bad(C=0) == 0 and bad(B=0, mult=None, tp_at=None) == 0      # nothing to do
    assert bad(B=-1) == -1 and "bad sizes" in err()                        # PE_ERR_INVALID_ARG
    assert bad(C=-1) == -1 and bad(I=0) == -1 and bad(R=0) == -1 and bad(n=-1) == -1
    for k in ("npig", "mult", "thr", "cells", "tp_at", "totals", "valid"):
        assert bad(**{k: None}) == -1 and "null pointer (npig" in err(), k
    assert bad(img=None) == -1 and "list_img / list_flags" in err()
    assert bad(flags=None) == -1 and "list_img / list_flags" in err()
    annotation, results, _, mult = R.case()
    m = export_lamr_matches(annotation, results)
    for wrong in (mult + 255, -mult - 1, mult[:, :8], mult.astype(np.float64)):
        with pytest.raises(ValueError):
            lamr_bootstrap(m, wrong, R.CELLS, device="cuda")              # refused before the device is touched


def test_cli_parsers():
    import proben_amd  # noqa: F401
    from proben_amd.cli import bootstrap_lamr as cli
    from proben_amd.cli import demo_LAMR_KAIST as demo
    a = demo.parser().parse_args(["--dataset_path", "D"])
    assert a.bootstrap == 0
    assert demo.parser().parse_args(["--dataset_path", "D", "--bootstrap", "500"]).bootstrap == 500
    a = cli.parse(["--annotation_json", "G.json", "--results", "A.txt"])
    assert (a.replicates, a.seed, a.confidence, a.setups, a.fix_row_index, a.day_frames, a.stratified, a.out, a.results) == \
        (2000, 0, 0.95, (0,), False, 1455, False, None, ["A.txt"])
    a = cli.parse(["--annotation_json", "G.json", "--results", "A.txt", "B.txt", "--replicates", "100", "--seed", "5", "--confidence", "0.9",
                   "--setups", "0,1,2,3", "--fix-row-index", "--day_frames", "5", "--stratified", "--out", "r.json"])
    assert (a.replicates, a.seed, a.confidence, a.setups, a.fix_row_index, a.day_frames, a.stratified, a.out, a.results) == \
        (100, 5, 0.9, (0, 1, 2, 3), True, 5, True, "r.json", ["A.txt", "B.txt"])
    for bad in (["--results", "A", "B", "C"], ["--results", "A", "--replicates", "1"], ["--results", "A", "--confidence", "1.0"],
                ["--results", "A", "--setups", "4"], ["--results", "A", "--setups", "x"], []):
        with pytest.raises(SystemExit):
            cli.parse(["--annotation_json", "G.json"] + bad)


def test_demo_without_bootstrap_writes_todays_summary(tmp_path, capsys):
    """--bootstrap 0 (the default) leaves the summary file and the printout as they were: no interval keys, no call into the bootstrap."""
    import json
    import proben_amd  # noqa: F401
    from proben_amd.cli import demo_LAMR_KAIST as demo
    annotation, _, _, _ = R.case()
    gt = tmp_path / "gt.json"
    gt.write_text(json.dumps(annotation))
    args = demo.parser().parse_args(["--dataset_path", "D", "--annotation_json", str(gt), "--out_folder", str(tmp_path), "--bootstrap", "0"])
    result = demo._write_and_score(args, [], [], str(tmp_path / "KAIST_thermal_only_result.txt"), None, 1)
    out = capsys.readouterr().out
    assert "interval" not in out and not any("interval" in k for k in result)
    assert sorted(json.load(open(tmp_path / "KAIST_thermal_only_summary.json"))) == sorted(
        ["rows", "frames", "txt", "world_size", "log_average_miss_rate", "MR_all", "MR_day", "MR_night", "recall_all", "miss_rate_at_fppi"])
