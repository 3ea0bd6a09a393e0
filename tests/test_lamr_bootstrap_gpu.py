"""pe_lamr_bootstrap (csrc/lamr_bootstrap.hip) on the GPU: the kernel's integers are the NumPy rule's, a replicate is
KAISTPedEval on the duplicated dataset bit for bit whatever else is in the launch, at every chunk seam; the paired mode; the CLI."""
import json

import numpy as np
import pytest

import lamr_bootstrap_ref as R

pytestmark = pytest.mark.gpu

SEAMS = (0, 1, 63, 64, 65, 128, 129)


@pytest.fixture(scope="module", params=[False, True], ids=["published_row_lookup", "fix_row_index"])
def launched(request):
    """(fix_row_index, matches, all six vectors and three cells in one launch)."""
    from proben_amd.lamr_bootstrap import export_lamr_matches, lamr_bootstrap
    annotation, results, _, mult = R.case()
    m = export_lamr_matches(annotation, results, 0, request.param)
    return request.param, m, lamr_bootstrap(m, mult, R.CELLS)


def assert_same_integers(run, want):
    for k in ("tp_at", "totals", "valid"):
        assert run[k].dtype == want[k].dtype and run[k].shape == want[k].shape, k
        np.testing.assert_array_equal(run[k], want[k], err_msg=k)


def assert_is_the_duplicated_evaluator(run, fix, n_entries=None, vectors=range(6)):
    from proben_amd.lamr_bootstrap import lamr_statistics
    stats = lamr_statistics(run)
    for v in vectors:
        for c in range(3):
            mr, mrs, rec = R.duplicated_figures(v, c, fix, n_entries)
            assert stats["MR"][v, c].tobytes() == mr.tobytes(), (v, c, stats["MR"][v, c], mr)
            assert stats["miss_rates"][v, c].tobytes() == mrs.tobytes(), (v, c, stats["miss_rates"][v, c], mrs)
            assert stats["recall_all"][v, c].tobytes() == rec.tobytes(), (v, c, stats["recall_all"][v, c], rec)


def test_integers_equal_the_numpy_rule(launched):
    _, m, run = launched
    assert run["tp_at"].shape == (6, 3, 9) and run["totals"].shape == (6, 3, 4) and run["valid"].shape == (6, 3)
    assert_same_integers(run, R.rule_run(m, R.case()[3]))
    assert (run["valid"] == 0).sum() == 2 and (run["valid"] == 1).sum() == 16


def test_statistics_equal_the_evaluator_on_the_duplicated_dataset(launched):
    fix, _, run = launched
    assert_is_the_duplicated_evaluator(run, fix)


def test_alone_as_among_the_others_and_twice_the_same(launched):
    from proben_amd.lamr_bootstrap import lamr_bootstrap
    _, m, run = launched
    mult = R.case()[3]
    for v in range(6):
        alone = lamr_bootstrap(m, mult[v:v + 1], R.CELLS)                          # B = 1
        for k in ("tp_at", "totals", "valid"):
            assert alone[k][0].tobytes() == run[k][v].tobytes(), (v, k)
    night = lamr_bootstrap(m, mult, R.CELLS[2:])                                   # one cell of the three
    again = lamr_bootstrap(m, mult, R.CELLS)
    for k in ("tp_at", "totals", "valid"):
        assert night[k][:, 0].tobytes() == np.ascontiguousarray(run[k][:, 2]).tobytes(), k
        assert again[k].tobytes() == run[k].tobytes(), k


@pytest.mark.parametrize("n_entries", SEAMS)
def test_chunk_seams(n_entries):
    """The result rows truncated so that the exported list has 0, 1, 63, 64, 65, 128 and 129 entries: the kernel's integers are the
    rule's and the statistics the duplicated evaluator's, as on the whole list."""
    from proben_amd.lamr_bootstrap import lamr_bootstrap
    m = R.truncated_matches(n_entries)
    mult = R.case()[3]
    run = lamr_bootstrap(m, mult, R.CELLS)
    assert_same_integers(run, R.rule_run(m, mult))
    assert_is_the_duplicated_evaluator(run, False, n_entries, vectors=(0, 1, 5))


def test_a_bad_cell_raises_through_the_wrapper(launched):
    from proben_amd.lamr_bootstrap import lamr_bootstrap
    _, m, _ = launched
    mult = R.case()[3]
    for cells in ([[0, 9], [5, 4]], [[0, 10]], [[-1, 3]]):
        with pytest.raises(ValueError, match="image-index range"):
            lamr_bootstrap(m, mult, cells)
    edge = lamr_bootstrap(m, mult[:1], [[9, 9], [0, 0], [4, 5]])                   # empty ranges and a single image are cells
    assert edge["valid"].tolist() == [[0, 0, 1]] and edge["totals"][0].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0]]


def test_paired_mode():
    """The same file twice: every paired difference is exactly 0 and p = 1.  File B against file A under the resamples of
    tests/test_lamr_bootstrap_cpu.py::test_paired_perturbation_moves_mr_under_the_numpy_rule, where the sign was fixed on the CPU: the
    interval of the MR difference excludes 0.  The point estimates are KAISTPedEval's own over each subset's image ids."""
    from proben_amd.lamr_bootstrap import bootstrap_lamr
    annotation, a, b, _ = R.case()
    same = bootstrap_lamr(annotation, a, a, replicates=200, seed=2, day_frames=R.DAY)
    for sub, r in same["paired"]["setups"]["0"].items():
        for rec in [r["MR"], r["recall"]] + r["miss_rate_at_fppi"]:
            assert rec["point"] == 0.0 and rec["lo"] == 0.0 and rec["hi"] == 0.0 and rec["p"] == 1.0, (sub, rec)
    rep = bootstrap_lamr(annotation, a, b, replicates=401, seed=1, day_frames=R.DAY)
    ids = [im["id"] for im in annotation["images"]]
    for key, res in (("a", a), ("b", b)):
        for c, sub in enumerate(("all", "day", "night")):
            mr, mrs, rec = R.evaluator_figures(annotation, res, ids[R.CELLS[c][0]:R.CELLS[c][1]])
            got = rep[key]["setups"]["0"][sub]
            assert got["MR"]["point"] == mr and [x["point"] for x in got["miss_rate_at_fppi"]] == mrs.tolist() and got["recall"]["point"] == rec
    d = rep["paired"]["setups"]["0"]["all"]["MR"]
    print("MR difference", d, "a", rep["a"]["setups"]["0"]["all"]["MR"], "b", rep["b"]["setups"]["0"]["all"]["MR"])
    assert d["lo"] > 0 and d["point"] > 0 and d["p"] < 0.05 and d["replicates"] == 400
    for key in ("a", "b"):
        r = rep[key]["setups"]["0"]["all"]["MR"]
        assert r["lo"] < r["hi"] and 0 < r["se"] < 0.5
    assert rep["seed"] == 1 and rep["replicates"] == 401 and rep["a"]["mixed_score_ties"] == {"0": 0}


def test_demo_bootstrap_flag_adds_the_intervals(tmp_path, capsys):
    """demo_LAMR_KAIST --bootstrap N: the writer and scorer with the case's rows as float32 detections; the summary gains the three
    interval keys beside the figures it had (9 images are all day at 1455 day frames: the night interval has no defined resample)."""
    import math
    from proben_amd.cli import demo_LAMR_KAIST as demo
    annotation, a, _, _ = R.case()
    gt = tmp_path / "gt.json"
    gt.write_text(json.dumps(annotation))
    table = [[r["image_id"], r["bbox"][0], r["bbox"][1], r["bbox"][0] + r["bbox"][2], r["bbox"][1] + r["bbox"][3], r["score"], 1.0] for r in a]
    insts = demo.rows_to_frames(table, 9)
    args = demo.parser().parse_args(["--dataset_path", "D", "--annotation_json", str(gt), "--out_folder", str(tmp_path), "--bootstrap", "60"])
    result = demo._write_and_score(args, [], insts, str(tmp_path / "KAIST_thermal_only_result.txt"), None, 1)
    out = capsys.readouterr().out
    summary = json.load(open(tmp_path / "KAIST_thermal_only_summary.json"))
    for k in ("all", "day"):
        lo, hi = summary[f"MR_{k}_interval"]
        assert result[f"MR_{k}_interval"] == [lo, hi] and 0.0 <= lo <= hi <= 1.0 and 0.0 <= summary[f"MR_{k}"] <= 1.0
        assert f"MR_{k}: {100 * summary['MR_' + k]:.2f}  95 % interval" in out
    assert all(math.isnan(x) for x in summary["MR_night_interval"]) and summary["MR_night"] == -1.0


def test_cli_prints_intervals_and_paired_rows(tmp_path, capsys):
    from proben_amd.cli import bootstrap_lamr as cli
    annotation, a, b, _ = R.case()
    gt = tmp_path / "KAIST_annotation.json"
    gt.write_text(json.dumps(annotation))
    files = []
    for name, res in (("A", a), ("B", b)):
        files.append(str(tmp_path / f"KAIST_{name}_result.txt"))
        with open(files[-1], "w") as f:
            f.write("".join(f"{r['image_id'] + 1},{','.join(repr(v) for v in r['bbox'])},{r['score']!r}\n" for r in res))
    base = ["--annotation_json", str(gt), "--day_frames", str(R.DAY), "--replicates", "50"]
    one = cli.main(base + ["--results", files[0], "--setups", "0,3"])
    out = capsys.readouterr().out
    assert "paired" not in one and " p " not in out and "Reasonable" in out and "All" in out and "night" in out
    assert sorted(one["a"]["setups"]) == ["0", "3"] and one["a"]["mixed_score_ties"] == {"0": 0, "3": 0}
    mr, _, _ = R.evaluator_figures(annotation, a, list(range(9)))
    assert one["a"]["setups"]["0"]["all"]["MR"]["point"] == mr                    # the text rows round-trip: the same figure as from the dicts
    report = tmp_path / "report.json"
    two = cli.main(base + ["--results", files[0], files[1], "--seed", "3", "--stratified", "--out", str(report)])
    out = capsys.readouterr().out
    assert "paired" in two and " p " in out and report.exists() and two["seed"] == 3 and two["stratified"]
    assert sorted(json.load(open(report))["paired"]["setups"]["0"]) == ["all", "day", "night"]
    for rep in (one, two):
        for sub, r in rep["a"]["setups"]["0"].items():
            assert r["MR"]["lo"] <= r["MR"]["hi"] and 0.0 <= r["MR"]["point"] <= 1.0 and 0.0 <= r["MR"]["lo"] and r["MR"]["hi"] <= 1.0, (sub, r)
