"""pe_ap_bootstrap (csrc/ap_bootstrap.hip) on the GPU: a replicate is the evaluator on the duplicated dataset,
bit for bit, whatever else is in the launch; the statistics; the paired mode; the CLI on a FLIR-layout folder."""
import numpy as np
import pytest

import ap_bootstrap_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def matches():
    from proben_amd.bootstrap import export_matches
    gt_json, results, _ = R.case()
    return export_matches(gt_json, results)


@pytest.fixture(scope="module")
def run_all(matches):
    """All 5 vectors of the case in one launch, full table."""
    from proben_amd.bootstrap import ap_bootstrap
    return ap_bootstrap(matches, R.case()[2], full_table=True)


def test_identity_replicate_is_the_native_evaluator(matches, run_all):
    from proben_amd.evaluation import COCOevalBBox
    gt_json, results, _ = R.case()
    ev = COCOevalBBox(gt_json, results, impl="native")
    ev.evaluate()
    ev.accumulate()
    K = len(ev.cat_ids)
    want_p = R.cells_of(ev.eval["precision"], K)          # [C, T, R]
    want_r = R.cells_of(ev.eval["recall"], K)             # [C, T]
    assert run_all["precision"][0].tobytes() == want_p.tobytes()
    assert run_all["recall"][0].tobytes() == want_r.tobytes()
    assert (run_all["valid"][0] == (want_r[:, 0] > -1)).all() and 0 < run_all["valid"][0].sum() < len(want_r)


@pytest.mark.parametrize("v", range(5))
def test_resampled_replicates_are_the_evaluator_on_the_duplicated_dataset(matches, run_all, v):
    from proben_amd.bootstrap import ap_bootstrap
    want = R.duplicated_eval(v)
    K = len(matches["evaluator"].cat_ids)
    want_p, want_r = R.cells_of(want.eval["precision"], K), R.cells_of(want.eval["recall"], K)
    alone = ap_bootstrap(matches, R.case()[2][v:v + 1], full_table=True)        # B = 1: independent of what else is in the launch
    for name, got in (("among the five", {k: run_all[k][v] for k in ("precision", "recall", "psum")}),
                      ("alone", {k: alone[k][0] for k in ("precision", "recall", "psum")})):
        assert got["precision"].tobytes() == want_p.tobytes(), name
        assert got["recall"].tobytes() == want_r.tobytes(), name
    assert alone["psum"][0].tobytes() == run_all["psum"][v].tobytes()
    # psum is the table's row added in order
    valid = want_r[:, 0] > -1
    seq = np.zeros(want_p.shape[:2])
    for r in range(want_p.shape[2]):
        seq += want_p[:, :, r]
    assert run_all["psum"][v][valid].tobytes() == seq[valid].tobytes() and (run_all["psum"][v][~valid] == 0).all()


@pytest.mark.parametrize("v", range(5))
def test_statistics_agree_with_summarize_within_the_summation_bound(matches, run_all, v):
    """Both sides are means of N doubles in [0, 1] added in different orders (summarize: NumPy's pairwise sum over the table; here: each
    cell's R values in order, then the cells): each sum is within N u of the exact one relatively, so the means differ by at most
    2 N u (u = 2^-53).  Derived, not measured.  A statistic without entries is -1 on both sides."""
    from proben_amd.bootstrap import statistics
    ev = matches["evaluator"]
    stats, class_ap = statistics(run_all, matches)
    want = R.duplicated_eval(v)
    T, Rn, K = len(ev.iou_thrs), len(ev.rec_thrs), len(ev.cat_ids)
    valid = run_all["valid"][v].reshape(K, 6) > 0
    for s, (cell, per_entry) in enumerate([(0, T * Rn), (0, Rn), (0, Rn), (1, T * Rn), (2, T * Rn), (3, T * Rn), (4, T), (5, T), (0, T), (1, T),
                                           (2, T), (3, T)]):
        N = int(valid[:, cell].sum()) * per_entry
        print(f"vector {v} statistic {s}: {stats[v, s]!r} vs {want.stats[s]!r}, N = {N}")
        if N == 0:
            assert stats[v, s] == -1.0 and want.stats[s] == -1.0
        else:
            assert abs(stats[v, s] - want.stats[s]) <= 2 * N * U
    p = want.eval["precision"][:, :, :, 0, -1]
    for k in range(K):
        if (p[:, :, k] > -1).any():
            assert abs(class_ap[v, k] - np.mean(p[:, :, k])) <= 2 * T * Rn * U
        else:
            assert np.isnan(class_ap[v, k])


def test_paired_mode():
    """The same file twice: every paired difference is exactly 0 and p = 1.  File B of ap_bootstrap_ref.paired_case against file A: the
    interval of the AP difference excludes 0 - the perturbation was chosen on the NumPy restatement, on the CPU
    (tests/test_ap_bootstrap_cpu.py::test_paired_perturbation_moves_ap_under_the_numpy_rule), not on what the kernel gives."""
    from proben_amd.bootstrap import bootstrap_ap
    from proben_amd.evaluation import COCOevalBBox
    gt_json, a, b = R.paired_case()
    same = bootstrap_ap(gt_json, a, a, replicates=200, seed=1)
    for group in ("stats", "class_ap"):
        for name, r in same["paired"][group].items():
            assert r["point"] == 0.0 and r["lo"] == 0.0 and r["hi"] == 0.0 and r["p"] == 1.0, (name, r)
    rep = bootstrap_ap(gt_json, a, b, replicates=400, seed=1)
    ev = COCOevalBBox(gt_json, a)
    ev.evaluate()
    ev.accumulate()
    assert [rep["a"]["stats"][s]["point"] for s in rep["statistics"]] == ev.summarize(printer=None).tolist()      # the evaluator's own
    d = rep["paired"]["stats"]["AP"]
    print("AP difference", d, "a", rep["a"]["stats"]["AP"], "b", rep["b"]["stats"]["AP"])
    assert d["hi"] < 0 and d["point"] < 0 and d["p"] < 0.05 and d["replicates"] == 399
    for key in ("a", "b"):
        r = rep[key]["stats"]["AP"]
        assert r["lo"] < r["hi"] and 0 < r["se"] < 0.1
    assert rep["paired"]["class_ap"]["1"]["hi"] < 0 and rep["paired"]["class_ap"]["2"]["p"] == 1.0      # only category 1 was touched
    assert rep["seed"] == 1 and rep["replicates"] == 400


def test_two_runs_give_identical_bytes(matches, run_all):
    from proben_amd.bootstrap import ap_bootstrap, resample_multiplicities
    again = ap_bootstrap(matches, R.case()[2], full_table=True)
    for k in ("psum", "recall", "valid", "precision"):
        assert again[k].tobytes() == run_all[k].tobytes(), k
    mult = resample_multiplicities(7, 64, 9)
    one, two = ap_bootstrap(matches, mult), ap_bootstrap(matches, mult)
    assert one["psum"].tobytes() == two["psum"].tobytes() and one["recall"].tobytes() == two["recall"].tobytes()
    assert len({one["psum"][b].tobytes() for b in range(64)}) > 8          # the replicates do differ


def test_cli_prints_intervals_and_paired_rows(tmp_path, capsys):
    from fuse_inputs import dependent_files
    from proben_amd.cli import bootstrap_ap as cli
    root, files, _, _ = dependent_files(tmp_path)
    one = cli.main(["--dataset_path", str(root), "--predictions", files[0], "--replicates", "50"])
    out = capsys.readouterr().out
    assert one["a"]["mixed_score_ties"] == 0 and "paired" not in one and "AP50" in out and "AP-1" in out and " p " not in out
    assert 0 < one["a"]["stats"]["AP"]["lo"] <= one["a"]["stats"]["AP"]["point"] <= one["a"]["stats"]["AP"]["hi"]
    report = tmp_path / "report.json"
    two = cli.main(["--dataset_path", str(root), "--predictions", files[0], files[1], "--replicates", "50", "--seed", "3", "--out", str(report)])
    out = capsys.readouterr().out
    assert "paired" in two and " p " in out and report.exists() and two["seed"] == 3
    assert two["a"]["stats"]["AP"]["point"] == one["a"]["stats"]["AP"]["point"]
