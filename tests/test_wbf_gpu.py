"""pe_wbf_fuse_batch (csrc/wbf.hip) on the GPU.  Every output is compared with wbf_ref.numpy_rule bit for bit -
boxes, scores and classes by tobytes(), counts, cluster, members and skipped as integers -, with no tolerance: the kernel runs the
rule's float64 operations in the rule's order."""
import json

import numpy as np
import pytest
import torch

import wbf_ref as W

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def image(boxes, scores, classes, source, **kw):
    return dict(boxes=np.asarray(boxes, dtype=np.float64).reshape(-1, 4), scores=np.asarray(scores, dtype=np.float64),
                classes=np.asarray(classes, dtype=np.int32), source=np.asarray(source, dtype=np.int32), **kw)


def run(images, u, thr, skip, K, max_rows=None):
    """One fuse_batch launch over `images`; every output on the host, per image."""
    from proben_amd import fusion as F
    cat = lambda k: np.concatenate([im[k] for im in images])  # noqa: E731
    offs = np.concatenate([[0], np.cumsum([len(im["scores"]) for im in images])]).astype(np.int32)
    out = F.fuse_batch(dev(cat("boxes").reshape(-1, 4)), dev(cat("scores")), None, None, dev(cat("classes")), dev(offs), "wbf", "wbf",
                       max_rows=max_rows, iou_thresh=thr, row_source=dev(cat("source")), wbf_weights=u, wbf_skip=skip, num_classes=K)
    torch.cuda.synchronize()
    assert set(out) == {"boxes", "scores", "classes", "counts", "cluster", "members", "skipped"}
    host = {k: v.cpu().numpy() for k, v in out.items()}
    res = []
    for b in range(len(images)):
        m = int(host["counts"][b])
        sl = slice(offs[b], offs[b] + max(m, 0))
        res.append({"count": m, "skipped": int(host["skipped"][b]), "boxes": host["boxes"][sl], "scores": host["scores"][sl],
                    "classes": host["classes"][sl], "members": host["members"][sl], "cluster": host["cluster"][offs[b]:offs[b + 1]]})
    return res


def same(got, want, what=""):
    assert got["count"] == want["count"] and got["skipped"] == want["skipped"], (what, got["count"], want["count"], got["skipped"], want["skipped"])
    assert got["boxes"].dtype == np.float64 and got["scores"].dtype == np.float32 and got["classes"].dtype == np.float32
    for k in ("boxes", "scores", "classes"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    assert got["members"].tolist() == want["members"].tolist() and got["cluster"].tolist() == want["cluster"].tolist(), what


def check(images, u, thr=0.55, skip=0.0, K=3, max_rows=None):
    got = run(images, u, thr, skip, K, max_rows)
    want = [W.numpy_rule(im["boxes"], im["scores"], im["classes"], im["source"], u, thr, skip, K) for im in images]
    for b, (g, w) in enumerate(zip(got, want)):
        same(g, w, b)
    return got, want


_SETS = {}


def random_set(seed, max_rows=130, K=3):
    """The seeded sets of the CPU test's kind at 130 rows, with their numpy_rule result: computed once, shared, left unchanged."""
    if (seed, max_rows, K) not in _SETS:
        c = W.random_set(seed, max_rows, K)
        _SETS[(seed, max_rows, K)] = (image(c["boxes"], c["scores"], c["classes"], c["source"]), W.numpy_rule(**c))
    return _SETS[(seed, max_rows, K)]


# ---- 1. the hand cases ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, clusters", [("joins_the_fused_box_only", [3]), ("matches_the_pivot_not_the_fused_box", [2, 1]),
                                            ("exactly_at_the_threshold", [1, 1])])
def test_hand_cases(name, clusters):
    c = W.hand_case(name)
    got, _ = check([image(c["boxes"], c["scores"], c["classes"], c["source"])], c["u"], c["thr"], 0.0, 1)
    assert got[0]["members"].tolist() == clusters


# ---- 2. empty, single and one-detector images ------------------------------------------------------------------------------------------

def test_empty_single_and_one_detector_images():
    """An image with 0 rows between two non-empty ones, an image of 1 row, an image whose rows all come from one detector (fused like
    any other: two of its rows overlap and merge, and a lone row ends at s * min(1, U) / U)."""
    a, b = random_set(0)[0], random_set(1)[0]
    empty = image(np.zeros((0, 4)), [], [], [])
    one = image([[10, 10, 50, 60]], [0.8], [2], [1])
    single = image([[10, 10, 50, 60], [11, 10, 51, 61], [200, 200, 260, 280]], [0.9, 0.7, 0.6], [1, 1, 0], [1, 1, 1])
    got, _ = check([a, empty, b, one, single], W.WEIGHTS3)
    assert got[1]["count"] == 0 and got[1]["skipped"] == 0
    U = (1.0 + 0.7) + 1.3
    assert got[3]["count"] == 1 and got[3]["scores"][0] == np.float32(((0.8 * 0.7) / 1.0 * 1.0) / U)
    assert got[4]["members"].tolist() == [2, 1] and got[4]["cluster"].tolist() == [0, 0, 1]


def test_an_image_over_the_bound_is_refused_alone():
    """counts -1, skipped 0 and nothing else for an image with more rows than max_rows; its neighbours are fused as ever."""
    small = image([[10, 10, 50, 60], [12, 10, 50, 60]], [0.8, 0.6], [0, 0], [0, 1])
    big = random_set(0)[0]
    got = run([small, big, small], [1.0, 1.0, 1.0], 0.55, 0.0, 3, max_rows=8)
    want = W.numpy_rule(small["boxes"], small["scores"], small["classes"], small["source"], [1.0, 1.0, 1.0], 0.55, 0.0, 3)
    same(got[0], want)
    same(got[2], want)
    assert got[1]["count"] == -1 and got[1]["skipped"] == 0 and (got[1]["cluster"] == -2).all()


def test_the_largest_bound_takes_the_large_lds_path():
    """max_rows at the capacity (996 rows: 160 KiB of LDS, above the 64 KiB a kernel gets unasked) gives the bits of a tight bound."""
    img, want = random_set(2)
    same(run([img], W.WEIGHTS3, 0.55, 0.0, 3, max_rows=996)[0], want)
    same(run([img], W.WEIGHTS3, 0.55, 0.0, 3, max_rows=len(img["scores"]))[0], want)


# ---- 3. lanes, ties and classes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [63, 64, 65])
def test_lane_seams(n):
    """One class with n clusters (disjoint boxes, descending scores), then a row that must join the LAST of them, then one that joins the
    first: clusters 63 and 64 are lane 63's first and lane 0's second."""
    grid = np.array([[30.0 * (i % 16), 30.0 * (i // 16), 30.0 * (i % 16) + 20, 30.0 * (i // 16) + 20] for i in range(n)])
    boxes = np.concatenate([grid, grid[-1:] + [0.5, 0, 0.5, 0], grid[:1] + [0, 0.5, 0, 0.5]])
    scores = np.concatenate([0.9 - 0.005 * np.arange(n), [0.2, 0.1]])
    got, want = check([image(boxes, scores, np.zeros(n + 2), np.arange(n + 2) % 2)], [1.0, 1.0], K=1)
    assert got[0]["count"] == n and want[0]["rows"][0] == [0, n + 1]
    assert got[0]["cluster"][n] == got[0]["cluster"][n - 1] and got[0]["cluster"][n + 1] == got[0]["cluster"][0] == 0
    assert sorted(got[0]["members"].tolist()) == [1] * (n - 2) + [2, 2]


def test_first_maximum_rule():
    """A row whose IoU with two clusters is the same double (mirror-image boxes) joins the earlier one - also when the two are 64 clusters
    apart, in one lane, and when the later one sits in a lower lane than the earlier."""
    a, b, c = [0, 0, 10, 10], [20, 0, 30, 10], [5, 0, 25, 10]
    assert W._iou(np.array([a, b], dtype=np.float64), np.array(c, dtype=np.float64), np.float64).tolist() == [0.2, 0.2]
    got, _ = check([image([a, b, c], [0.9, 0.8, 0.5], [0, 0, 0], [0, 1, 0])], [1.0, 1.0], thr=0.1, K=1)
    assert got[0]["cluster"].tolist() == [0, 1, 0]
    for first, second in ((3, 67), (10, 70), (63, 64)):
        n = 72
        boxes = np.array([[100.0 * i, 50, 100.0 * i + 10, 60] for i in range(n)])
        boxes[first], boxes[second] = [0, 0, 10, 10], [20, 0, 30, 10]
        scores = np.concatenate([0.9 - 0.005 * np.arange(n), [0.1]])
        got, want = check([image(np.concatenate([boxes, [c]]), scores, np.zeros(n + 1), np.zeros(n + 1))], [1.0], thr=0.1, K=1)
        assert want[0]["rows"][want[0]["cluster"][n]] == [first, n] and got[0]["cluster"][n] == got[0]["cluster"][first]


@pytest.mark.parametrize("K", [1, 3, 17])
def test_class_counts(K):
    """K = 1 (one wavefront works), 3, and 17: more classes than wavefronts, class 16 shares wavefront 0 with class 0."""
    imgs = [random_set(s, 130, K)[0] for s in (3, 4)]
    got = run(imgs, W.WEIGHTS3, 0.55, 0.0, K)
    for s, g in zip((3, 4), got):
        same(g, random_set(s, 130, K)[1], (K, s))
    if K == 17:
        assert {0, 16} <= set(np.concatenate([g["classes"] for g in got]).astype(int).tolist())


def test_classes_are_independent():
    box = [10, 10, 60, 70]
    got, _ = check([image([box, box, box], [0.9, 0.8, 0.7], [0, 1, 0], [0, 1, 1])], [1.0, 1.0], K=2)
    assert got[0]["count"] == 2 and got[0]["cluster"].tolist() == [0, 1, 0] and got[0]["classes"].tolist() == [0.0, 1.0]


def test_score_ties_go_by_original_index_descending():
    """Equal s inside a detector and across detectors (0.5 * 1 and 1.0 * 0.5): the LAST row is visited first.  The boxes are those of the
    second hand case, where the order of the visits decides the clusters."""
    c = W.hand_case("matches_the_pivot_not_the_fused_box")
    got, want = check([image(c["boxes"], [0.5, 0.5, 0.5], [0, 0, 0], [0, 0, 0])], [1.0, 1.0], K=1)
    assert want[0]["rows"][0][0] == 2
    got2, want2 = check([image(c["boxes"], [0.5, 1.0, 0.5], [0, 0, 0], [0, 1, 0])], [1.0, 0.5], K=1)
    assert want2[0]["rows"] == want[0]["rows"] and got2[0]["cluster"].tolist() == got[0]["cluster"].tolist()
    # conf ties in the output: class ascending, then creation order
    box = [[10, 10, 50, 50], [100, 100, 150, 150], [200, 200, 250, 250]]
    got, _ = check([image(box + box, [0.5] * 6, [2, 2, 2, 0, 0, 0], [0] * 6)], [1.0, 1.0], K=3)
    assert got[0]["classes"].tolist() == [0.0] * 3 + [2.0] * 3 and got[0]["cluster"].tolist() == [5, 4, 3, 2, 1, 0]


def test_skip_conditions():
    """s == skip is kept; one ulp below skip, a NaN score, an infinite score, a score of 0, a negative score, a NaN and an infinite
    coordinate, a bad source (-1, D) and a bad class (-1, K) each skip their row and are counted."""
    u = [1.0, 0.7]
    skip = 0.3 * 0.7
    below = np.nextafter(0.3, 0.0)
    assert below * 0.7 < skip
    far = lambda i: [100.0 * i, 0, 100.0 * i + 40, 40]  # noqa: E731
    rows = [(far(0), 0.3, 0, 1), (far(1), below, 0, 1), (far(2), np.nan, 0, 0), (far(3), np.inf, 0, 0), (far(4), 0.0, 0, 0),
            (far(5), -0.5, 0, 0), ([np.nan, 0, 40, 40], 0.9, 0, 0), ([0, 0, np.inf, 40], 0.9, 0, 0), (far(8), 0.9, 0, -1),
            (far(9), 0.9, 0, 2), (far(10), 0.9, -1, 0), (far(11), 0.9, 3, 0), (far(12), 0.9, 2, 0)]
    img = image([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    got, _ = check([img], u, skip=skip, K=3)
    assert got[0]["skipped"] == 11 and got[0]["count"] == 2 and got[0]["cluster"].tolist() == [1] + [-1] * 11 + [0]
    # every condition alone, beside a good row
    for bad in rows[1:12]:
        pair = image([bad[0], far(0)], [bad[1], 0.9], [bad[2], 0], [bad[3], 0])
        got, _ = check([pair], u, skip=skip, K=3)
        assert got[0]["skipped"] == 1 and got[0]["cluster"].tolist() == [-1, 0], bad


def test_degenerate_boxes():
    """Two zero-area boxes at one point give IoU 0 / 0: a NaN never wins, they do not merge, and the boxes stay finite.  A zero-area box
    inside a real one has IoU 0 with it."""
    pt = [5, 5, 5, 5]
    got, _ = check([image([pt, pt, [0, 0, 10, 10]], [0.9, 0.8, 0.7], [0, 0, 0], [0, 1, 0])], [1.0, 1.0], thr=0.0, K=1)
    assert got[0]["count"] == 3 and np.isfinite(got[0]["boxes"]).all() and got[0]["boxes"][:2].tolist() == [[5.0] * 4] * 2


def test_conf_rescale_with_unequal_weights():
    """D = 3, u = 1, 0.7, 1.3 (U = 3): clusters of n = 1, 2, 3 are scored down by n / U, one of n = 5 > U is not."""
    boxes, scores, source = [], [], []
    for k, n in enumerate((1, 2, 3, 5)):
        for t in range(n):
            boxes.append([100.0 * k, 0, 100.0 * k + 50, 50])
            scores.append(0.9 - 0.1 * t)
            source.append(t % 3)
    got, want = check([image(boxes, scores, np.zeros(len(scores)), source)], W.WEIGHTS3, K=1)
    by_size = {int(m): float(c) for m, c in zip(want[0]["members"], want[0]["conf"])}
    U = (1.0 + 0.7) + 1.3
    assert sorted(by_size) == [1, 2, 3, 5] and by_size[1] == ((0.9 * 1.0) / 1.0 * 1.0) / U
    s5 = [0.9 * 1.0, 0.8 * 0.7, 0.7 * 1.3, 0.6 * 1.0, 0.5 * 0.7]
    S = 0.0
    for s in sorted(s5, reverse=True):          # the visiting order
        S = S + s
    assert by_size[5] == ((S / 5.0) * U) / U
    assert sorted(got[0]["members"].tolist()) == [1, 2, 3, 5]


# ---- 4. independence of the batch and of the run ------------------------------------------------------------------------------------------

def test_random_sets_alone_in_a_batch_and_twice():
    """Eight seeded sets of 130 rows: each image alone, inside a batch of 8, and the batch twice - all equal numpy_rule's bytes."""
    seeds = range(10, 18)
    imgs = [random_set(s)[0] for s in seeds]
    first, second = run(imgs, W.WEIGHTS3, 0.55, 0.0, 3), run(imgs, W.WEIGHTS3, 0.55, 0.0, 3)
    multi = 0
    for s, img, g1, g2 in zip(seeds, imgs, first, second):
        want = random_set(s)[1]
        same(g1, want, s)
        same(g2, want, s)
        same(run([img], W.WEIGHTS3, 0.55, 0.0, 3)[0], want, s)
        multi += int((want["members"] > 1).sum())
    assert multi > 100


def test_fusion_takes_three_infos():
    """fusion(("wbf", "wbf"), info_1, info_2, info_3): one image through the reference-style call, a row's detector = its info's position."""
    from proben_amd import fusion as F
    img, _ = random_set(5)
    infos = []
    for d in range(3):
        m = img["source"] == d
        infos.append({"img_name": "x", "bbox": img["boxes"][m].tolist(), "score": img["scores"][m].tolist(), "class": img["classes"][m].tolist(),
                      "prob": np.full((int(m.sum()), 3), 0.25).tolist(), "vars": np.ones((int(m.sum()), 1)).tolist()})
    boxes, scores, classes = F.fusion(("wbf", "wbf"), *infos)
    want = W.numpy_rule(img["boxes"], img["scores"], img["classes"], img["source"], [1.0, 1.0, 1.0], 0.55, 0.0, 3)
    assert np.asarray(boxes).tobytes() == want["boxes"].tobytes() and scores.numpy().tobytes() == want["scores"].tobytes()
    assert classes.numpy().tobytes() == want["classes"].tobytes()


# ---- 5. the routes ---------------------------------------------------------------------------------------------------------------------

def test_file_route_equals_device_route():
    """late_fusion on two hand-made prediction dicts against fuse_detections on the same rows as padded detector dicts (no detector is
    run): equal bytes on images where both detectors fired, where one fired (fused on both routes: two of its rows merge) and where none
    did.  The device route's second call - the weights are uploaded at the first - runs with torch's synchronisation check set to
    "error": it makes no host synchronisation."""
    from proben_amd import fusion as F
    from proben_amd.late_fusion import late_fusion
    from proben_amd.options import FusionOptions
    rng = np.random.default_rng(7)
    B, Dn, K = 4, 12, 3
    fired = [[True, True], [True, False], [False, True], [False, False]]
    dets, j1 = [], []
    for d in range(2):
        cnt = np.array([8 if f[d] else 0 for f in fired], np.int32)
        anchor = rng.integers(0, 5, (B, Dn))
        box = np.stack([40.0 * anchor, 40.0 * anchor, 40.0 * anchor + 30, 40.0 * anchor + 30], 2) + rng.uniform(-1.5, 1.5, (B, Dn, 4))
        cls = (anchor % K).astype(np.int32)
        arrs = {"boxes": box.astype(np.float32), "scores": rng.uniform(0.3, 1, (B, Dn)).astype(np.float32), "classes": cls,
                "prob_score": rng.dirichlet(np.ones(K + 1), (B, Dn))[:, :, :K].astype(np.float32),
                "class_logits": rng.normal(0, 3, (B, Dn, K + 1)).astype(np.float32), "vars": rng.uniform(0.5, 2, (B, Dn)).astype(np.float32),
                "counts": cnt}
        dets.append({k: dev(v) for k, v in arrs.items()})
        rec = {k: [] for k in ("image", "boxes", "scores", "classes", "image_id", "class_logits", "probs", "vars")}
        for b in range(B):
            n = int(cnt[b])
            rec["image"].append(f"f{b}.jpeg")
            rec["image_id"].append(b)
            for key, s in (("boxes", "boxes"), ("scores", "scores"), ("classes", "classes"), ("class_logits", "class_logits"), ("probs", "prob_score")):
                rec[key].append(arrs[s][b, :n].tolist())
            rec["vars"].append([[float(v)] for v in arrs["vars"][b, :n]])
        j1.append(json.loads(json.dumps(rec)))
    opts = FusionOptions("wbf", "wbf", num_detectors=2, wbf_weights=[1.0, 0.7], wbf_skip=0.25)
    stats = {}
    via = late_fusion(j1, ["wbf", "wbf"], options=opts, stats=stats)
    F.fuse_detections(dets, options=opts)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = F.fuse_detections(dets, options=opts)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert "keep" not in out and out["stride"] == 2 * Dn
    S = out["stride"]
    cnt = out["counts"].cpu().numpy()
    host = {k: out[k].cpu().numpy() for k in ("boxes", "scores", "classes", "members")}
    assert stats["skipped"] == int(out["skipped"].sum()) > 0
    for b in range(B):
        if via[b] is None:
            assert cnt[b] == 0 and fired[b] == [False, False]
            continue
        sl = slice(b * S, b * S + cnt[b])
        assert len(via[b]) == 3 and len(via[b][1]) == cnt[b] > 0
        for k, got in zip(("boxes", "scores", "classes"), via[b]):
            got = got.numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
            assert got.dtype == host[k].dtype and got.tobytes() == host[k][sl].tobytes(), (b, k)
        if sum(fired[b]) == 1:
            assert host["members"][sl].max() >= 2          # an image one detector fired on is fused, not passed through


def test_demo_writes_a_prediction_file_the_bootstrap_reads(tmp_path, capsys):
    """demo_probEn --score_fusion wbf --box_fusion wbf --write_fused on hand-written prediction files over a tiny dataset: the file reads
    back through read_j1 with class_logits [], probs [], vars [1.0], the run says how many rows it skipped, names its weights, and
    bootstrap_ap accepts the file beside a detector's."""
    from fuse_inputs import dependent_files
    from proben_amd.cli import bootstrap_ap, demo_probEn
    from proben_amd.late_fusion import read_j1
    root, files, preds, _ = dependent_files(tmp_path, n_img=6)
    fused = tmp_path / "pred" / "val_wbf_predictions.json"
    res = demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(tmp_path / "pred"), "--detectors", "thermal_only,early_fusion",
                            "--outfolder", str(tmp_path / "o"), "--dataset_name", "flir_wbf", "--score_fusion", "wbf", "--box_fusion", "wbf",
                            "--wbf_weights", "thermal_only=1,early_fusion=0.7", "--wbf_skip", "0.3", "--write_fused", str(fused)])
    printed = capsys.readouterr().out
    assert f"fused detections: {fused}" in printed and "rows on 6 images written" in printed and "rows skipped" in printed
    assert "background rows dropped" not in printed
    assert res["wbf_weights"] == {"thermal_only": 1.0, "early_fusion": 0.7} and res["wbf_skip"] == 0.3 and res["wbf_iou"] == 0.55 and "bbox" in res
    d = read_j1(str(fused))
    assert d["image_id"] == preds[1]["image_id"] and d["image"] == preds[1]["image"]
    rows = sum(len(r) for r in d["scores"])
    skipped = int(printed.split("rows on 6 images written, ")[1].split(" rows skipped")[0])
    kept = sum(1 for p, w in zip(preds, (1.0, 0.7)) for img in p["scores"] for s in img if not s * w < 0.3)
    assert rows > 0 and skipped == sum(len(i) for p in preds for i in p["scores"]) - kept > 0
    for i in range(6):
        n = len(d["scores"][i])
        assert d["class_logits"][i] == [[]] * n and d["probs"][i] == [[]] * n and d["vars"][i] == [[1.0]] * n
        assert len(d["boxes"][i]) == n and all(len(b) == 4 for b in d["boxes"][i]) and d["scores"][i] == sorted(d["scores"][i], reverse=True)
    rep = bootstrap_ap.main(["--dataset_path", str(root), "--predictions", files[0], str(fused), "--replicates", "30"])
    assert "paired" in rep and rep["replicates"] == 30
    assert 0 <= rep["b"]["stats"]["AP"]["lo"] <= rep["b"]["stats"]["AP"]["point"] <= rep["b"]["stats"]["AP"]["hi"] <= 1


def test_one_pass_equals_the_two_stage_route(tmp_path, capsys):
    """demo_probEn --one-pass with wbf (FramePairPipeline -> fuse_detections) writes the file the two-stage route writes from the
    prediction files the same run wrote."""
    from fuse_inputs import weights, write_flir
    from proben_amd.cli import demo_probEn
    root = tmp_path / "val"
    write_flir(root, 4, 96, 120, (150, 180))
    names = ["thermal_only", "early_fusion"]
    paths = [weights(tmp_path, m, s) for s, m in enumerate(names, 1)]
    pdir = tmp_path / "pred"
    f1, f2 = tmp_path / "one.json", tmp_path / "two.json"
    wbf = ["--score_fusion", "wbf", "--box_fusion", "wbf", "--wbf_weights", "1,0.7", "--wbf_iou", "0.5"]
    r1 = demo_probEn.main(["--one-pass", "--dataset_path", str(root), "--detectors", ",".join(names), "--model_paths", ",".join(paths), "--workers",
                           "0", "--batch", "4", "--outfolder", str(tmp_path / "o1"), "--dataset_name", "flir_wbf1", "--write-predictions",
                           "--prediction_path", str(pdir), "--write_fused", str(f1)] + wbf)
    r2 = demo_probEn.main(["--dataset_path", str(root), "--prediction_path", str(pdir), "--detectors", ",".join(names), "--outfolder",
                           str(tmp_path / "o2"), "--dataset_name", "flir_wbf2", "--write_fused", str(f2)] + wbf)
    printed = capsys.readouterr().out
    assert printed.count("rows skipped") == 2
    assert f1.read_bytes() == f2.read_bytes() and sum(len(r) for r in json.load(open(f1))["scores"]) > 0
    assert r1["wbf_iou"] == r2["wbf_iou"] == 0.5 and r1["wbf_weights"] == r2["wbf_weights"]
