"""The cost record of weighted boxes fusion: writes profiles/wbf.txt.

The bench's fusion shape - 32 images, two detectors' padded rows (100 per detector and image, 60-100 live, half of them on shared
ground truth, K = 3: the step of scripts/presence_probe.py) - packed once by pe_proben_pack_pooled; then, on the same rows,
pe_wbf_fuse_batch and beside it pe_proben_fuse_batch ("probEn", "v-avg") as the yardstick, each called through the C-ABI with its
outputs allocated beforehand (nothing but the entry point's one kernel inside the timed window): device events around every launch,
the median of 10 launches after 5 warm-up launches, and the mean over a window of 200 back-to-back launches.  A third timing runs
pe_wbf_fuse_batch on the same rows with every class set to 0, so that one wavefront walks all of an image's rows: the difference
over the difference of the longest walks is what a row of the serial walk costs.  The NumPy restatement (tests/wbf_ref.numpy_rule)
runs on the host over the same rows: its time, and whether the kernel's bytes equal it.

    python scripts/wbf_probe.py [--out profiles/wbf.txt]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import proben_amd  # noqa: E402,F401
from proben_amd import fusion as F  # noqa: E402
from proben_amd.options import FusionOptions  # noqa: E402
import wbf_ref  # noqa: E402

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "wbf.txt")
B, D, K, G = 32, 100, 3, 12
rng = np.random.default_rng(3)
x1 = rng.uniform(0, 520, (B, G)); y1 = rng.uniform(0, 400, (B, G))
gt = np.stack([x1, y1, x1 + rng.uniform(20, 120, (B, G)), y1 + rng.uniform(20, 100, (B, G))], 2)
dets = []
for d in range(2):
    cnt = rng.integers(60, 101, B).astype(np.int32)
    x1 = rng.uniform(0, 520, (B, D)); y1 = rng.uniform(0, 400, (B, D))
    bx = np.stack([x1, y1, x1 + rng.uniform(20, 120, (B, D)), y1 + rng.uniform(20, 100, (B, D))], 2)
    bx[:, :48] = np.tile(gt, (1, 4, 1)) + rng.normal(0, 2, (B, 48, 4))          # half of the rows sit on ground truth (and on each other)
    lg = rng.normal(0, 3, (B, D, K + 1)).astype(np.float32)
    cls = lg[:, :, :K].argmax(2).astype(np.int32)
    if d == 1:
        cls[:, :48] = dets[0]["classes"].cpu().numpy()[:, :48]
    e = np.exp(lg - lg.max(2, keepdims=True)); p = (e / e.sum(2, keepdims=True)).astype(np.float32)
    dets.append({"boxes": torch.from_numpy(bx.astype(np.float32)).cuda(),
                 "scores": torch.from_numpy(np.take_along_axis(p, cls[..., None].astype(np.int64), 2)[..., 0].copy()).cuda(),
                 "classes": torch.from_numpy(cls).cuda(), "prob_score": torch.from_numpy(p[:, :, :K].copy()).cuda(),
                 "class_logits": torch.from_numpy(lg).cuda(), "vars": torch.from_numpy((10.0 ** rng.uniform(-3, -1, (B, D))).astype(np.float32)).cuda(),
                 "counts": torch.from_numpy(cnt).cuda()})
S = 2 * D
opts = FusionOptions("wbf", "wbf", num_detectors=2)
ob, os_, op, ov, oc, ooff, ocnt, osingle, osrc = F.pack_rows(dets, 2, options=opts)
one_class = torch.zeros_like(oc)          # the same rows as ONE class: a single wavefront walks all of an image's rows


def wbf_out():
    return F.fuse_batch(ob, os_, op, ov, oc, ooff, max_rows=S, row_counts=ocnt, row_source=osrc, options=opts)


def proben_out():
    return F.fuse_batch(ob, os_, op, ov, oc, ooff, "probEn", "v-avg", max_rows=S, row_counts=ocnt, passthrough=osingle)


P, L = proben_amd._lib.ptr, proben_amd._lib.lib()
w_out, p_out = wbf_out(), proben_out()
weights = opts.wbf_on("cuda")


def wbf(classes=oc):          # the entry point alone: outputs allocated once, no fill kernels inside the timed window
    st = L.pe_wbf_fuse_batch(P(ob), P(os_), P(classes), P(osrc), P(ooff), P(ocnt), B, K, S, P(weights), 2, F.WBF_IOU, 0.0, P(w_out["boxes"]),
                             P(w_out["scores"]), P(w_out["classes"]), P(w_out["counts"]), P(w_out["cluster"]), P(w_out["members"]),
                             P(w_out["skipped"]), proben_amd._lib.stream())
    assert st == 0, L.pe_last_error()


def proben():
    st = L.pe_proben_fuse_batch(P(ob), P(os_), P(op), P(ov), P(oc), P(ooff), P(ocnt), P(osingle), B, K, S, F.SCORE_MODES["probEn"],
                                F.BOX_MODES["v-avg"], 0.5, F.FRAME_W, F.FRAME_H, P(p_out["boxes"]), P(p_out["scores"]), P(p_out["classes"]),
                                P(p_out["keep"]), P(p_out["counts"]), proben_amd._lib.stream())
    assert st == 0, L.pe_last_error()


def timed(call):
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    single = []
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record()
        torch.cuda.synchronize()
        single.append(a.elapsed_time(b) * 1e3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        call()
    b.record()
    torch.cuda.synchronize()
    return sorted(single), a.elapsed_time(b) * 1e3 / 200


w_single, w_window = timed(wbf)
p_single, p_window = timed(proben)
o_single, o_window = timed(lambda: wbf(one_class))
wbf()           # the outputs compared below are those of the rows' own classes
torch.cuda.synchronize()
host = {k: v.cpu().numpy() for k, v in w_out.items()}
rows = {k: v.cpu().numpy() for k, v in (("boxes", ob), ("scores", os_), ("classes", oc), ("source", osrc), ("counts", ocnt))}
t0 = time.perf_counter()
want = []
for b in range(B):
    sl = slice(b * S, b * S + int(rows["counts"][b]))
    want.append(wbf_ref.numpy_rule(rows["boxes"][sl], rows["scores"][sl], rows["classes"][sl], rows["source"][sl], [1.0, 1.0], F.WBF_IOU, 0.0, K))
numpy_s = time.perf_counter() - t0
equal = all(host["counts"][b] == w["count"] and host["boxes"][b * S:b * S + w["count"]].tobytes() == w["boxes"].tobytes() and
            host["scores"][b * S:b * S + w["count"]].tobytes() == w["scores"].tobytes() and
            host["cluster"][b * S:b * S + int(rows["counts"][b])].tolist() == w["cluster"].tolist() for b, w in enumerate(want))
per_class = [int(max(np.bincount(rows["classes"][b * S:b * S + int(rows["counts"][b])], minlength=K))) for b in range(B)]
lines = [
    "weighted boxes fusion: the cost record (scripts/wbf_probe.py; every time below is MEASURED on " + torch.cuda.get_device_name(0) + ")",
    f"shape: {B} images, 2 detectors x {D} padded rows, {int(rows['counts'].sum())} live rows ({int(rows['counts'].min())}-{int(rows['counts'].max())} per image), K = {K}, "
    f"max_rows {S}, thr {F.WBF_IOU}, weights 1, 1",
    f"the longest serial walk: {max(per_class)} rows of one class in one image (mean of the per-image maxima {np.mean(per_class):.1f})",
    f"fused rows: wbf {int(host['counts'].sum())} clusters ({int((host['members'] > 1).sum())} of two or more rows, largest {int(host['members'].max())}), "
    f"skipped {int(host['skipped'].sum())}; probEn v-avg {int(p_out['counts'].sum())} clusters",
    "",
    "per launch, device events, 10 launches after 5 warm-up launches (us, sorted):",
    f"  pe_wbf_fuse_batch     median {np.median(w_single):8.1f}   " + " ".join(f"{x:.1f}" for x in w_single),
    f"  pe_proben_fuse_batch  median {np.median(p_single):8.1f}   " + " ".join(f"{x:.1f}" for x in p_single),
    f"  pe_wbf_fuse_batch, the same rows as ONE class (the walk is {int(rows['counts'].max())} rows on one wavefront)",
    f"                        median {np.median(o_single):8.1f}   " + " ".join(f"{x:.1f}" for x in o_single),
    f"  the walk's slope: ({np.median(o_single):.1f} - {np.median(w_single):.1f}) us / ({int(rows['counts'].max())} - {max(per_class)}) rows = "
    f"{(np.median(o_single) - np.median(w_single)) / (int(rows['counts'].max()) - max(per_class)):.2f} us per row of the longest walk",
    "mean per launch over a window of 200 back-to-back launches (us; includes the host's enqueue where it is the slower side):",
    f"  pe_wbf_fuse_batch     {w_window:8.1f}",
    f"  pe_proben_fuse_batch  {p_window:8.1f}",
    f"  pe_wbf_fuse_batch, ONE class  {o_window:8.1f}",
    f"tests/wbf_ref.numpy_rule on the host, the same {B} images: {numpy_s * 1e3:.1f} ms",
    f"kernel output equals numpy_rule bit for bit (counts, boxes, scores, cluster): {equal}",
]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
assert equal
