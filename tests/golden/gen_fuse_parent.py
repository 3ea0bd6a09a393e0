"""Generate tests/golden/fuse_parent.npz: what fusion.fuse_batch returned for a set of small batches, recorded on the GPU at the commit
BEFORE csrc/proben.hip's rules, LDS layout and argument table were each stated once (DESIGN.md section 24 names it).
tests/test_fuse_golden_gpu.py holds the same calls to these bits.

    python tests/golden/gen_fuse_parent.py [--out PATH]       on the GPU, at that commit
    python tests/golden/gen_fuse_parent.py --check-inputs     anywhere: the coverage conditions below on the host alone

Only fusion.fuse_batch is used and the file holds OUTPUTS ONLY.  The inputs are closed-form integer formulas (multipliers modulo the
prime 8191, scaled; no logarithm or exponential, so every machine builds the same bits) that the test rebuilds by importing this file:
no random generator is involved.

The batch (SIZES): eight images of 0, 1, 2, 63, 64, 65, 131 and 9 rows - the 64-row word seams of the bit matrices, and 131 = 4 * 32 + 3,
a tail of the walk's four-row unroll that is neither empty nor full.  Rows come in groups of 1, 2, 3 and 5 near-duplicate boxes (one grid
cell per group, jittered by under 3 pixels, so a group clusters at IoU > 0.5 and two groups never touch), the groups spread over three
classes, scores / probabilities / log-posteriors / variances from modular formulas, detectors alternating inside a group.  The 131-row
image also holds (SPECIAL): two exactly tied scores inside a cluster, a NaN score, a NaN coordinate (that row leaves the pool without
matching), a pair whose IoU is exactly the threshold (30-wide boxes 10 apart: 400 / 800), a saturated row (p = 1, log-posterior 0 / -inf:
"probEn" takes log 0), a row whose source is outside [0, D) (poisons its cluster in the pooled and the presence forms) and a group of
three whose summation order shows in the float32 score ("cancel": in cluster order an ordinary row, a row with log-posterior 2^44 in
column 0, a row with -2^44 there, the last two of one detector, so that the ordinary entry is rounded to 2^-8 in this order and kept
exactly in the reversed one).

Runs.  A mode case is (score_fusion, box_fusion, pool, post, pres, prior, D):
  plain   "probEn", "avg", "max" (K = 3) and "probEn_binary" (K = 1) x the four box modes, less ("max", "argmax")
  LOGP    the eight combinations of pool_weights / with_posterior / presence, each with and without a class prior, at "v-avg" and at one
          of "s-avg" / "avg" / "argmax" in rotation; D = 2 or 3 detectors, weights neither 1 nor equal, a presence table with a distinct
          entry per pattern and column; presence without with_posterior is the score-only run
Every mode case runs four times: with row_counts + passthrough (the pipeline's form; the 9-row image is flagged) and with plain offsets,
each at max_rows = 132 (bit-matrix form) and 1024 (sequential form).  One plain and one full (pool + post + pres) case also run at the two
even max_rows either side of the form switch, computed by form_switch() from the parent's per-row formula (restated here as frozen
text), and the full case once on a single image of max_rows + 1 rows: count -1, its rows untouched.

The file.  Per run, image and field: counts; the live rows [offsets[b], offsets[b] + counts[b]) of boxes, scores, classes, keep, vars and
members; the image's whole slice of the prefilled arrays cluster, log_posterior and pattern (their untouched elements are the prefill).
Most of these byte strings repeat - the two clustering forms give the same bits, seven images do not depend on the batch form, the boxes
not on the score rule -, so the file keeps each distinct string once: `blob` (all strings back to back), `ends` (where each stops) and
`index` i32 [run, image, field] (which string, -1 = the run has no such output), with `runs` and `fields` naming the axes.

Coverage conditions, asserted on the host before anything is written (and alone by --check-inputs; the clustering restated here must
give oracle/proben.py's keep lists):
  * the batch holds clusters of exactly 1, exactly 2 and at least 3 rows (every mode case runs the same rows);
  * in the 131-row image a cluster spans a 64-row word seam of the sorted order;
  * per mode case at most a quarter of the fused rows have a NaN score (oracle.proben's score rules for the plain cases, the
    log-posterior rule restated below for the others); the recorded scores are held to the same bound;
  * per LOGP case at least one cluster's fused score, as the float32 the file stores, differs in bits from the score with the members
    summed in reversed order: otherwise the file could not tell one summation order from another.
"""
import functools
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

P = 8191
K = 3
FRAME = (640.0, 512.0)
THR = 0.5
SIZES = (0, 1, 2, 63, 64, 65, 131, 9)
BIG, PASS = 6, 7                        # the image with the special rows; the image flagged passthrough in the row_counts form
TIGHT, WIDE = 132, 1024                 # max_rows of the bit-matrix and of the sequential form
SPECIAL = {"tie": (3, 4), "nan_score": 7, "nan_coord": 18, "threshold": (12, 13), "saturated": 15, "bad_source": 26, "cancel": (36, 37, 38)}
CANCEL = 2.0 ** 44
WEIGHTS = {2: [0.75, 1.5], 3: [0.75, 1.5, 1.25]}
LOG_PRIOR = [-1.25, -1.5, -0.75, -2.0]
BOXES = ("v-avg", "s-avg", "avg", "argmax")
FIELDS = ("counts", "boxes", "scores", "classes", "keep", "vars", "members", "cluster", "log_posterior", "pattern")
WHOLE = ("cluster", "log_posterior", "pattern")

PLAIN = [(s, b, 0, 0, 0, 0, 2) for s in ("probEn", "avg", "max", "probEn_binary") for b in BOXES if (s, b) != ("max", "argmax")]
LOGP = [("probEn-log", b, pool, post, pres, prior, 2 + (pool + post + pres + prior) % 2)
        for i, (pool, post, pres, prior) in enumerate(itertools.product((0, 1), repeat=4)) for b in ("v-avg", BOXES[1 + i % 3])]
FULL = ("probEn-log", "v-avg", 1, 1, 1, 1, 3)


def form_switch(L, pool, pres):
    """The largest even max_rows that takes the bit-matrix form, from the parent's formula (frozen text): per row
    8 * (6 + L + 5 + pool) + 4 + 4 + 4 * pres + 4 * 2 + 1 bytes, 16 bytes of slack, 16 bytes per row and 64-row word for the two
    matrices, 512 bytes of static LDS, 160 KiB in all."""
    per_row = 8 * (6 + L + 5 + pool) + 4 + 4 + 4 * pres + 4 * 2 + 1
    fits = [R for R in range(2, 2049, 2) if R * per_row + 16 + R * ((R + 63) // 64) * 16 + 512 <= 160 * 1024]
    return fits[-1]


def runs():
    """(mode case, batch form, max_rows): batch form "counts" (row_counts + passthrough), "offsets" or "over" (one image too long)."""
    out = [(c, form, R) for c in PLAIN + LOGP for form in ("counts", "offsets") for R in (TIGHT, WIDE)]
    for c in (PLAIN[0], FULL):
        last = form_switch(K + 1, c[2], c[4])
        out += [(c, "counts", last), (c, "counts", last + 2)]
    return out + [(FULL, "over", 8)]


def run_name(run):
    (s, b, pool, post, pres, prior, D), form, R = run
    return f"{s}_{b}_{pool}{post}{pres}{prior}_d{D}_{form}_{R}"


def frac(i, a=1, c=0):
    """((a * i + c) mod P) / P in [0, 1): exact integer arithmetic, one float64 division."""
    return ((np.asarray(i, np.int64) * a + c) % P) / P


@functools.lru_cache(None)
def image_rows(b, n):
    """Image b's n rows: boxes f64 [n, 4], scores, probs [n, K], log_probs [n, K + 1], vars, classes i32, and the group / place in its
    group of each row (a row's detector is (group + place) mod D)."""
    sizes = list(itertools.islice(itertools.cycle((1, 2, 3, 5)), n))
    g = np.repeat(np.arange(len(sizes)), sizes)[:n].astype(np.int64)
    place = np.concatenate([np.arange(s) for s in sizes] + [np.zeros(0, int)])[:n].astype(np.int64)
    r = np.arange(n, dtype=np.int64)
    x1 = 4.0 + 48.0 * (g % 13) + 3.0 * frac(r * 613 + b * 29, 1, 7)
    y1 = 4.0 + 40.0 * ((g // 13) % 12) + 3.0 * frac(r * 1277 + b * 31, 1, 2)
    boxes = np.stack([x1, y1, x1 + 36.0 + 2.0 * frac(r * 389 + b, 1, 3), y1 + 30.0 + 2.0 * frac(r * 997 + b, 1, 5)], 1)
    scores = 0.30 + 0.65 * frac(r * 2731 + b * 97, 1, 11)
    j = np.arange(K + 1, dtype=np.int64)[None]
    probs = 0.01 + 0.3 * frac(r[:, None] * 389 + j[:, :K] * 1277 + r[:, None] * j[:, :K] * 31 + b, 1, 5)
    log_probs = -(0.05 + 6.0 * frac(r[:, None] * 613 + j * 2731 + r[:, None] * j * 29 + b * 53, 1, 17))
    variances = 0.5 + 2.5 * frac(r * 1543 + b, 1, 3)
    classes = (g % 3).astype(np.int32)
    if b == BIG:
        S = SPECIAL
        scores[S["tie"][1]] = scores[S["tie"][0]]
        scores[S["nan_score"]] = np.nan
        boxes[S["nan_coord"], 0], scores[S["nan_coord"]] = np.nan, 0.05          # the lowest score: it is never a pivot
        boxes[S["threshold"][0]], boxes[S["threshold"][1]] = [250.0, 5.0, 279.0, 24.0], [260.0, 5.0, 289.0, 24.0]
        probs[S["saturated"]] = [1.0, 0.0, 0.0]
        log_probs[S["saturated"]] = [0.0] + [-np.inf] * K
        x, up, down = S["cancel"]             # cluster order (matches by score, the pivot last): x, up, down
        scores[x], scores[up], scores[down] = 0.98, 0.97, 0.99
        log_probs[up, 0], log_probs[down, 0] = CANCEL, -CANCEL
    return boxes, scores, probs, log_probs, variances, classes, g, place


def sources(b, n, D):
    g, place = image_rows(b, n)[6:]
    src = ((g + place) % D).astype(np.int32)
    if b == BIG:
        src[SPECIAL["bad_source"]] = D
        src[list(SPECIAL["cancel"][1:])] = 0            # one detector, one pool weight: the two large entries cancel exactly
    return src


def presence_table(D):
    pat, col = np.arange(1 << D)[:, None], np.arange(K + 1)[None]
    return -(0.125 + 0.0625 * (pat * (K + 1) + col))


def batch(form, max_rows):
    return [(BIG - 1, max_rows + 1)] if form == "over" else list(enumerate(SIZES))


# ---- the host's restatement, for the coverage conditions only --------------------------------------------------------------------

def clusters(b, n):
    """The greedy clustering of oracle.proben.nms_bayesian, keeping the membership: [(pivot's sorted position, member sorted positions in
    cluster order - matches ascending, the pivot last)] and the sorted order itself."""
    from oracle.proben import order_desc
    boxes, scores, _, _, _, classes = image_rows(b, n)[:6]
    c = classes.astype(np.float64)
    x1, y1, x2, y2 = (boxes[:, e] + c * FRAME[e % 2] for e in range(4))
    area = (x2 - x1 + 1.0) * (y2 - y1 + 1.0)
    order = order_desc(scores)
    alive = np.ones(n, bool)
    out = []
    for pos in range(n):
        if not alive[pos]:
            continue
        alive[pos] = False
        rest = np.flatnonzero(alive)
        rest = rest[rest > pos]
        i, q = order[pos], order[rest]
        w = np.maximum(0.0, np.minimum(x2[i], x2[q]) - np.maximum(x1[i], x1[q]) + 1.0)
        h = np.maximum(0.0, np.minimum(y2[i], y2[q]) - np.maximum(y1[i], y1[q]) + 1.0)
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (area[i] + area[q] - inter)
            alive[rest[~(ovr <= THR)]] = False
            out.append((pos, list(rest[ovr > THR]) + [pos]))
    return out, order


def logp_score(lp, w, log_prior, prow):
    """The log-posterior rule's fused score (float64) of one cluster: lp [m, K + 1] in cluster order, w [m] pool weights or None,
    log_prior or None, prow the presence row or None; a NaN w poisons."""
    acc = np.zeros(K + 1)
    for t in range(len(lp)):
        acc = acc + (lp[t] if w is None else w[t] * lp[t])
    if log_prior is not None:
        W = float(len(lp))
        if w is not None:
            W = 0.0
            for t in range(len(lp)):
                W += w[t]
        acc = acc - (W - 1.0) * np.asarray(log_prior)
    if prow is not None:
        acc = acc + prow
    with np.errstate(invalid="ignore"):
        e = np.exp(acc - np.max(acc))
        tot = 0.0
        for v in e:
            tot += v
        return float(np.max(e / tot))


def host_scores(case):
    """Per cluster of the batch (the row_counts form's passthrough image left out): (rows in the cluster, fused score, the score with the
    members reversed or None, image, the pivot's row).  Plain cases: oracle.proben's score rule."""
    from oracle import proben as O
    s, _, pool, post, pres, prior, D = case
    out = []
    for b, n in enumerate(SIZES[:PASS]):
        boxes, scores, probs, log_probs, variances, classes = image_rows(b, n)[:6]
        cl, order = clusters(b, n)
        if n == 0:
            continue
        if s != "probEn-log":
            pr = probs[:, :1] if s == "probEn_binary" else probs
            keep, fused = O.nms_bayesian(boxes, scores, classes, pr, variances, THR, s, "avg", *FRAME)[:2]
            assert list(keep) == [int(order[p]) for p, _ in cl], (b, n)
            out += [(len(m), float(v), None, b, int(order[p])) for (p, m), v in zip(cl, fused)]
            continue
        src = sources(b, n, D)
        ok = (src >= 0) & (src < D)
        w_row = np.where(ok, np.asarray(WEIGHTS[D])[np.clip(src, 0, D - 1)], np.nan)
        table = presence_table(D)
        for pos, mem in cl:
            rows = order[mem]
            if len(mem) == 1 and not pres:
                out.append((1, float(scores[rows[0]]), None, b, int(order[pos])))
                continue
            prow = None
            if pres:
                pat = int(np.bitwise_or.reduce(np.where(ok[rows], 1 << np.clip(src[rows], 0, D - 1), 0)))
                prow = table[pat] if ok[rows].all() else np.full(K + 1, np.nan)
            lone = len(mem) == 1            # a lone row under presence: no weight, no prior
            args = (None if lone or not pool else w_row, None if lone or not prior else LOG_PRIOR)
            fwd = logp_score(log_probs[rows], None if args[0] is None else args[0][rows], args[1], prow)
            rev = logp_score(log_probs[rows[::-1]], None if args[0] is None else args[0][rows[::-1]], args[1], prow)
            out.append((len(mem), fwd, rev, b, int(order[pos])))
    return out


def check_inputs(say=print):
    from oracle import proben as O
    for b, n in enumerate(SIZES):           # the clustering restated above is the oracle's
        if n == 0:
            continue
        boxes, scores, probs, _, variances, classes = image_rows(b, n)[:6]
        keep = O.nms_bayesian(boxes, scores, classes, probs, variances, THR, "avg", "avg", *FRAME)[0]
        cl, order = clusters(b, n)
        assert list(keep) == [int(order[p]) for p, _ in cl], (b, n)
    sizes = [len(m) for b, n in enumerate(SIZES[:PASS]) for _, m in clusters(b, n)[0]]
    assert 1 in sizes and 2 in sizes and max(sizes) >= 3, sizes
    cl, order = clusters(BIG, SIZES[BIG])
    seam = [(p, m) for p, m in cl if len({q >> 6 for q in m}) > 1]
    assert seam, "no cluster spans a 64-row word seam"
    where = {int(order[p]): len(m) for p, m in cl}
    S = SPECIAL
    assert where.get(S["threshold"][0]) == 1 and where.get(S["threshold"][1]) == 1, "the exact-threshold pair must not match"
    assert S["nan_coord"] not in where and not any(list(order).index(S["nan_coord"]) in m for _, m in cl), "the NaN coordinate row matched"
    assert any(len(m) >= 2 and {list(order).index(r) for r in S["tie"]} <= set(m) for _, m in cl), "the tied scores share no cluster"
    say(f"clusters of the batch: {len(sizes)} ({sizes.count(1)} of one row, {sizes.count(2)} of two, {sum(s >= 3 for s in sizes)} of three or "
        f"more); {len(seam)} span a word seam; form switch at max_rows {form_switch(K + 1, 0, 0)} (plain) / {form_switch(K + 1, 1, 1)} (full)")
    for case in PLAIN + LOGP:
        got = host_scores(case)
        nan = sum(c[1] != c[1] for c in got)
        assert 4 * nan <= len(got), (case, nan, len(got))
        if case[0] == "probEn-log":
            told = sum(rev is not None and np.float32(v).tobytes() != np.float32(rev).tobytes() for _, v, rev, _, _ in got)
            assert told >= 1, (case, "no fused score tells the summation order")
            say(f"{case}: {len(got)} fused rows, {nan} NaN, {told} float32 scores change with the member order")
        else:
            say(f"{case}: {len(got)} fused rows, {nan} NaN")


# ---- the device side -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(None)
def device_batch(form, max_rows, D, binary):
    import torch
    imgs = batch(form, max_rows)
    rows = [image_rows(b, n) for b, n in imgs]
    cat = [np.concatenate([r[e] for r in rows]) for e in range(6)]
    if binary:
        cat[2] = cat[2][:, :1]
    offs = np.concatenate([[0], np.cumsum([n for _, n in imgs])]).astype(np.int32)
    src = np.concatenate([sources(b, n, D) for b, n in imgs])
    flags = np.asarray([int(form == "counts" and i == PASS) for i in range(len(imgs))], np.int32)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in cat + [offs, src, flags]]
    return dev, offs


def run_case(run):
    """fuse_batch for one run -> {field: [one array per image]}, the slices the file holds."""
    import torch
    from proben_amd import fusion as F
    (s, box, pool, post, pres, prior, D), form, max_rows = run
    (boxes, scores, probs, log_probs, variances, classes, offsets, src, flags), offs = device_batch(form, max_rows, D, s == "probEn_binary")
    kw = dict(score_fusion=s, box_fusion=box, max_rows=max_rows, iou_thresh=THR, frame=FRAME)
    if form == "counts":
        kw.update(row_counts=(offsets[1:] - offsets[:-1]).contiguous(), passthrough=flags)
        offsets = offsets[:-1].contiguous()
    if s == "probEn-log":
        kw.update(log_probs=log_probs, with_posterior=bool(post))
        if prior:
            kw["class_prior"] = torch.tensor(LOG_PRIOR, dtype=torch.float64).cuda()         # a device tensor is the log-prior itself
        if pool:
            kw["pool_weights"] = WEIGHTS[D]
        if pres:
            kw["presence"] = torch.from_numpy(presence_table(D)).cuda()
        if pool or pres:
            kw["row_source"] = src
    out = F.fuse_batch(boxes, scores, probs, variances, classes, offsets, **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    res = {f: [] for f in FIELDS if f in out}
    for i in range(len(offs) - 1):
        lo, hi, cnt = int(offs[i]), int(offs[i + 1]), int(out["counts"][i])
        assert -1 <= cnt <= hi - lo, (run_name(run), i, cnt)
        for f in res:
            res[f].append(out[f][i:i + 1] if f == "counts" else out[f][lo:hi] if f in WHOLE else out[f][lo:lo + max(cnt, 0)])
    return res


def main():
    if "--check-inputs" in sys.argv:
        check_inputs()
        return
    import proben_amd  # noqa: F401
    check_inputs(say=lambda *_: None)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "fuse_parent.npz")
    all_runs = runs()
    blobs, index = {}, np.full((len(all_runs), len(SIZES), len(FIELDS)), -1, np.int32)
    for r, run in enumerate(all_runs):
        res = run_case(run)
        fused = np.concatenate(res["scores"])
        counts = np.concatenate(res["counts"])
        assert 4 * int(np.isnan(fused).sum()) <= len(fused), (run_name(run), int(np.isnan(fused).sum()), len(fused))
        assert (counts == -1).all() if run[1] == "over" else (counts >= 0).all(), (run_name(run), counts)
        for f, per_image in res.items():
            for i, a in enumerate(per_image):
                index[r, i, FIELDS.index(f)] = blobs.setdefault(np.ascontiguousarray(a).tobytes(), len(blobs))
        print(f"{run_name(run):44s} counts {counts.tolist()}", flush=True)
    order = sorted(blobs, key=blobs.get)
    z = {"blob": np.frombuffer(b"".join(order), np.uint8), "ends": np.cumsum([len(x) for x in order]).astype(np.int64), "index": index,
         "runs": np.asarray([run_name(r) for r in all_runs]), "fields": np.asarray(FIELDS)}
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes,", len(all_runs), "runs,", len(order), "distinct byte strings,", len(z["blob"]), "bytes of them")


if __name__ == "__main__":
    main()
