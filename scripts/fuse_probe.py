"""The fusion kernel's timing and clustering form, for profiles/fuse_refactor.txt.

    python scripts/fuse_probe.py [--lib PATH] [--calls N]     time the five entry points, one line of medians
    rocprofv3 --kernel-trace -d OUT -o switch --output-format csv -- python scripts/fuse_probe.py --switch [--lib PATH]
                                                             the kernels either side of the bit-matrix / sequential switch

--lib: another build of libproben_hip.so (the parent's, from a second checkout) driven by this tree's Python; the C ABI is the same.
Timing: bench.py's proben_micro input (4096 images, n1, n2 ~ U{0..100}, K = 3, seed 2) through fuse_batch as "probEn" / "v-avg" and as
"probEn-log" plain, pooled, with_posterior and pooled + with_posterior + presence (the rows' log-posteriors are log p and log(1 - sum p));
10 warm-up calls, then the median of the HIP-event time of N calls, in ms.
--switch: gen_fuse_parent's batch at the last max_rows of the bit-matrix form and the next even one, plain and full."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import proben_amd  # noqa: F401
    from proben_amd import _lib, fusion as F
    if "--lib" in sys.argv:
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    if "--switch" in sys.argv:
        spec = importlib.util.spec_from_file_location("gen_fuse_parent", os.path.join(ROOT, "tests", "golden", "gen_fuse_parent.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        for run in gen.runs():
            if run[2] not in (gen.TIGHT, gen.WIDE) and run[1] == "counts":
                gen.run_case(run)
                print("ran", gen.run_name(run), flush=True)
        return
    from proben_amd.synthetic import synth_detections
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 200
    b, s, p, v, c, offs, src = F.pack_infos(synth_detections(4096, seed=2, kdet=2, nmax=100, K=3), "cuda", with_sources=True)
    nmax = int((offs[1:] - offs[:-1]).max().item())
    lp = torch.log(torch.cat([p, 1.0 - p.sum(1, keepdim=True)], 1).clamp_min(1e-300))
    table = torch.from_numpy(-(0.125 + 0.0625 * np.arange(16, dtype=np.float64).reshape(4, 4))).cuda()
    logp = dict(score_fusion="probEn-log", log_probs=lp)
    modes = [("plain", dict(score_fusion="probEn")), ("logp", logp), ("pooled", dict(logp, pool_weights=[0.75, 1.5], row_source=src)),
             ("posterior", dict(logp, with_posterior=True)),
             ("full", dict(logp, pool_weights=[0.75, 1.5], row_source=src, with_posterior=True, presence=table))]
    line = [os.path.relpath(_lib.LIB_PATH, ROOT)]
    for name, kw in modes:
        opts = F.O.FusionOptions.of(None, "fuse_probe", None, kw.pop("score_fusion"), "v-avg",
                                    **{k: kw.pop(k) for k in ("pool_weights", "with_posterior", "presence") if k in kw})
        ms = []
        for i in range(10 + calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            F.fuse_batch(b, s, p, v, c, offs, max_rows=nmax, options=opts, **kw)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        line.append(f"{name} {float(np.median(ms[10:])):.4f}")
    print("  ".join(line), flush=True)


if __name__ == "__main__":
    main()
