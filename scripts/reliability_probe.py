"""Kernel-trace workload for the reliability kernels (profiles/reliability_trace.txt): at M = 10^6 rows,
K + 1 = 4 and B = 15 bins, 10 launches each of pe_reliability_logits with the rows' own classes, pe_reliability_logits for the top
label and pe_reliability_scores, beside one pe_temperature_nll at 64 candidate temperatures over the same rows (the fit's kernel,
1.07 ms in profiles/calibration_trace.txt).

    rocprofv3 --kernel-trace --stats -d OUT -o reliability --output-format csv -- python scripts/reliability_probe.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import proben_amd  # noqa: E402,F401
from proben_amd import calibration as C  # noqa: E402

M, K1, B = 1_000_000, 4, 15
g = torch.Generator(device="cuda").manual_seed(14)
logits = torch.randn((M, K1), generator=g, device="cuda") * 3
labels = torch.randint(0, K1, (M,), generator=g, device="cuda", dtype=torch.int32)
classes = logits[:, :K1 - 1].argmax(dim=1).to(torch.int32)
conf = torch.rand((M,), generator=g, device="cuda", dtype=torch.float64)
correct = (torch.rand((M,), generator=g, device="cuda", dtype=torch.float64) < conf).to(torch.int32)
torch.cuda.synchronize()
for it in range(10):
    own = C.reliability(logits, labels, 1.3, classes, bins=B)            # reliability_kernel<LogitsSource> + pe::finish_kernel (csrc/reduce2.h)
    top = C.reliability(logits, labels, 1.3, None, bins=B)
    sc = C.reliability_scores(conf, correct, bins=B)                     # reliability_kernel<ScoresSource> + pe::finish_kernel
nll, _ = C.temperature_nll(logits, labels, np.exp(np.linspace(np.log(0.05), np.log(20.0), 64)))
torch.cuda.synchronize()
print("rows", own["rows"], top["rows"], sc["rows"], "ECE own / top / scores", own["ece"], top["ece"], sc["ece"], "NLL candidates", len(nll))
