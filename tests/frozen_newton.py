"""The two projected-Newton loops calibration.fit_pool_weights and calibration._fit_bias held before they became
calibration._projected_newton, kept as the reference of tests/test_fit_newton_cpu.py.  The bodies are the earlier ones line for line
with two changes: the objective is the injected `pool_nll(candidates)` / `bias_nll(candidates)` -> (nll [n], grad [n, .], excluded,
last) instead of the device call, and the lines marked `# hit` count the branch they stand in."""
import math

import numpy as np


def fit_pool_weights(pool_nll, C, D, hi, gtol, max_rounds, hits):
    h = 1e-4
    w = np.ones(D)
    f1, _, bad, _ = pool_nll([w])
    used = C - bad
    if used <= 0:
        raise ValueError(f"fit_pool_weights: no usable cluster ({bad} of {C} excluded: fewer than 2 rows, a label or a row source "
                         "out of range)")
    if not math.isfinite(f1[0]):
        raise ValueError("fit_pool_weights: the NLL at w = 1 is not finite (non-finite log-posteriors?)")
    rounds, converged = 0, False
    f, g = float(f1[0]), None
    while rounds < max_rounds:
        rounds += 1
        cand = np.vstack([w] + [w + h * np.eye(D)[d] for d in range(D)])
        fs, gs, _, _ = pool_nll(cand)
        f, g = float(fs[0]), gs[0]
        held = ((w <= 0) & (g > 0)) | ((w >= hi) & (g < 0))
        hits["held"] += int(held.any())                                     # hit
        pg = np.where(held, 0.0, g)
        if np.max(np.abs(pg)) <= gtol * used:
            converged = True
            hits["converged"] += 1                                          # hit
            break
        H = (gs[1:] - g[None, :]) / h
        H = 0.5 * (H + H.T)
        free = ~held
        p = np.zeros(D)
        try:
            Hf = H[np.ix_(free, free)] + 1e-10 * max(np.trace(H), 1.0) * np.eye(int(free.sum()))
            p[free] = -np.linalg.solve(Hf, g[free])
        except np.linalg.LinAlgError:
            p[free] = -g[free]
        if not (np.all(np.isfinite(p)) and p @ g < 0):
            p = np.where(free, -g, 0.0) / max(np.max(np.abs(np.diag(H))), 1e-300)
            hits["fallback"] += 1                                           # hit
        steps = 2.0 ** (1 - np.arange(40))
        trial = np.clip(w[None, :] + steps[:, None] * p[None, :], 0.0, hi)
        ft, _, _, _ = pool_nll(trial)
        ft = np.where(np.isfinite(ft), ft, np.inf)
        i = int(np.argmin(ft))
        if not ft[i] < f:
            hits["no_step"] += 1                                            # hit
            break
        w, f = trial[i], float(ft[i])
    else:
        hits["max_rounds"] += 1                                             # hit
    fs, gs, _, _ = pool_nll([w])
    f, g = float(fs[0]), gs[0]
    at = ["lo" if (w[d] <= 0 and g[d] > 0) else "hi" if (w[d] >= hi and g[d] < 0) else None for d in range(D)]
    return {"weights": [float(x) for x in w], "nll": f, "nll_at_1": float(f1[0]), "grad": [float(x) for x in g], "clusters": used,
            "excluded": bad, "rounds": rounds, "converged": converged, "at_bound": at}


def fit_bias(bias_nll, C, k1, hi, gtol, max_rounds, hits):
    K = k1 - 1
    h = 1e-4
    b = np.zeros(k1)
    f0, _, bad, _ = bias_nll([b])
    used = C - bad
    rec = {"clusters": used, "excluded": bad, "nll_at_0": float(f0[0]), "nll": float(f0[0]), "rounds": 0, "converged": used == 0,
           "at_bound": [None] * K, "grad": [0.0] * K}
    if used == 0:
        hits["zero_row"] += 1                                               # hit
        return b, rec
    if not math.isfinite(f0[0]):
        raise ValueError("fit_presence: the NLL at a zero row is not finite")
    eye = np.eye(k1)[:K]
    rounds, converged, f = 0, False, float(f0[0])
    while rounds < max_rounds:
        rounds += 1
        fs, gs, _, _ = bias_nll(np.vstack([b] + [b + h * eye[d] for d in range(K)]))
        f, g = float(fs[0]), gs[0, :K]
        x = b[:K]
        held = ((x <= -hi) & (g > 0)) | ((x >= hi) & (g < 0))
        hits["held"] += int(held.any())                                     # hit
        pg = np.where(held, 0.0, g)
        if np.max(np.abs(pg)) <= gtol * used:
            converged = True
            hits["converged"] += 1                                          # hit
            break
        H = (gs[1:, :K] - g[None, :]) / h
        H = 0.5 * (H + H.T)
        free = ~held
        p = np.zeros(K)
        try:
            Hf = H[np.ix_(free, free)] + 1e-10 * max(np.trace(H), 1.0) * np.eye(int(free.sum()))
            p[free] = -np.linalg.solve(Hf, g[free])
        except np.linalg.LinAlgError:
            p[free] = -g[free]
        if not (np.all(np.isfinite(p)) and p @ g < 0):
            p = np.where(free, -g, 0.0) / max(np.max(np.abs(np.diag(H))), 1e-300)
            hits["fallback"] += 1                                           # hit
        steps = 2.0 ** (1 - np.arange(40))
        trial = np.zeros((40, k1))
        trial[:, :K] = np.clip(x[None, :] + steps[:, None] * p[None, :], -hi, hi)
        ft, _, _, _ = bias_nll(trial)
        ft = np.where(np.isfinite(ft), ft, np.inf)
        i = int(np.argmin(ft))
        if not ft[i] < f:
            hits["no_step"] += 1                                            # hit
            break
        b, f = trial[i], float(ft[i])
    else:
        hits["max_rounds"] += 1                                             # hit
    fs, gs, _, _ = bias_nll([b])
    g = gs[0, :K]
    rec.update({"nll": float(fs[0]), "rounds": rounds, "converged": converged, "grad": [float(v) for v in g],
                "at_bound": ["lo" if (b[d] <= -hi and g[d] > 0) else "hi" if (b[d] >= hi and g[d] < 0) else None for d in range(K)]})
    return b, rec
