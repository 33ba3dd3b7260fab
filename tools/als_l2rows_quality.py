"""Fit quality under the frequency-scaled regulariser (als_l2_scale = nu), from the float64 yardstick on the CPU
(tests/als_l2rows_yardstick.py): no device, no library.

    python tools/als_l2rows_quality.py [--out profiles/als_l2rows_quality.json]

Two settings, nu in {0, 0.5, 1}, each at the best l2 of GRID (the best by the reported figure itself, per seed: an upper bound of
what a validation split would pick, the same for every nu), seeds 3 / 5 / 7, signed exact rows:
  ratings   the planted rating problem of tests/als_bias_yardstick.py (120 x 150, rank 3, unit-variance row and column offsets,
            noise 0.5, Y full) with 10 % of the cells observed, redrawn so that the row lengths follow a Zipf law (row i is
            observed with probability min(1, c / (i + 1)), c such that a tenth of the cells is expected: about 150, 150, 112, 84 ...
            down to 3 expected entries; a row may draw none).  The data are centred by the mean of the observed entries and fitted WITHOUT biases at k = 6 (the
            bias blocks keep their own unscaled regulariser; the yardstick under multipliers has none), 10 iterations.  Figure:
            RMSE on the unobserved cells.
  clicks    the click problem of tests/click_problem.py (120 x 150, confidences 1 + count, a held-out quarter of the clicks) under
            the background weight 1 at k = 8, 10 iterations; the multipliers are (n_i + 1 * D)^nu.  Figure: recall@10."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import als_bias_yardstick as B  # noqa: E402
import als_l2rows_yardstick as LR  # noqa: E402
import click_problem as CP  # noqa: E402
from pycmf_amd.solver_shell import l2_multipliers  # noqa: E402

GRID = (0.001, 0.003, 0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0, 300.0)
NUS = (0.0, 0.5, 1.0)
SEEDS = (3, 5, 7)
ITERS = 10


def zipf_mask(seed, m, d, share=0.10):
    lo, hi = 0.0, float(m)
    for _ in range(60):                                      # c with mean_i min(1, c / (i + 1)) = share
        c = 0.5 * (lo + hi)
        lo, hi = (c, hi) if np.minimum(1.0, c / np.arange(1, m + 1)).mean() < share else (lo, c)
    prob = np.minimum(1.0, c / np.arange(1, m + 1))
    return (np.random.RandomState(1000 + seed).rand(m, d) < prob[:, None]).astype(np.float64)


def ratings(seed, nu, l2):
    X, Y, _, _ = B.planted(seed, 0.10, 0.5, k=6)
    W = zipf_mask(seed, *X.shape)
    Ws = sp.csr_matrix(W)
    Xc = X - (X * W).sum() / W.sum()
    F = tuple(0.1 * np.random.RandomState(2000 + seed).randn(n, 6) for n in (X.shape[0], X.shape[1], Y.shape[1]))
    mults = l2_multipliers(X.shape, Y.shape, Ws, None, nu=nu)
    for _ in range(ITERS):
        F = LR.step(Xc, Y, Ws, None, *F, l2, mults)
    off = W == 0
    return float(np.sqrt((((Xc - F[0] @ F[1].T) ** 2)[off]).mean())), [int(W.sum(axis=1).max()), int(W.sum(axis=1).min())]


def clicks(seed, nu, l2):
    counts, train, test, Y, U0, V0, Z0 = CP.clicks(seed)
    P, W = CP.click_relations(counts, train)
    mults = l2_multipliers(P.shape, Y.shape, W, None, x_background_weight=1.0, nu=nu)
    F = (U0, V0, Z0)
    for _ in range(ITERS):
        F = LR.step(P.toarray(), Y, W, None, *F, l2, mults, cx=1.0)
    return CP.recall_at(F[0] @ F[1].T, train, test, 10), [float(mults[0].max()), float(mults[0].min())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_l2rows_quality.json"))
    a = ap.parse_args()
    out = {"what": __doc__.split("\n\n")[0], "grid": list(GRID), "nus": list(NUS), "seeds": list(SEEDS), "iterations": ITERS, "settings": {}}
    for name, run, better in (("ratings", ratings, min), ("clicks", clicks, max)):
        rows = []
        for nu in NUS:
            per_seed = []
            for seed in SEEDS:
                vals = [run(seed, nu, l2)[0] for l2 in GRID]
                best = better(range(len(GRID)), key=lambda i: vals[i])
                per_seed.append({"seed": seed, "best_l2": GRID[best], "best": vals[best], "all": vals, "extent": run(seed, nu, GRID[best])[1]})
                print(name, "nu", nu, "seed", seed, "best l2", GRID[best], "figure %.4f" % vals[best], flush=True)
            rows.append({"nu": nu, "mean_best": float(np.mean([p["best"] for p in per_seed])), "per_seed": per_seed})
        out["settings"][name] = {"figure": "RMSE on the unobserved cells (lower is better)" if name == "ratings" else "recall@10 (higher is better)",
                                 "rows": rows}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
