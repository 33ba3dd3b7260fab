"""Time of the non-negative row solve of the ALS solver (als_nnls_kernel, cmf_als_nnls_step) beside the Cholesky solves of
cmf_als_step that it replaces.

    python tools/als_nnls_timing.py [--out profiles/als_nnls_timing.json] [--reps 5] [--sweeps 4] [--rows 65536]

Case 1 of tools/als_timing.py: 65536 rows x 1024 uniformly drawn stored entries per row over d = 65536 columns, p = 256, k = 256, Y
dense and unweighted -- the U sweep (65536 rows) and the V sweep (65536 rows, a full side beside the pattern) go row by row, the Z
sweep has the one shared matrix.  After a warm-up call, median of `reps` device-timed repetitions, every one from the same
factors, profiler off, all samples kept:
  nnls_*_hals_ms          class "hals" (the coordinate-descent kernel) of a U-only / V-only / whole cmf_als_nnls_step, nn_mask = 7
  als_*_eigen_ms          class "eigen" (the Cholesky solves) of the same cmf_als_step calls on the same context, nn_mask = 7
  nnls_over_cholesky      their ratio for the U and V sweeps together (the aim: <= 1)
  *_step_wall_ms          wall time of whole iterations of both, timing off
  h_bytes_per_pass        rows k_pad^2 4: what one pass over every H_i reads; the kernel makes sweeps + 1 passes
Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kl_timing import _wall  # noqa: E402  (the same protocol)

U_BIT, V_BIT, Z_BIT = 1, 2, 4


def _timed(ctx, reps, reset, call, cls):
    """median over reps of the kernel ms of class `cls` for one `call` after `reset`; also every sample and the launches."""
    reset()
    call()                                                  # warm-up (sizes every workspace)
    ctx.kernel_timing(True)
    out, launches = [], 0
    for _ in range(reps):
        reset()
        ctx.sync()
        ctx.kernel_timing_reset()
        call()
        ms, launches = ctx.kernel_time(cls)[:2]
        out.append(ms)
    ctx.kernel_timing(False)
    return statistics.median(out), out, launches


def measure(lib, reps, sweeps, m=65536, d=65536, per_row=1024, p=256, k=256):
    l2 = 0.1
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    rng = np.random.default_rng(42)
    indices = rng.integers(0, d, size=m * per_row, dtype=np.int32)
    indptr = np.arange(0, m * per_row + 1, per_row, dtype=np.int64)
    ctx.set_weighted_csr(0, indptr, indices, np.random.default_rng(1).random(indices.size) + 0.5, np.ones(indices.size))
    del indices
    ctx.fill_data_synthetic(1, 43)
    scale = (0.7979 / k) ** 0.5

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    kp = ctx.geometry()[3]
    rec = {"case": "case1", "m": m, "d": d, "p": p, "k": k, "k_pad": kp, "entries_per_row": per_row, "reps": reps, "l2": l2, "sweeps": sweeps,
           "nn_mask": 7, "h_bytes_per_pass": {"U": m * kp * kp * 4, "V": d * kp * kp * 4}, "passes_over_h": sweeps + 1}
    for name, mask in (("u", U_BIT), ("v", V_BIT), ("step", 7)):
        a, a_all, n = _timed(ctx, reps, reset, lambda: ctx.als_nnls_step(l2, 7, mask, sweeps), "hals")
        b, b_all, nb = _timed(ctx, reps, reset, lambda: ctx.als_step(l2, 7, mask), "eigen")
        rec.update({"nnls_%s_hals_ms" % name: a, "nnls_%s_hals_ms_all" % name: a_all, "nnls_%s_hals_launches" % name: n,
                    "als_%s_eigen_ms" % name: b, "als_%s_eigen_ms_all" % name: b_all, "als_%s_eigen_launches" % name: nb})
    rec["nnls_over_cholesky"] = (rec["nnls_u_hals_ms"] + rec["nnls_v_hals_ms"]) / (rec["als_u_eigen_ms"] + rec["als_v_eigen_ms"])
    rec["nnls_u_h_read_tb_per_s"] = rec["h_bytes_per_pass"]["U"] * (sweeps + 1) / rec["nnls_u_hals_ms"] * 1e-9
    rec["four_sweeps_cost_no_more_than_the_solves"] = bool(rec["nnls_over_cholesky"] <= 1.0)
    names = list(lib.KERNEL_CLASSES) + list(lib.LATER_KERNEL_CLASSES)
    for tag, call in (("nnls", lambda: ctx.als_nnls_step(l2, 7, 7, sweeps)), ("als", lambda: ctx.als_step(l2, 7, 7))):
        reset()
        ctx.kernel_timing(True)
        ctx.kernel_timing_reset()
        call()
        rec["%s_step_kernel_classes_ms" % tag] = {n: ctx.kernel_time(n)[0] for n in names if ctx.kernel_time(n)[1]}
        ctx.kernel_timing(False)
        reset()
        w, w_all = _wall(ctx, reps, call)
        rec["%s_step_wall_ms" % tag], rec["%s_step_wall_ms_all" % tag] = w, w_all
    rec["nnls_over_als_step_wall"] = rec["nnls_step_wall_ms"] / rec["als_step_wall_ms"]
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_nnls_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--rows", type=int, default=65536)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("als_nnls_timing: no GPU visible (needs an MI355X)")
    rec = measure(_lib, a.reps, a.sweeps, m=a.rows)
    print(json.dumps(rec), flush=True)
    out = {"what": "coordinate-descent row solve of cmf_als_nnls_step against the Cholesky solves of cmf_als_step on the same pattern, "
                   "context and machine; medians of device-timed repetitions, every repetition from the same factors", "cases": [rec]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
