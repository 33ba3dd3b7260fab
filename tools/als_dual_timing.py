"""Time of the dual form of the exact ALS rows (cmf_als_dual_step, csrc/cmf_als_dual.hip.h) beside the exact sweep of cmf_als_step
that it replaces (normal equations + k x k Cholesky solves) and, for context, 6 conjugate-gradient steps (cmf_als_cg_step), in the
same process, on the same pattern and factors, nn_mask = 0, U sweep.

    python tools/als_dual_timing.py [--out profiles/als_dual_timing.json] [--reps 5] [--cases c5_256 c5_128 lt_256 lt_128 a]

The protocol of tools/als_cg_timing.py: every case in a child process of its own under its own time limit (after a child that
fails, is killed or runs out of time nothing more is started); profiler off; after a warm-up call the median of `reps` device-timed
repetitions, every one from the same factors, all samples kept.  Cases:
  c5_256 / c5_128   C5's pattern as bench.py defines it: 1e6 x 1e5, 100 entries per row, uniform columns, k = 256 / 128
                    (k = 128: the class of 100 entries is 128 = k_pad, so no row goes dual: the figure must equal the exact sweep's)
  lt_256 / lt_128   a long-tail pattern: 1e6 x 1e5, 20 entries per row, k = 256 / 128
  a                 65536 rows x 1024 entries over 65536 columns, k = 256: no row is eligible, the figure must equal the exact
                    sweep's within the run-to-run spread of that sweep
Per case: als_* the exact sweep (the yardstick: the parent's code, untouched), dual_* the same sweep under dual_max = 128,
cg6_* six CG steps; *_kernel_ms every kernel class added up, *_kernel_classes_ms the classes (rowhess: normal equations / dual
Gram, eigen: the Cholesky solves, elementwise: finish, back-product, scatter), *_wall_ms the wall time of the same calls with
timing off (host planning and the indptr read-back included); dual_over_als their ratio; dual_last the rows per route.
Fails without a GPU."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from als_cg_timing import _timed  # noqa: E402  (the same protocol)
from kl_timing import _csr_matrix, _wall  # noqa: E402  (and the same C5 pattern)

U_BIT = 1
DUAL_MAX = 128
CG_STEPS = 6
CASES = ("c5_256", "c5_128", "lt_256", "lt_128", "a")
CHILD_LIMIT_S = 420


def measure(lib, case, reps):
    l2 = 0.1
    if case == "a":
        m, d, p, k, npr = 65536, 65536, 256, 256, 1024
        rng = np.random.default_rng(42)
        indices = rng.integers(0, d, size=m * npr, dtype=np.int32)
        indptr = np.arange(0, m * npr + 1, npr, dtype=np.int64)
        scale = (0.7979 / k) ** 0.5
    else:
        m, d, p, k, npr = 1000000, 100000, 64, int(case.split("_")[1]), 100 if case.startswith("c5") else 20
        Xs = _csr_matrix("c5", m, d, npr)
        indptr, indices = Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32)
        del Xs
        scale = (npr / d / k) ** 0.5
    print("case %s: pattern ready" % case, flush=True)
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    nnz = indices.size
    ctx.set_weighted_csr(0, indptr, indices, np.random.default_rng(1 if case == "a" else 2).random(nnz) + 0.5, np.ones(nnz))
    del indices
    ctx.fill_data_synthetic(1, 43)
    print("case %s: bound" % case, flush=True)

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    rec = {"case": case, "m": m, "d": d, "p": p, "k": k, "k_pad": ctx.geometry()[3], "entries_per_row": npr, "nnz": int(nnz), "reps": reps, "l2": l2,
           "nn_mask": 0, "dual_max": DUAL_MAX, "cg_steps": CG_STEPS}
    calls = (("als", lambda: ctx.als_step(l2, 0, U_BIT)),
             ("dual", lambda: ctx.als_dual_step(l2, 0, U_BIT, DUAL_MAX)),
             ("cg%d" % CG_STEPS, lambda: ctx.als_cg_step(l2, 0, U_BIT, CG_STEPS, 0)))
    for tag, call in calls:
        kms, k_all, classes = _timed(ctx, lib, reps, reset, call)
        reset()
        w, w_all = _wall(ctx, reps, call)
        rec.update({tag + "_kernel_ms": kms, tag + "_kernel_ms_all": k_all, tag + "_kernel_classes_ms": classes,
                    tag + "_wall_ms": w, tag + "_wall_ms_all": w_all})
        if tag == "dual":
            rec["dual_last"] = list(ctx.als_dual_last())
        print("  %s: kernels %.2f ms, wall %.2f ms, classes %s" % (tag, kms, w, {n: round(v, 2) for n, v in classes.items()}), flush=True)
    rec["dual_over_als"] = rec["dual_kernel_ms"] / rec["als_kernel_ms"]
    rec["dual_wall_over_als"] = rec["dual_wall_ms"] / rec["als_wall_ms"]
    rec["als_spread"] = (max(rec["als_kernel_ms_all"]) - min(rec["als_kernel_ms_all"])) / rec["als_kernel_ms"]
    # the same rows from both routes, once: the largest difference relative to the largest entry
    reset()
    ctx.als_step(l2, 0, U_BIT)
    exact = ctx.get_factor(0)[:4096]
    reset()
    ctx.als_dual_step(l2, 0, U_BIT, DUAL_MAX)
    dual = ctx.get_factor(0)[:4096]
    rec["dual_minus_als_max_rel"] = float(np.abs(dual - exact).max() / np.abs(exact).max())
    print("  dual / als: kernels %.3f, wall %.3f; rows differ by %.2e of the largest entry" %
          (rec["dual_over_als"], rec["dual_wall_over_als"], rec["dual_minus_als_max_rel"]), flush=True)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_dual_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case, in this process; the record goes to the file --out names
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_dual_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    out = {"what": "U sweep of cmf_als_dual_step (dual_max = 128) against the same sweep of cmf_als_step (normal equations + k x k Cholesky solves) "
                   "and of cmf_als_cg_step (6 steps), same process, pattern and factors, nn_mask = 0; medians of device-timed repetitions, "
                   "every repetition from the same factors",
           "cases": []}
    if os.path.exists(a.out):                                # cases measured by an earlier call stay
        with open(a.out) as f:
            out["cases"] = [r for r in json.load(f).get("cases", []) if r.get("case") not in a.cases]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases:
        part = a.out + "." + case + ".part"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--out", part, "--reps", str(a.reps)]
        try:
            status = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("als_dual_timing: case %s ran out of its %d s; nothing more is started" % (case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_dual_timing: case %s ended with status %d; nothing more is started" % (case, status))
        with open(part) as f:
            out["cases"].append(json.load(f))
        os.remove(part)
        print(json.dumps(out["cases"][-1]), flush=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
