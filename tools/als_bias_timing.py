"""Cost of the bias terms of the ALS solver (cmf_set_biases, cmf_als_bias_step; csrc/cmf_als_bias.hip.h) beside the code without
them, in the same process, on the same context, pattern and factors, nn_mask = 0.

    python tools/als_bias_timing.py [--out profiles/als_bias_timing.json] [--reps 5] [--cases a u64 u256 z256] [--parts a b c]

The protocol of tools/als_cg_timing.py: every case in a child process of its own under its own time limit, nothing more is started
after a child that fails; after a warm-up call, median of `reps` device-timed repetitions, every one from the same factors and
biases, all samples kept.  The yardstick is the code without biases: cmf_weighted_residual_sq's CSR pass over X (it reads what one
bias sweep reads, less one gathered float per entry and two doubles per piece), cmf_als_cg_step and cmf_als_step.
Cases:
  a              65536 x 65536, 1024 entries per row, k = 256
  u64 / u256     C5's pattern with uniform columns, 1e6 x 1e5, 100 entries per row, k = 64 / 256
  z256           C5's pattern with Zipf(1.1) columns (columns of up to 1e6 entries), k = 256
Parts:
  a   one row-bias sweep of X (cmf_als_bias_rows, axis 0) against that pass
  b   cmf_als_bias_step with 6 CG steps against cmf_als_cg_step (6 steps), and with the exact rows against cmf_als_step: the share
      of an iteration that the biases cost (the bias sweeps and the rewrite of the adjusted targets)
  c   the column-bias sweep of X (axis 1) at "als_bias_piece" = 2048, 16384 and -1 (every row one piece)
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

from kl_timing import _csr_matrix  # noqa: E402  (the same C5 patterns)
from als_cg_timing import _timed  # noqa: E402  (the same protocol)

STEPS = 6
PIECES = (2048, 16384, -1)
CASES = ("a", "u64", "u256", "z256")
PARTS = ("a", "b", "c")
CHILD_LIMIT_S = 540


def measure(lib, case, reps, parts):
    l2, lb = 0.1, 0.1
    if case == "a":
        m, d, p, k, npr = 65536, 65536, 256, 256, 1024
        rng = np.random.default_rng(42)
        indices = rng.integers(0, d, size=m * npr, dtype=np.int32)
        indptr = np.arange(0, m * npr + 1, npr, dtype=np.int64)
        scale = (0.7979 / k) ** 0.5
    else:
        m, d, p, k, npr = 1000000, 100000, 64, int(case[1:]), 100
        Xs = _csr_matrix("c5z" if case.startswith("z") else "c5", m, d, npr)
        indptr, indices = Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32)
        del Xs
        scale = (npr / d / k) ** 0.5
    print("case %s: pattern ready" % case, flush=True)
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    nnz = indices.size
    ctx.set_weighted_csr(0, indptr, indices, np.random.default_rng(2).random(nnz) + 0.5, np.ones(nnz))
    col_len = np.bincount(indices, minlength=d)
    del indices
    ctx.fill_data_synthetic(1, 43)
    print("case %s: bound" % case, flush=True)
    zeros = (np.zeros(m), np.zeros(d))

    def factors():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)

    def reset():
        factors()
        if ctx.get_biases(0)[2]:
            ctx.set_bias(0, 0, zeros[0])
            ctx.set_bias(0, 1, zeros[1])
    rec = {"case": case, "m": m, "d": d, "p": p, "k": k, "k_pad": ctx.geometry()[3], "entries_per_row": npr, "nnz": int(nnz), "reps": reps,
           "l2": l2, "lb": lb, "nn_mask": 0, "cg_steps": STEPS, "col_entries_max_median": [int(col_len.max()), float(np.median(col_len))]}

    def put(name, call):
        v, v_all, classes = _timed(ctx, lib, reps, reset, call)
        rec.update({name + "_kernel_ms": v, name + "_kernel_ms_all": v_all, name + "_kernel_classes_ms": classes})
        print("  %s: kernels %.3f ms" % (name, v), flush=True)
        return v
    # the code without biases first, on a context that has never had any
    res = put("residual_pass", lambda: ctx.weighted_residual_sq(True, False))
    if "b" in parts:
        cg = put("als_cg_step", lambda: ctx.als_cg_step(l2, 0, 7, STEPS, 0))
        ex = put("als_step", lambda: ctx.als_step(l2, 0, 7))
    ctx.set_biases(0, True, 0.75, lb)
    if "a" in parts:
        v = put("row_bias_sweep", lambda: ctx.als_bias_rows(0, 0))
        rec["row_bias_sweep_over_residual_pass"] = v / res
    if "c" in parts:
        for piece in PIECES:
            ctx.set_option("als_bias_piece", piece)
            name = "col_bias_sweep_piece_%s" % ("off" if piece < 0 else str(piece))
            v = put(name, lambda: ctx.als_bias_rows(0, 1))
            rec[name + "_over_residual_pass"] = v / res
        ctx.set_option("als_bias_piece", 0)
    if "b" in parts:
        bcg = put("als_bias_step_cg", lambda: ctx.als_bias_step(l2, 0, 7, STEPS, 0))
        bex = put("als_bias_step_exact", lambda: ctx.als_bias_step(l2, 0, 7, 0, 0))
        rec["bias_share_of_cg_iteration"] = (bcg - cg) / bcg
        rec["bias_share_of_exact_iteration"] = (bex - ex) / bex
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_bias_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--parts", nargs="*", default=list(PARTS), choices=PARTS)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case, in this process; the record goes to the file --out names
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_bias_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps, a.parts)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    out = {"what": "bias sweeps of X (cmf_als_bias_rows) beside the CSR pass of cmf_weighted_residual_sq, and cmf_als_bias_step beside "
                   "cmf_als_cg_step (6 steps) and cmf_als_step; same process, context, pattern and factors, nn_mask = 0; medians of "
                   "device-timed repetitions, every repetition from the same factors and zero biases",
           "cases": []}
    if os.path.exists(a.out):                                # cases measured by an earlier call stay
        with open(a.out) as f:
            out["cases"] = [r for r in json.load(f).get("cases", []) if r.get("case") not in a.cases]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases:
        part = a.out + "." + case + ".part"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--out", part, "--reps", str(a.reps), "--parts"] + list(a.parts)
        try:
            status = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("als_bias_timing: case %s ran out of its %d s; nothing more is started" % (case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_bias_timing: case %s ended with status %d; nothing more is started" % (case, status))
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
