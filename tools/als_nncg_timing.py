"""Time of the matrix-free non-negative row solve of the ALS solver (als_nncg_kernel, cmf_als_nncg_step) beside the formed route it
stands in for (cmf_als_nnls_step with 4 sweeps: normal equations + coordinate descent), in the same process, on the same pattern
and factors, every factor non-negative.

    python tools/als_nncg_timing.py [--out profiles/als_nncg_timing.json] [--reps 5] [--cases a b64 b256 bz256] [--steps 3 6]

The protocol of tools/als_cg_timing.py: every case in a child process of its own under its own time limit, nothing more is started
after a child that fails; after a warm-up call the median of `reps` device-timed repetitions, every one from the same factors.
Cases:
  a        65536 rows x 1024 uniformly drawn entries over 65536 columns, k = 256                                       (U sweep)
  b64 / b256   C5's pattern as bench.py defines it, 1e6 x 1e5, 100 entries per row, uniform columns, k = 64 / 256     (U sweep)
  bz256    the same with Zipf(1.1) columns, k = 256: the V sweep (its long rows), with pieces ("als_cg_piece" default) and without
Per sweep:
  nnls4_kernel_ms          every kernel class of a one-factor cmf_als_nnls_step with 4 sweeps added up; nnls4_kernel_classes_ms
  nncg<n>_kernel_ms        every kernel class of the same one-factor cmf_als_nncg_step with n steps (rowhess: the new kernels)
  nncg<n>_passes_per_row   passes actually run (cmf_als_nncg_passes), mean over the rows; nncg<n>_entry_passes: stored entries read
  nncg<n>_ms_per_pass      kernel ms of the rowhess class over entry passes / nnz
  nncg<n>_over_nnls4       the ratio of the two kernel times
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

U_BIT, V_BIT = 1, 2
NN_ALL = 7
CASES = ("a", "b64", "b256", "bz256")
CHILD_LIMIT_S = 540


def _sweep(ctx, lib, reps, reset, l2, mask, steps_list, tag, rec, nnz, rows, formed=True):
    a = None
    if formed:
        a, a_all, classes = _timed(ctx, lib, reps, reset, lambda: ctx.als_nnls_step(l2, NN_ALL, mask, 4))
        rec.update({tag + "nnls4_kernel_ms": a, tag + "nnls4_kernel_ms_all": a_all, tag + "nnls4_kernel_classes_ms": classes})
        print("  %snnls 4 sweeps: kernels %.2f ms" % (tag, a), flush=True)
    for n in steps_list:
        b, b_all, cl = _timed(ctx, lib, reps, reset, lambda: ctx.als_nncg_step(l2, NN_ALL, mask, 0, n, 0))
        passes, entry_passes = ctx.als_nncg_passes()
        name = "%snncg%d_" % (tag, n)
        rec.update({name + "kernel_ms": b, name + "kernel_ms_all": b_all, name + "kernel_classes_ms": cl,
                    name + "passes_per_row": passes / rows, name + "entry_passes": entry_passes,
                    name + "ms_per_pass": cl.get("rowhess", b) / (entry_passes / nnz) if entry_passes else None,
                    name + "long_rows_pieces": list(ctx.als_nncg_last())})
        if a is not None:
            rec[name + "over_nnls4"] = b / a
        print("  %snncg %d steps: kernels %.2f ms, %.2f passes per row%s" % (tag, n, b, passes / rows, "" if a is None else " (%.3f of nnls4)" % (b / a)),
              flush=True)


def measure(lib, case, reps, steps_list):
    l2 = 0.1
    if case == "a":
        m, d, p, k, npr = 65536, 65536, 256, 256, 1024
        rng = np.random.default_rng(42)
        indices = rng.integers(0, d, size=m * npr, dtype=np.int32)
        indptr = np.arange(0, m * npr + 1, npr, dtype=np.int64)
        scale = (0.7979 / k) ** 0.5
    else:
        zipf = case.startswith("bz")
        m, d, p, k, npr = 1000000, 100000, 64, int(case[2 if zipf else 1:]), 100
        Xs = _csr_matrix("c5z" if zipf else "c5", m, d, npr)
        indptr, indices = Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32)
        del Xs
        scale = (npr / d / k) ** 0.5
    print("case %s: pattern ready" % case, flush=True)
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    nnz = indices.size
    ctx.set_weighted_csr(0, indptr, indices, np.random.default_rng(1 if case == "a" else 2).random(nnz) + 0.5, np.ones(nnz))
    col_len = np.bincount(indices, minlength=d)
    del indices
    ctx.fill_data_synthetic(1, 43)
    print("case %s: bound" % case, flush=True)

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    rec = {"case": case, "m": m, "d": d, "p": p, "k": k, "k_pad": ctx.geometry()[3], "entries_per_row": npr, "nnz": int(nnz), "reps": reps, "l2": l2,
           "nn_mask": NN_ALL, "steps": list(steps_list)}
    if case != "bz256":
        _sweep(ctx, lib, reps, reset, l2, U_BIT, steps_list, "u_", rec, nnz, m)
    else:                                                   # the V sweep: the hot columns are rows of up to ~m entries
        rec["v_row_entries_max_median"] = [int(col_len.max()), float(np.median(col_len))]
        _sweep(ctx, lib, reps, reset, l2, V_BIT, steps_list, "v_", rec, nnz, d)
        ctx.set_option("als_cg_piece", -1)
        _sweep(ctx, lib, reps, reset, l2, V_BIT, steps_list, "v_uncut_", rec, nnz, d, formed=False)
        ctx.set_option("als_cg_piece", 0)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_nncg_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--steps", nargs="*", type=int, default=[3, 6])
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case, in this process; the record goes to the file --out names
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_nncg_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps, a.steps)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    out = {"what": "one-factor sweep of cmf_als_nncg_step (matrix-free projected CG rows) against the same sweep of cmf_als_nnls_step with "
                   "4 sweeps (normal equations + coordinate descent), same process, pattern and factors, every factor non-negative; "
                   "medians of device-timed repetitions, every repetition from the same factors",
           "cases": []}
    if os.path.exists(a.out):                                # cases measured by an earlier call stay
        with open(a.out) as f:
            out["cases"] = [r for r in json.load(f).get("cases", []) if r.get("case") not in a.cases]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases:
        part = a.out + "." + case + ".part"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--out", part, "--reps", str(a.reps), "--steps"] + [str(s) for s in a.steps]
        try:
            status = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("als_nncg_timing: case %s ran out of its %d s; nothing more is started" % (case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_nncg_timing: case %s ended with status %d; nothing more is started" % (case, status))
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
