"""Time of the V sweep of cmf_als_cg_step with its long rows cut into pieces (option "als_cg_piece", als_cg_piece_kernel /
als_cg_combine_kernel) beside the same sweep with no row cut and beside the V sweep of cmf_als_step, in the same process, on the
same context, pattern and factors, nn_mask = 0.

    python tools/als_cg_pieces_timing.py [--out profiles/als_cg_pieces_timing.json] [--reps 5] [--cases vz64 vz256 vu64 vu256 ua ub64 ub256]

The protocol of tools/als_cg_timing.py: every case in a child process of its own under its own time limit, nothing more is started
after a child that fails; after a warm-up call, median of `reps` device-timed repetitions, every one from the same factors, all
samples kept.  Cases (6 CG steps):
  vz64 / vz256   C5's pattern with Zipf(1.1) columns, 1e6 x 1e5, 100 entries per row, k = 64 / 256: the V sweep (its hot columns are
                 rows of up to 1e6 entries) with "als_cg_piece" = -1 (no row is cut), 2048, 4096, 16384, 65536, and of cmf_als_step
  vu64 / vu256   the same with uniform columns (rows of ~1000 entries: none is cut at any of these lengths)
  ua / ub64 / ub256   the U sweeps of cases a, b64 and b256 of tools/als_cg_timing.py at the default piece length and with
                 "als_cg_piece" = -1: their rows are short, the code path is the one without pieces
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
STEPS = 6
PIECES = (-1, 2048, 4096, 16384, 65536)
CASES = ("vz64", "vz256", "vu64", "vu256", "ua", "ub64", "ub256")
CHILD_LIMIT_S = 420


def measure(lib, case, reps):
    l2 = 0.1
    if case == "ua":
        m, d, p, k, npr = 65536, 65536, 256, 256, 1024
        rng = np.random.default_rng(42)
        indices = rng.integers(0, d, size=m * npr, dtype=np.int32)
        indptr = np.arange(0, m * npr + 1, npr, dtype=np.int64)
        scale = (0.7979 / k) ** 0.5
    else:
        zipf = case.startswith("vz")
        m, d, p, k, npr = 1000000, 100000, 64, int(case[2:]), 100
        Xs = _csr_matrix("c5z" if zipf else "c5", m, d, npr)
        indptr, indices = Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32)
        del Xs
        scale = (npr / d / k) ** 0.5
    print("case %s: pattern ready" % case, flush=True)
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    nnz = indices.size
    ctx.set_weighted_csr(0, indptr, indices, np.random.default_rng(1 if case == "ua" else 2).random(nnz) + 0.5, np.ones(nnz))
    col_len = np.bincount(indices, minlength=d)
    del indices
    ctx.fill_data_synthetic(1, 43)
    print("case %s: bound" % case, flush=True)

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    rec = {"case": case, "m": m, "d": d, "p": p, "k": k, "k_pad": ctx.geometry()[3], "entries_per_row": npr, "nnz": int(nnz), "reps": reps,
           "l2": l2, "nn_mask": 0, "steps": STEPS}
    sweep_v = case.startswith("v")
    mask, tag = (V_BIT, "v_") if sweep_v else (U_BIT, "u_")
    if sweep_v:
        rec["v_row_entries_max_median"] = [int(col_len.max()), float(np.median(col_len))]
        a, a_all, classes = _timed(ctx, lib, reps, reset, lambda: ctx.als_step(l2, 0, mask))
        rec.update({"v_als_kernel_ms": a, "v_als_kernel_ms_all": a_all, "v_als_kernel_classes_ms": classes})
        print("  v_als: kernels %.2f ms" % a, flush=True)
    for piece in (PIECES if sweep_v else (-1, 0)):
        ctx.set_option("als_cg_piece", piece)
        b, b_all, cl = _timed(ctx, lib, reps, reset, lambda: ctx.als_cg_step(l2, 0, mask, STEPS, 0))
        name = "%scg%d_piece_%s" % (tag, STEPS, "off" if piece < 0 else ("default" if piece == 0 else str(piece)))
        rec.update({name + "_kernel_ms": b, name + "_kernel_ms_all": b_all, name + "_kernel_classes_ms": cl,
                    name + "_long_rows_pieces": list(ctx.als_cg_last())})
        if sweep_v:
            rec[name + "_over_als"] = b / rec["v_als_kernel_ms"]
        print("  %s: kernel %.2f ms, long rows and pieces %s" % (name, b, ctx.als_cg_last()), flush=True)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_cg_pieces_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case, in this process; the record goes to the file --out names
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_cg_pieces_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    out = {"what": "V sweep of cmf_als_cg_step (6 steps) with the long rows cut into pieces of als_cg_piece entries, with no row cut, and "
                   "the V sweep of cmf_als_step; U sweeps at the default piece length; same process, context, pattern and factors, "
                   "nn_mask = 0; medians of device-timed repetitions, every repetition from the same factors",
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
            raise SystemExit("als_cg_pieces_timing: case %s ran out of its %d s; nothing more is started" % (case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_cg_pieces_timing: case %s ended with status %d; nothing more is started" % (case, status))
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
