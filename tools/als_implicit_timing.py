"""Cost of a background weight (implicit feedback, cmf_set_background_weight) on the U sweep of the ALS solver: the same sweep with
c0 = 1 and with c0 = 0 in the same process, on the same pattern, weights and factors, on the exact route (cmf_als_step) and with
6 CG steps (cmf_als_cg_step), nn_mask = 0.

    python tools/als_implicit_timing.py [--out profiles/als_implicit_timing.json] [--reps 5] [--cases b64 b256 a]

The protocol of tools/als_cg_timing.py: every case runs in a child process of its own under its own time limit; after a child that
fails, is killed or runs out of time nothing more is started.  After a warm-up call, median of `reps` device-timed repetitions,
every one from the same factors, profiler off, all samples kept.  Cases:
  b64 / b256   C5's pattern as bench.py defines it, 1e6 x 1e5, 100 entries per row, uniform columns, k = 64 / 256
  a            65536 rows x 1024 uniformly drawn entries over 65536 columns, k = 256
The confidences are 1 + a count in 1 .. 4, the targets 1.  Per route (als: exact, cg6):
  <route>_c0_0_kernel_ms / <route>_c0_1_kernel_ms    every kernel class of the one-factor step added up (with a background: the Gram
                                                     of V and the kernel that scales it included); *_all: every repetition;
                                                     *_classes_ms: the classes of the last one
  <route>_bg_over_plain                              ratio of the medians
  <route>_c0_0_spread                                (max - min) / median of the repetitions without a background
  cg6_bg_over_als_bg                                 the CG sweep against the exact sweep, both with a background
The exact route adds two small launches and the read of S in the finish kernel: als_bg_over_plain is expected within 1.10 (the
margin covers the spread of the repetitions; als_within_1_10 records it).  The CG route streams S (k_pad^2 floats) from L2 once per
row and pass: its ratio is recorded whatever it is.
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
from kl_timing import _csr_matrix  # noqa: E402  (the same C5 pattern)

U_BIT = 1
CG_STEPS = 6
CASES = ("b64", "b256", "a")
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
        m, d, p, k, npr = 1000000, 100000, 64, int(case[1:]), 100
        Xs = _csr_matrix("c5", m, d, npr)
        indptr, indices = Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32)
        del Xs
        scale = (npr / d / k) ** 0.5
    print("case %s: pattern ready" % case, flush=True)
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    nnz = indices.size
    ctx.set_weighted_csr(0, indptr, indices, np.ones(nnz), 1.0 + np.random.default_rng(3).integers(1, 5, size=nnz))
    del indices
    ctx.fill_data_synthetic(1, 43)
    print("case %s: bound" % case, flush=True)

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    rec = {"case": case, "m": m, "d": d, "p": p, "k": k, "k_pad": ctx.geometry()[3], "entries_per_row": npr, "nnz": int(nnz), "reps": reps, "l2": l2,
           "nn_mask": 0, "cg_steps": CG_STEPS, "confidences": "1 + a count in 1 .. 4", "sweep": "U"}
    routes = (("als", lambda: ctx.als_step(l2, 0, U_BIT)), ("cg%d" % CG_STEPS, lambda: ctx.als_cg_step(l2, 0, U_BIT, CG_STEPS, 0)))
    for c0 in (0.0, 1.0):
        ctx.set_background_weight(0, c0)
        assert ctx.get_background_weight(0) == c0
        for name, call in routes:
            med, every, classes = _timed(ctx, lib, reps, reset, call)
            tag = "%s_c0_%d_" % (name, int(c0))
            rec.update({tag + "kernel_ms": med, tag + "kernel_ms_all": every, tag + "kernel_classes_ms": classes})
            print("  %s c0 = %g: kernels %.2f ms %s" % (name, c0, med, ["%.2f" % v for v in every]), flush=True)
    for name, _ in routes:
        plain, bg = rec[name + "_c0_0_kernel_ms"], rec[name + "_c0_1_kernel_ms"]
        every = rec[name + "_c0_0_kernel_ms_all"]
        rec[name + "_bg_over_plain"] = bg / plain
        rec[name + "_c0_0_spread"] = (max(every) - min(every)) / plain
    rec["als_within_1_10"] = bool(rec["als_bg_over_plain"] <= 1.10)
    rec["cg%d_bg_over_als_bg" % CG_STEPS] = rec["cg%d_c0_1_kernel_ms" % CG_STEPS] / rec["als_c0_1_kernel_ms"]
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_implicit_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case, in this process; the record goes to the file --out names
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_implicit_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    out = {"what": "U sweep of cmf_als_step and of cmf_als_cg_step (6 steps) with a background weight c0 = 1 against the same sweep with c0 = 0, "
                   "same process, pattern, weights and factors, nn_mask = 0; medians of device-timed repetitions, every repetition from the same "
                   "factors",
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
            raise SystemExit("als_implicit_timing: case %s ran out of its %d s; nothing more is started" % (case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_implicit_timing: case %s ended with status %d; nothing more is started" % (case, status))
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
