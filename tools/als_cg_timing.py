"""Time of the conjugate-gradient row solve of the ALS solver (als_cg_kernel, cmf_als_cg_step) beside the sweep of cmf_als_step that
it replaces (normal equations + Cholesky solves), in the same process, on the same pattern and factors, nn_mask = 0.

    python tools/als_cg_timing.py [--out profiles/als_cg_timing.json] [--reps 5] [--cases a b64 b256 bz64 bz256] [--steps 6 2 8]

Every case runs in a child process of its own under its own time limit; after a child that fails, is killed or runs out of time
nothing more is started.  After a warm-up call, median of `reps` device-timed repetitions, every one from the same factors,
profiler off, all samples kept.  Cases:
  a       case 1 of tools/als_timing.py: 65536 rows x 1024 uniformly drawn entries over 65536 columns, k = 256            (U sweep)
  b64 / b256     C5's pattern as bench.py defines it, 1e6 x 1e5, 100 entries per row, uniform columns, k = 64 / 256       (U sweep;
                 at k = 256 also with "als_cg_lds" = 0, every row gathers again in every pass, and with all of the LDS allowed)
  bz64 / bz256   the same with Zipf(1.1) columns                                        (U sweep, and the V sweep: its long rows)
Per sweep:
  als_kernel_ms            every kernel class of a one-factor cmf_als_step added up (rowhess: the normal equations, elementwise: the
                           finish and apply kernels, eigen: the Cholesky solves); als_kernel_classes_ms lists them
  cg<n>_kernel_ms          every kernel class of the same one-factor cmf_als_cg_step with n steps (rowhess: als_cg_kernel; the V
                           sweep also forms S and N of its full side)
  cg<n>_over_als           their ratio (the aim for the documented count on b256: <= 1)
  *_wall_ms                wall time of the same calls, timing off (host planning and the indptr read-back included)
Fails without a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kl_timing import _csr_matrix, _wall  # noqa: E402  (the same protocol and the same C5 patterns)

U_BIT, V_BIT = 1, 2
DOCUMENTED_STEPS = 6
CASES = ("a", "b64", "b256", "bz64", "bz256")
CHILD_LIMIT_S = 420


def _timed(ctx, lib, reps, reset, call):
    """median over reps of the kernel ms of all classes for one `call` after `reset`; every sample; the classes of the last one."""
    names = list(lib.KERNEL_CLASSES) + list(lib.LATER_KERNEL_CLASSES)
    reset()
    call()                                                  # warm-up (sizes every workspace)
    ctx.kernel_timing(True)
    out, classes = [], {}
    for _ in range(reps):
        reset()
        ctx.sync()
        ctx.kernel_timing_reset()
        call()
        classes = {n: ctx.kernel_time(n)[0] for n in names if ctx.kernel_time(n)[1]}
        out.append(sum(classes.values()))
    ctx.kernel_timing(False)
    return statistics.median(out), out, classes


def _sweep(ctx, lib, reps, reset, l2, mask, steps_list, tag, rec):
    a, a_all, classes = _timed(ctx, lib, reps, reset, lambda: ctx.als_step(l2, 0, mask))
    reset()
    w, w_all = _wall(ctx, reps, lambda: ctx.als_step(l2, 0, mask))
    rec.update({tag + "als_kernel_ms": a, tag + "als_kernel_ms_all": a_all, tag + "als_kernel_classes_ms": classes,
                tag + "als_wall_ms": w, tag + "als_wall_ms_all": w_all})
    print("  %sals: kernels %.2f ms, wall %.2f ms" % (tag, a, w), flush=True)
    for n in steps_list:
        b, b_all, cl = _timed(ctx, lib, reps, reset, lambda: ctx.als_cg_step(l2, 0, mask, n, 0))
        reset()
        w2, w2_all = _wall(ctx, reps, lambda: ctx.als_cg_step(l2, 0, mask, n, 0))
        rec.update({"%scg%d_kernel_ms" % (tag, n): b, "%scg%d_kernel_ms_all" % (tag, n): b_all, "%scg%d_over_als" % (tag, n): b / a,
                    "%scg%d_kernel_classes_ms" % (tag, n): cl,
                    "%scg%d_wall_ms" % (tag, n): w2, "%scg%d_wall_ms_all" % (tag, n): w2_all, "%scg%d_wall_over_als" % (tag, n): w2 / w})
        print("  %scg %d steps: kernel %.2f ms (%.3f of als), wall %.2f ms" % (tag, n, b, b / a, w2), flush=True)


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
           "nn_mask": 0, "documented_steps": DOCUMENTED_STEPS, "steps": list(steps_list),
           "gathered_bytes_per_pass_u": int(nnz) * ctx.geometry()[3] * 4}
    _sweep(ctx, lib, reps, reset, l2, U_BIT, steps_list, "u_", rec)
    if case == "b256":                                      # the same sweep with nothing resident in LDS, and with all of it allowed
        for name, lds in (("streamed", 0), ("all_lds", 1 << 20)):
            ctx.set_option("als_cg_lds", lds)
            b, b_all, _ = _timed(ctx, lib, reps, reset, lambda: ctx.als_cg_step(l2, 0, U_BIT, DOCUMENTED_STEPS, 0))
            ctx.set_option("als_cg_lds", -1)
            rec.update({"u_cg%d_%s_kernel_ms" % (DOCUMENTED_STEPS, name): b, "u_cg%d_%s_kernel_ms_all" % (DOCUMENTED_STEPS, name): b_all,
                        "u_%s_over_default" % name: b / rec["u_cg%d_kernel_ms" % DOCUMENTED_STEPS]})
            print("  u_cg %d steps, als_cg_lds = %d: kernel %.2f ms" % (DOCUMENTED_STEPS, lds, b), flush=True)
    if case.startswith("bz"):                               # the V sweep: the hot columns are rows of up to ~m entries, one workgroup each
        rec["v_row_entries_max_median"] = [int(col_len.max()), float(np.median(col_len))]
        _sweep(ctx, lib, reps, reset, l2, V_BIT, steps_list, "v_", rec)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_cg_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--steps", nargs="*", type=int, default=[DOCUMENTED_STEPS, 2, 8])
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case, in this process; the record goes to the file --out names
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_cg_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps, a.steps)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    out = {"what": "U (and V) sweep of cmf_als_cg_step against the same sweep of cmf_als_step (normal equations + Cholesky solves), same "
                   "process, pattern and factors, nn_mask = 0; medians of device-timed repetitions, every repetition from the same factors",
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
            raise SystemExit("als_cg_timing: case %s ran out of its %d s; nothing more is started" % (case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_cg_timing: case %s ended with status %d; nothing more is started" % (case, status))
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
