"""Time of the logistic reweighting pass of the ALS solver (als_logit_pass_kernel) beside the Huber pass of the same build over the
same pattern, and of the U sweep on a logistic X: fused exact (the flag off) against the pass in front of every route.

    python tools/als_logit_pass_timing.py [--out profiles/als_logit_pass_timing.json] [--reps 5] [--cases a b64 b256] [--fused-only]

The protocol and the cases of tools/als_huber_timing.py: every case runs in a child process of its own under its own time limit;
after a child that fails, is killed or runs out of time nothing more is started.  After a warm-up call, median of `reps`
device-timed repetitions, every one from the same factors, profiler off, all samples kept.  Cases:
  a       65536 rows x 1024 uniformly drawn entries over 65536 columns, k = 256
  b64 / b256     C5's pattern as bench.py defines it, 1e6 x 1e5, 100 entries per row, uniform columns, k = 64 / 256
Per case, in this order:
  fused_exact_kernel_ms     cmf_als_step on the logistic X with the flag off: every kernel class added up (the default route)
  huber_pass_ms             the class of the pass (klmu) in cmf_als_cg_step under delta = 1 on the same pattern, Frobenius
  pass_exact / pass_cg6 / pass_nncg3 / pass_dual   the flag on: cmf_als_step, cmf_als_cg_step (6 steps), cmf_als_nncg_step (U
                            non-negative, 3 projected steps), cmf_als_dual_step (dual_max = 128)
      <route>_kernel_ms         every kernel class of the one-factor step, the pass included
      <route>_pass_ms           the class of the pass (klmu) in that step
      <route>_over_fused_exact  <route>_kernel_ms / fused_exact_kernel_ms
  logit_pass_ms             pass_cg6_pass_ms, every sample kept; logit_over_huber_pass: its ratio to huber_pass_ms
  pass_bytes_model          nnz (4 k_pad + 12): what the pass moves, from the code
--fused-only measures fused_exact_kernel_ms alone through entry points older than the flag: the same file runs against a build of
an earlier commit, in the same session, to show that the default route kept its time.
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

from als_cg_timing import _timed  # noqa: E402  (the same protocol)
from kl_timing import _csr_matrix  # noqa: E402  (the same C5 pattern)

U_BIT = 1
CASES = ("a", "b64", "b256")
CHILD_LIMIT_S = 420
DELTA = 1.0


def _timed_class(ctx, lib, reps, reset, call, name):
    """``_timed``, and the kernel ms of class ``name`` in every repetition: (median of all classes, its samples, median of the
    class, its samples, the classes of the last repetition)."""
    names = list(lib.KERNEL_CLASSES) + list(lib.LATER_KERNEL_CLASSES)
    reset()
    call()                                                  # warm-up (sizes every workspace, builds the arrays of the pass)
    ctx.kernel_timing(True)
    total, part, classes = [], [], {}
    for _ in range(reps):
        reset()
        ctx.sync()
        ctx.kernel_timing_reset()
        call()
        classes = {n: ctx.kernel_time(n)[0] for n in names if ctx.kernel_time(n)[1]}
        total.append(sum(classes.values()))
        part.append(classes.get(name, 0.0))
    ctx.kernel_timing(False)
    return statistics.median(total), total, statistics.median(part), part, classes


def measure(lib, case, reps, fused_only):
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
    labels = (np.random.default_rng(1 if case == "a" else 2).random(nnz) < 0.5).astype(np.float64)
    ctx.set_weighted_csr(0, indptr, indices, labels, np.ones(nnz))
    del indices, labels
    ctx.fill_data_synthetic(1, 43)
    print("case %s: bound" % case, flush=True)

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    kp = ctx.geometry()[3]
    rec = {"case": case, "m": m, "d": d, "p": p, "k": k, "k_pad": kp, "entries_per_row": npr, "nnz": int(nnz), "reps": reps, "l2": l2,
           "pass_bytes_model": int(nnz) * (4 * kp + 12), "huber_pass_bytes_model": int(nnz) * (4 * kp + 24)}
    ctx.set_relation_loss(0, "logistic")
    f, f_all, classes = _timed(ctx, lib, reps, reset, lambda: ctx.als_step(l2, 0, U_BIT))
    rec.update({"fused_exact_kernel_ms": f, "fused_exact_kernel_ms_all": f_all, "fused_exact_kernel_classes_ms": classes})
    print("  fused exact: %.2f ms (%s)" % (f, " ".join("%.2f" % v for v in f_all)), flush=True)
    if fused_only:
        ctx.close()
        return rec
    ctx.set_relation_loss(0, "frobenius")
    ctx.set_huber_delta(0, DELTA)
    _, _, h, h_all, _ = _timed_class(ctx, lib, reps, reset, lambda: ctx.als_cg_step(l2, 0, U_BIT, 6, 0), "klmu")
    ctx.set_huber_delta(0, 0)
    rec.update({"huber_pass_ms": h, "huber_pass_ms_all": h_all})
    print("  Huber pass: %.2f ms (%s)" % (h, " ".join("%.2f" % v for v in h_all)), flush=True)
    ctx.set_relation_loss(0, "logistic")
    ctx.set_logit_pass(0, True)
    routes = (("pass_exact", lambda: ctx.als_step(l2, 0, U_BIT)), ("pass_cg6", lambda: ctx.als_cg_step(l2, 0, U_BIT, 6, 0)),
              ("pass_nncg3", lambda: ctx.als_nncg_step(l2, U_BIT, U_BIT, 0, 3, 0)), ("pass_dual", lambda: ctx.als_dual_step(l2, 0, U_BIT, 128)))
    for name, call in routes:
        t, t_all, ps, ps_all, classes = _timed_class(ctx, lib, reps, reset, call, "klmu")
        rec.update({name + "_kernel_ms": t, name + "_kernel_ms_all": t_all, name + "_kernel_classes_ms": classes, name + "_pass_ms": ps,
                    name + "_pass_ms_all": ps_all, name + "_over_fused_exact": t / f})
        print("  %s: %.2f ms (pass %.2f ms), %.3f of fused exact" % (name, t, ps, t / f), flush=True)
    rec.update({"logit_pass_ms": rec["pass_cg6_pass_ms"], "logit_pass_ms_all": rec["pass_cg6_pass_ms_all"],
                "logit_over_huber_pass": rec["pass_cg6_pass_ms"] / h,
                "pass_gb_per_s_model": rec["pass_bytes_model"] / (rec["pass_cg6_pass_ms"] * 1e-3) / 1e9,
                "huber_pass_gb_per_s_model": rec["huber_pass_bytes_model"] / (h * 1e-3) / 1e9})
    print("  logistic pass %.2f ms, Huber pass %.2f ms: ratio %.3f" % (rec["logit_pass_ms"], h, rec["logit_over_huber_pass"]), flush=True)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_logit_pass_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case, in this process; the record goes to the file --out names
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_logit_pass_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps, a.fused_only)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    out = {"what": "the logistic reweighting pass beside the Huber pass of the same build, and the U sweep on a logistic X: fused exact "
                   "(flag off) against the pass in front of the exact, CG, projected-CG and dual rows; same process, pattern and "
                   "factors per case; medians of device-timed repetitions, every repetition from the same factors",
           "cases": []}
    if os.path.exists(a.out):                                # cases measured by an earlier call stay
        with open(a.out) as f:
            out["cases"] = [r for r in json.load(f).get("cases", []) if r.get("case") not in a.cases]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in a.cases:
        part = a.out + "." + case + ".part"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--out", part, "--reps", str(a.reps)] + (["--fused-only"] if a.fused_only else [])
        try:
            status = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("als_logit_pass_timing: case %s ran out of its %d s; nothing more is started" % (case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_logit_pass_timing: case %s ended with status %d; nothing more is started" % (case, status))
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
