"""Time of the Huber reweighting pass of the ALS solver (als_huber_pass_kernel) and of the U sweep with and without a delta on X, in
the same process, on the same pattern and factors, beside als_logit_loss_kernel of the same build over the same pattern -- the
nearest existing pass over the same bytes.

    python tools/als_huber_timing.py [--out profiles/als_huber_timing.json] [--reps 5] [--cases a b64 b256]

The protocol and the cases of tools/als_cg_timing.py: every case runs in a child process of its own under its own time limit; after a
child that fails, is killed or runs out of time nothing more is started.  After a warm-up call, median of `reps` device-timed
repetitions, every one from the same factors, profiler off, all samples kept.  Cases:
  a       65536 rows x 1024 uniformly drawn entries over 65536 columns, k = 256
  b64 / b256     C5's pattern as bench.py defines it, 1e6 x 1e5, 100 entries per row, uniform columns, k = 64 / 256
Per case, for the routes exact (cmf_als_step), cg6 (cmf_als_cg_step, 6 steps), nncg3 (cmf_als_nncg_step, U non-negative, 3 projected
steps) and dual (cmf_als_dual_step, dual_max = 128; at k_pad = 64 no class is below k_pad and its rows are the exact ones):
  <route>_kernel_ms         every kernel class of the one-factor step without a delta, added up
  <route>_huber_kernel_ms   the same step under delta = 1: the same launches behind one reweighting pass
  <route>_pass_ms           the class of the pass (klmu) in that step: the pass alone
  <route>_pass_share        pass / (step under the delta)
and once:
  logit_loss_kernel_ms      als_logit_loss_kernel + its sum over the same pattern (cmf_als_logistic_loss)
  huber_loss_kernel_ms      the LOSS form of the pass (cmf_als_huber_loss)
  pass_bytes_model          nnz (4 k_pad + 24): what the pass moves, from the code
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
CASES = ("a", "b64", "b256")
CHILD_LIMIT_S = 420
DELTA = 1.0


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
    # targets in 0.5 .. 1.5 against scores near 0: about half of the residuals exceed delta = 1 (the time does not depend on it)
    ctx.set_weighted_csr(0, indptr, indices, np.random.default_rng(1 if case == "a" else 2).random(nnz) + 0.5, np.ones(nnz))
    del indices
    ctx.fill_data_synthetic(1, 43)
    print("case %s: bound" % case, flush=True)

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    kp = ctx.geometry()[3]
    rec = {"case": case, "m": m, "d": d, "p": p, "k": k, "k_pad": kp, "entries_per_row": npr, "nnz": int(nnz), "reps": reps, "l2": l2,
           "delta": DELTA, "pass_bytes_model": int(nnz) * (4 * kp + 24)}
    routes = (("exact", lambda: ctx.als_step(l2, 0, U_BIT)), ("cg6", lambda: ctx.als_cg_step(l2, 0, U_BIT, 6, 0)),
              ("nncg3", lambda: ctx.als_nncg_step(l2, U_BIT, U_BIT, 0, 3, 0)), ("dual", lambda: ctx.als_dual_step(l2, 0, U_BIT, 128)))
    for name, call in routes:
        ctx.set_huber_delta(0, 0)
        a, a_all, _ = _timed(ctx, lib, reps, reset, call)
        ctx.set_huber_delta(0, DELTA)
        b, b_all, classes = _timed(ctx, lib, reps, reset, call)
        ps = classes.get("klmu", 0.0)
        rec.update({name + "_kernel_ms": a, name + "_kernel_ms_all": a_all, name + "_huber_kernel_ms": b, name + "_huber_kernel_ms_all": b_all,
                    name + "_huber_kernel_classes_ms": classes, name + "_pass_ms": ps, name + "_pass_share": ps / b,
                    name + "_huber_over_plain": b / a})
        print("  %s: %.2f ms without a delta, %.2f ms with (pass %.2f ms, %.3f of it)" % (name, a, b, ps, ps / b), flush=True)
    rec["pass_gb_per_s_model"] = rec["pass_bytes_model"] / (rec["cg6_pass_ms"] * 1e-3) / 1e9
    h, h_all, _ = _timed(ctx, lib, reps, reset, lambda: ctx.als_huber_loss(True, False))
    ctx.set_huber_delta(0, 0)
    ctx.set_relation_loss(0, "logistic")     # (the targets are not inspected; the kernel's time does not depend on them)
    g, g_all, _ = _timed(ctx, lib, reps, reset, lambda: ctx.als_logistic_loss(True, False))
    ctx.set_relation_loss(0, "frobenius")
    rec.update({"huber_loss_kernel_ms": h, "huber_loss_kernel_ms_all": h_all, "logit_loss_kernel_ms": g, "logit_loss_kernel_ms_all": g_all,
                "pass_over_logit_loss": rec["cg6_pass_ms"] / g})
    print("  loss form of the pass %.2f ms, als_logit_loss_kernel %.2f ms; the pass is %.3f of the latter" % (h, g, rec["pass_over_logit_loss"]),
          flush=True)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_huber_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case, in this process; the record goes to the file --out names
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_huber_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    out = {"what": "the Huber reweighting pass and the U sweep of every ALS row route with and without delta = 1 on X, same process, pattern "
                   "and factors; als_logit_loss_kernel over the same pattern beside them; medians of device-timed repetitions, every "
                   "repetition from the same factors",
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
            raise SystemExit("als_huber_timing: case %s ran out of its %d s; nothing more is started" % (case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_huber_timing: case %s ended with status %d; nothing more is started" % (case, status))
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
