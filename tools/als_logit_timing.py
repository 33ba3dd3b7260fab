"""Time of the logistic normal-equation pass (als_normal_kernel<KP, true>) beside the Frobenius pass (als_normal_kernel<KP, false>) over
the same pattern, in the same process.

    python tools/als_logit_timing.py [--out profiles/als_logit_timing.json] [--reps 5] [--cases case1 c5] [--csr-rows N]
                                     [--csr-k 256 64] [--case1-rows M]

The protocol of tools/als_timing.py: after a warm-up call, median of `reps` device-timed repetitions, profiler off.  What is timed
is class "rowhess" of a U-only cmf_als_step -- the normal-equation kernel over all rows (one launch per chunk of rows), not the
solves -- once with X Frobenius and once with X logistic (cmf_set_relation_loss); the factors are put back before every call, so
both passes gather the same rows and the scores of the logistic pass do not drift.  Beside it the wall time of the whole U-only
step (piece plan, uploads, normal equations, solves), timing off.
case1: 65536 rows x 1024 uniformly drawn stored entries per row over d = 65536 columns, k = 256.
c5:    C5's pattern as bench.py defines it (1e6 x 1e5, 100 stored entries per row, uniform columns), k = 256 and k = 64.
Targets 0 / 1, weights 1.  Added work per gathered row: k FMAs, a lane reduction and one tanh against 2 k^2 matrix-pipe flops; the
expectation at k = 256 is a ratio within 1.10, at k = 64 it is recorded without a target.
Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from kl_timing import _csr_matrix, PEAK_TF  # noqa: E402  (the same C5 pattern)

U_BIT = 1


def _timed_reset(ctx, reps, reset, call, cls):
    """_timed of kl_timing.py with the factors put back before every call."""
    reset()
    call()                                                  # warm-up (sizes every workspace)
    ctx.kernel_timing(True)
    out, launches = [], 0
    for _ in range(reps):
        reset()
        ctx.kernel_timing_reset()
        call()
        ms, launches, _ = ctx.kernel_time(cls)
        out.append(ms)
    ctx.kernel_timing(False)
    return statistics.median(out), out, launches


def _wall_reset(ctx, reps, reset, call):
    """_wall of kl_timing.py with the factors put back before every call: wall time of the whole call, timing off."""
    out = []
    for _ in range(reps):
        reset()
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def measure(lib, case, reps, m, d, k, per_row, indptr, indices, scale):
    l2 = 0.1
    ctx = lib.Context(0)
    ctx.set_problem(m, d, 64, k)
    rng = np.random.default_rng(3)
    nnz = indices.size
    ctx.set_weighted_csr(0, indptr, indices, (rng.random(nnz) < 0.5).astype(np.float64), np.ones(nnz))

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    rec = {"case": case, "m": m, "d": d, "k": k, "entries_per_row": per_row, "nnz": float(nnz), "reps": reps, "l2": l2,
           "fp32_mfma_peak_tflops": PEAK_TF, "als_layout_piece_U_V_Z": list(ctx.als_layout())}
    for name, kind in (("frobenius", "frobenius"), ("logistic", "logistic"), ("frobenius_again", "frobenius")):
        ctx.set_relation_loss(0, kind)
        ms, ms_all, n = _timed_reset(ctx, reps, reset, lambda: ctx.als_step(l2, 0, U_BIT), "rowhess")
        flops = 2.0 * nnz * k * k + (2.0 * nnz * k if kind == "logistic" else 0.0)
        rec[name + "_u_pass_kernel_ms"], rec[name + "_u_pass_kernel_ms_all"], rec[name + "_u_pass_launches"] = ms, ms_all, n
        rec[name + "_u_pass_tflops"] = flops / ms * 1e-9
        rec[name + "_u_step_wall_ms"], rec[name + "_u_step_wall_ms_all"] = _wall_reset(ctx, reps, reset, lambda: ctx.als_step(l2, 0, U_BIT))
    rec["logistic_over_frobenius"] = rec["logistic_u_pass_kernel_ms"] / rec["frobenius_u_pass_kernel_ms"]
    if k == 256:
        rec["within_1_10_expectation"] = bool(rec["logistic_over_frobenius"] <= 1.10)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_logit_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=["case1", "c5"])
    ap.add_argument("--csr-rows", type=int, default=1000000)
    ap.add_argument("--csr-k", nargs="*", type=int, default=[256, 64])
    ap.add_argument("--case1-rows", type=int, default=65536)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("als_logit_timing: no GPU visible (needs an MI355X)")
    out = {"what": "logistic normal-equation pass (als_normal_kernel<KP, true>) against the Frobenius pass (als_normal_kernel<KP, false>) over the same "
                   "pattern, U sweep, class rowhess; medians of device-timed repetitions", "cases": []}
    if os.path.exists(a.out):                                # cases measured by an earlier call stay (one case per call fits a time limit)
        with open(a.out) as f:
            old = json.load(f)
        redo = {c if c == "case1" or a.csr_rows == 1000000 else "%s_%drows" % (c, a.csr_rows) for c in a.cases}
        out["cases"] = [r for r in old.get("cases", []) if r.get("case") not in redo]
        out.update({key: v for key, v in old.items() if key not in out})      # (records other runs left beside the cases stay too)
    for case in a.cases:
        if case == "case1":
            m, d, per_row = a.case1_rows, 65536, 1024
            indices = np.random.default_rng(42).integers(0, d, size=m * per_row, dtype=np.int32)
            indptr = np.arange(0, m * per_row + 1, per_row, dtype=np.int64)
            recs = [measure(_lib, case, a.reps, m, d, 256, per_row, indptr, indices, (0.7979 / 256) ** 0.5)]
        else:
            m, d, per_row = a.csr_rows, 100000, 100
            Xs = _csr_matrix("c5", m, d, per_row)
            indptr, indices = Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32)
            del Xs
            name = case if m == 1000000 else "%s_%drows" % (case, m)      # (a part of the pattern is a case of its own)
            recs = [measure(_lib, name, a.reps, m, d, k, per_row, indptr, indices, (per_row / d / k) ** 0.5) for k in a.csr_k]
        for rec in recs:
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
