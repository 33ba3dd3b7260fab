"""Time of the ALS normal-equation pass beside the per-row Hessian kernel of the Newton sweeps, and of an ALS iteration beside a
weighted MU iteration.

    python tools/als_timing.py [--out profiles/als_timing.json] [--reps 5] [--cases case1 c5 c5z] [--csr-rows N] [--csr-k 64 256]
                                [--case1-rows M]

After a warm-up call, median of `reps` device-timed repetitions, profiler off.
case1: 65536 rows x 1024 uniformly drawn stored entries per row over d = 65536 columns, p = 256, k = 256, Y dense and unweighted.
  (a) als_u_pass_kernel_ms      class "rowhess" of a U-only cmf_als_step: als_normal_kernel over all rows (one launch per chunk of
                                rows), 2 nnz k^2 flops, TF/s and share of the 157.3 TF/s fp32-MFMA figure
  (b) rowhess_u_pass_kernel_ms  the unchanged row_hess_kernel on the same context: class "rowhess" of the U sweep of
                                cmf_newton_step_device_sampled with a logit x link (the per-row kernel, not the class path) and
                                sg_sample_ratio = 1024 / d -- the same 1024 gathered rows per output row; X dense sigmoid(N(0,1))
  (c) als_step_wall_ms beside wmu_step_wall_ms: a whole ALS iteration and a whole weighted MU iteration on the same pattern
      (wall time of single steps, timing off), and every kernel class of the ALS iteration
c5 / c5z: C5's pattern as bench.py defines it (1e6 x 1e5, 100 stored entries per row, uniform / Zipf(1.1) columns), k = 64 and
256: the U-side normal-equation pass alone (class "rowhess" of a U-only step) with its TF/s.
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

from kl_timing import _csr_matrix, _timed, _wall, PEAK_TF  # noqa: E402  (the same protocol and the same C5 patterns)

U_BIT, V_BIT, Z_BIT = 1, 2, 4


def _bind_pattern(ctx, indptr, indices, seed):
    rng = np.random.default_rng(seed)
    nnz = indices.size
    ctx.set_weighted_csr(0, indptr, indices, rng.random(nnz) + 0.5, np.ones(nnz))


def _pass(ctx, reps, l2, nnz, k):
    a, a_all, n = _timed(ctx, reps, lambda: ctx.als_step(l2, 0, U_BIT), ["rowhess"])
    flops = 2.0 * nnz * k * k
    return {"als_u_pass_kernel_ms": a, "als_u_pass_kernel_ms_all": a_all, "als_u_pass_launches": n, "flops_2nnzk2": flops,
            "als_u_pass_tflops": flops / a * 1e-9, "als_u_pass_share_of_fp32_mfma_peak": flops / a * 1e-9 / PEAK_TF}


def measure_case1(lib, reps, m=65536, d=65536, per_row=1024, p=256, k=256):
    l2 = 0.1
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    rng = np.random.default_rng(42)
    indices = rng.integers(0, d, size=m * per_row, dtype=np.int32)
    indptr = np.arange(0, m * per_row + 1, per_row, dtype=np.int64)
    _bind_pattern(ctx, indptr, indices, 1)
    del indices
    ctx.fill_data_synthetic(0, 42, kind=1)                 # X dense, sigmoid(N(0,1)): what the Newton comparison reads
    ctx.fill_data_synthetic(1, 43)
    scale = (0.7979 / k) ** 0.5

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    reset()
    nnz = float(m) * per_row
    rec = {"case": "case1", "m": m, "d": d, "p": p, "k": k, "entries_per_row": per_row, "nnz": nnz, "reps": reps, "l2": l2,
           "fp32_mfma_peak_tflops": PEAK_TF, "als_layout_piece_U_V_Z": list(ctx.als_layout())}
    rec.update(_pass(ctx, reps, l2, nnz, k))
    reset()
    ratio = per_row / d
    seed = [0]

    def newton_u():
        seed[0] += 1
        ctx.newton_step_device_sampled(0.5, 0.0, l2, "logit", "linear", 0, U_BIT, 0.2, ratio, seed[0])
    b, b_all, nb = _timed(ctx, reps, newton_u, ["rowhess"])
    rec.update({"rowhess_u_pass_kernel_ms": b, "rowhess_u_pass_kernel_ms_all": b_all, "rowhess_u_pass_launches": nb,
                "rowhess_samples_per_row": int(d * ratio), "als_over_rowhess": rec["als_u_pass_kernel_ms"] / b,
                "within_25_percent_aim": bool(rec["als_u_pass_kernel_ms"] <= 1.25 * b)})
    reset()
    ctx.kernel_timing(True)
    ctx.kernel_timing_reset()
    ctx.als_step(l2, 0, 7)
    names = list(lib.KERNEL_CLASSES) + list(lib.LATER_KERNEL_CLASSES)
    rec["als_step_kernel_classes_ms"] = {n: ctx.kernel_time(n)[0] for n in names if ctx.kernel_time(n)[1]}
    ctx.kernel_timing(False)
    reset()
    w, w_all = _wall(ctx, reps, lambda: ctx.als_step(l2, 0, 7))
    rec["als_step_wall_ms"], rec["als_step_wall_ms_all"] = w, w_all
    reset()
    w2, w2_all = _wall(ctx, reps, lambda: ctx.mu_weighted_step(0.0, l2, 7))
    rec["wmu_step_wall_ms"], rec["wmu_step_wall_ms_all"] = w2, w2_all
    rec["als_over_wmu_step"] = w / w2
    ctx.close()
    return rec


def measure_csr(lib, kind, reps, rows, k):
    m, d, p, npr, l2 = rows, 100000, 64, 100, 0.1
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    Xs = _csr_matrix("c5z" if kind == "c5z" else "c5", m, d, npr)
    _bind_pattern(ctx, Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32), 2)
    del Xs
    ctx.fill_data_synthetic(1, 43)
    scale = (npr / d / k) ** 0.5
    for w, seed in ((0, 101), (1, 102), (2, 103)):
        ctx.fill_factor_synthetic(w, seed, 0, scale)
    nnz = float(m) * npr
    rec = {"case": kind, "m": m, "d": d, "p": p, "k": k, "entries_per_row": npr, "nnz": nnz, "reps": reps, "l2": l2,
           "fp32_mfma_peak_tflops": PEAK_TF, "als_layout_piece_U_V_Z": list(ctx.als_layout())}
    rec.update(_pass(ctx, reps, l2, nnz, k))
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=["case1", "c5", "c5z"])
    ap.add_argument("--csr-rows", type=int, default=1000000)
    ap.add_argument("--csr-k", nargs="*", type=int, default=[64, 256])
    ap.add_argument("--case1-rows", type=int, default=65536)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("als_timing: no GPU visible (needs an MI355X)")
    out = {"what": "ALS normal-equation pass against row_hess_kernel for the same gathered rows, ALS iteration against a weighted MU "
                   "iteration; medians of device-timed repetitions", "cases": []}
    if os.path.exists(a.out):                                # cases measured by an earlier call stay (one case per call fits a time limit)
        with open(a.out) as f:
            old = json.load(f)
        out["cases"] = [r for r in old.get("cases", []) if r.get("case") not in a.cases]
    for case in a.cases:
        recs = [measure_case1(_lib, a.reps, m=a.case1_rows)] if case == "case1" else [measure_csr(_lib, case, a.reps, a.csr_rows, k) for k in a.csr_k]
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
