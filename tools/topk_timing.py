"""Time of the top-n prediction call beside the parent's own pass over the same f(U V^T) tiles.

    python tools/topk_timing.py [--out profiles/topk_timing.json] [--reps 5] [--shapes 65536,256 16384,128]

For every shape (m = d, k) and n in {10, 100}, all rows in one call, after a warm-up call, median of `reps` device-timed
repetitions, profiler off:
  (a) topk_kernel_ms      kernel time of the call (class "topk": scan + merge kernels, device events)
  (b) nt_error_kernel_ms  the x-side NT error kernel (class "gemm_nt" of one residual_sq) on the same context and factors with
                          synthetic X: the same 2 m d k flops on the same fp32 matrix pipe, which also streams X and
                          materialises nothing.  p = 256, so the y side of that call adds d p / (m d) = 256 / m of its flops
                          (0.39 % at m = 65536, 1.6 % at m = 16384); it is included in (b) and said so in the record.
  (c) topk_wall_ms        end-to-end wall time of Context.topk (scratch, launches, the nq x n read-back), timing off
Rates: algorithmic TFLOP/s = 2 m d k / kernel time; share of the 157.3 TF/s fp32-MFMA peak.  Fails without a GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TF = 157.3


def measure(lib, m, k, ns, reps):
    d, p = m, 256
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    ctx.fill_data_synthetic(0, 42)
    ctx.fill_data_synthetic(1, 43)
    scale = (0.7979 / k) ** 0.5
    for w, seed in ((0, 101), (1, 102), (2, 103)):
        ctx.fill_factor_synthetic(w, seed, 0, scale)
    flops = 2.0 * m * d * k
    rec = {"m": m, "d": d, "p": p, "k": k, "flops_2mdk": flops, "reps": reps, "fp32_mfma_peak_tflops": PEAK_TF,
           "nt_note": "gemm_nt of one residual_sq: x side (2 m d k) plus the y side (2 d p k = %.2f %% of it)" % (100.0 * p / m)}
    ctx.residual_sq()                                   # warm-up
    ctx.kernel_timing(True)
    nt = []
    for _ in range(reps):
        ctx.kernel_timing_reset()
        ctx.residual_sq()
        nt.append(ctx.kernel_time("gemm_nt")[0])
    rec["nt_error_kernel_ms"] = statistics.median(nt)
    rec["nt_error_kernel_ms_all"] = nt
    rec["nt_error_tflops"] = flops * (1.0 + p / m) / rec["nt_error_kernel_ms"] * 1e-9
    ctx.kernel_timing(False)
    for n in ns:
        ctx.topk(lib.CMF_U, lib.CMF_V, n)               # warm-up
        ctx.kernel_timing(True)
        ks = []
        for _ in range(reps):
            ctx.kernel_timing_reset()
            ctx.topk(lib.CMF_U, lib.CMF_V, n)
            ks.append(ctx.kernel_time("topk")[0])
        ctx.kernel_timing(False)
        wall = []
        for _ in range(reps):
            ctx.sync()
            t0 = time.perf_counter()
            ctx.topk(lib.CMF_U, lib.CMF_V, n)
            wall.append((time.perf_counter() - t0) * 1e3)
        kms = statistics.median(ks)
        qb, split, chunk, scratch = ctx.topk_layout(m, lib.CMF_V, n)
        rec["n%d" % n] = {
            "topk_kernel_ms": kms, "topk_kernel_ms_all": ks,
            "topk_algorithmic_tflops": flops / kms * 1e-9,
            "topk_share_of_fp32_mfma_peak": flops / kms * 1e-9 / PEAK_TF,
            "topk_over_nt_error_kernel": kms / rec["nt_error_kernel_ms"],
            "within_25_percent_allowance": bool(kms <= 1.25 * rec["nt_error_kernel_ms"]),
            "topk_wall_ms": statistics.median(wall), "topk_wall_ms_all": wall,
            "candidate_shares": split, "queries_per_launch": chunk, "scratch_bytes": scratch,
            "scratch_share_of_dense_product": scratch / (4.0 * m * d),
        }
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["65536,256", "16384,128"])
    ap.add_argument("--n", nargs="*", type=int, default=[10, 100])
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("topk_timing: no GPU visible (needs an MI355X)")
    out = {"what": "top-n prediction (all rows, one call) against the x-side NT error kernel; medians of device-timed repetitions",
           "shapes": []}
    for s in a.shapes:
        m, k = (int(v) for v in s.split(","))
        rec = measure(_lib, m, k, a.n, a.reps)
        out["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
