"""Time of the weighted multiplicative-update passes beside the Kullback-Leibler quotient passes of the same shape.

    python tools/wmu_timing.py [--out profiles/wmu_timing.json] [--reps 5] [--shapes 65536,256 16384,128] [--csr c5] [--csr-rows N]

The weighted denominator pass (W .* (A B^T)) B is the quotient pass's kernel (pairpass_kernel) with w s in place of t / s: the same flops (4 m d k), the
same tiles, the same 4 bytes per cell streamed.  So the yardstick of every figure is the KL pass on the same context and factors.
Dense, for every shape (m = d, k), p = 256, synthetic |N(0,1)| data, a Bernoulli(0.3) mask as weights on X, after a warm-up call,
median and spread of `reps` device-timed repetitions, profiler off:
  kl_pass_kernel_ms        class "klmu" of a U-only cmf_mu_kl_step: one launch of pairpass_kernel<.., KlQuotient>
  wmu_den_kernel_ms        class "klmu" of a U-only cmf_mu_weighted_step: one launch of pairpass_kernel<.., WmDen>
  wmu_num_kernel_ms        class "gemm_nn" of the same step: the numerator pass P V (pairpass_kernel<.., WmNum>)
  wmu_den1_kernel_ms       the denominator pass of the unweighted relation of a weighted fit (W == 1 flag, no W loads)
  wmu_den_over_kl          ratio of the medians; aim: wmu median <= 1.05 x the slowest KL repetition
  step wall times          a full weighted step beside a full KL step and a full Frobenius step (timing off)
CSR: C5's shape as bench.py defines it (m = 1e6, d = 1e5, p = 64, k = 256, 100 stored entries per row, uniform columns): the
U-side and V-side passes over the pattern held as weights (cmf_set_weighted_csr, weight 1) beside the KL passes over the same
matrix held as native CSR data.  Both V-side figures hold the dense pass over Y as well.
Fails without a GPU.
"""
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

PEAK_TF = 157.3
U_BIT, V_BIT, Z_BIT = 1, 2, 4


def _timed(ctx, reps, call, classes):
    """per class: median over reps of the kernel ms of one `call`, every sample, the launches of the last one"""
    call()                                                  # warm-up (sizes every workspace)
    ctx.kernel_timing(True)
    out = {c: [] for c in classes}
    launches = {}
    for _ in range(reps):
        ctx.kernel_timing_reset()
        call()
        for c in classes:
            t = ctx.kernel_time(c)
            out[c].append(t[0])
            launches[c] = t[1]
    ctx.kernel_timing(False)
    return {c: (statistics.median(v), v, launches[c]) for c, v in out.items()}


def _wall(ctx, reps, call):
    call()
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), out


def _aim(rec, key, wmu, kl_all):
    rec[key + "_over_kl"] = wmu / statistics.median(kl_all)
    rec[key + "_within_kl_spread_plus_5_percent"] = bool(wmu <= 1.05 * max(kl_all))


def measure_dense(lib, m, k, reps):
    d, p = m, 256
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    ctx.fill_data_synthetic(0, 42)
    ctx.fill_data_synthetic(1, 43)
    scale = (0.7979 / k) ** 0.5

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    reset()
    flops = 4.0 * m * d * k
    rec = {"m": m, "d": d, "p": p, "k": k, "flops_4mdk": flops, "reps": reps, "fp32_mfma_peak_tflops": PEAK_TF, "weights": "Bernoulli(0.3) mask on X, Y unweighted"}
    kl = _timed(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, U_BIT), ["klmu"])["klmu"]
    assert kl[2] == 1, kl
    rec["kl_pass_kernel_ms"], rec["kl_pass_kernel_ms_all"] = kl[0], kl[1]
    reset()
    w, _ = _wall(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, 7))
    rec["kl_step_wall_ms"] = w
    reset()
    w, _ = _wall(ctx, reps, lambda: ctx.mu_step(0.0, 0.0, 7))
    rec["frobenius_step_wall_ms"] = w
    reset()
    t = _timed(ctx, reps, lambda: ctx.mu_weighted_step(0.0, 0.0, U_BIT), ["klmu", "gemm_nn"])
    assert t["klmu"][2] == 1, t
    rec["wmu_den1_kernel_ms"], rec["wmu_den1_kernel_ms_all"] = t["klmu"][0], t["klmu"][1]
    _aim(rec, "wmu_den1", t["klmu"][0], kl[1])
    ctx.fill_weight_synthetic(0, 44, 0.3)
    rec["wmu_layout_shares_U_V_Z_scratch_bytes"] = list(ctx.mu_weighted_layout())
    reset()
    t = _timed(ctx, reps, lambda: ctx.mu_weighted_step(0.0, 0.0, U_BIT), ["klmu", "gemm_nn"])
    assert t["klmu"][2] == 1 and t["gemm_nn"][2] == 1, t
    rec["wmu_den_kernel_ms"], rec["wmu_den_kernel_ms_all"] = t["klmu"][0], t["klmu"][1]
    rec["wmu_num_kernel_ms"], rec["wmu_num_kernel_ms_all"] = t["gemm_nn"][0], t["gemm_nn"][1]
    _aim(rec, "wmu_den", t["klmu"][0], kl[1])
    rec["wmu_den_tflops"] = flops / t["klmu"][0] * 1e-9
    rec["wmu_den_share_of_fp32_mfma_peak"] = rec["wmu_den_tflops"] / PEAK_TF
    rec["kl_pass_tflops"] = flops / kl[0] * 1e-9
    reset()
    w, w_all = _wall(ctx, reps, lambda: ctx.mu_weighted_step(0.0, 0.0, 7))
    rec["wmu_step_wall_ms"], rec["wmu_step_wall_ms_all"], rec["wmu_it_per_s"] = w, w_all, 1e3 / w
    ctx.close()
    return rec


def _csr_matrix(rows, d, npr):
    """X of bench.py's workload c5 (uniform columns), values 1.0, canonical (sorted, duplicates summed)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(42)
    cols = rng.integers(0, d, size=rows * npr, dtype=np.int32)
    A = sp.csr_matrix((np.ones(rows * npr), cols, np.arange(0, rows * npr + 1, npr, dtype=np.int64)), shape=(rows, d))
    A.sum_duplicates()
    return A


def measure_csr(lib, kind, reps, rows):
    m, d, p, k, npr = rows, 100000, 64, 256, 100
    ctx = lib.Context(0)
    ctx.set_option("sparse_mode", 2)
    ctx.set_problem(m, d, p, k)
    A = _csr_matrix(m, d, npr)
    ctx.set_data(0, A)
    ctx.fill_data_synthetic(1, 43)
    scale = (npr / d / k) ** 0.5

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    nnz = float(A.nnz)
    rec = {"workload": kind, "m": m, "d": d, "p": p, "k": k, "nnz": nnz, "reps": reps}
    kl = {}
    for name, bit in (("u_side", U_BIT), ("v_side", V_BIT)):
        reset()
        kl[name] = _timed(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, bit), ["klmu"])["klmu"]
    ctx.set_weighted_csr(0, A.indptr, A.indices, A.data, np.ones(A.nnz))
    rec["wmu_layout_shares_U_V_Z_scratch_bytes"] = list(ctx.mu_weighted_layout())
    for name, bit in (("u_side", U_BIT), ("v_side", V_BIT)):
        reset()
        t = _timed(ctx, reps, lambda: ctx.mu_weighted_step(0.0, 0.0, bit), ["klmu"])["klmu"]
        r = {"kl_pass_kernel_ms": kl[name][0], "kl_pass_kernel_ms_all": kl[name][1], "kl_launches": kl[name][2],
             "wmu_pass_kernel_ms": t[0], "wmu_pass_kernel_ms_all": t[1], "wmu_launches": t[2],
             "wmu_gathered_GBps": nnz * (k * 4.0 + 20.0) / (t[0] * 1e-3) / 1e9}
        _aim(r, "wmu_pass", t[0], kl[name][1])
        rec[name] = r
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wmu_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["65536,256", "16384,128"])
    ap.add_argument("--csr", nargs="*", default=["c5"])
    ap.add_argument("--csr-rows", type=int, default=1000000)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("wmu_timing: no GPU visible (needs an MI355X)")
    out = {"what": "weighted MU passes against the Kullback-Leibler quotient passes of the same shape on the same context; medians of device-timed repetitions",
           "shapes": [], "csr": []}
    for s in a.shapes:
        m, k = (int(v) for v in s.split(","))
        rec = measure_dense(_lib, m, k, a.reps)
        out["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    for kind in a.csr:
        rec = measure_csr(_lib, kind, a.reps, a.csr_rows)
        out["csr"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
