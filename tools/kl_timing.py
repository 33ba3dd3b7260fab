"""Time of the Kullback-Leibler quotient passes beside the parent's own kernels for the same flops.

    python tools/kl_timing.py [--out profiles/kl_timing.json] [--reps 5] [--shapes 65536,256 16384,128] [--csr c5 c5z] [--csr-rows N]

Dense, for every shape (m = d, k), p = 256, synthetic |N(0,1)| data, after a warm-up call, median of `reps` device-timed
repetitions, profiler off:
  (a) kl_pass_kernel_ms   one fused quotient pass Q(X,U,V) V (class "klmu" of a U-only cmf_mu_kl_step: one launch, 4 m d k flops)
      kl_step_kernel_ms   all kernels of a full KL step (classes "klmu" + "elementwise")
  (b) parent_*            the parent's cost of the same 4 m d k flops with no quotient traffic: class "gemm_nt" of one residual_sq
                          (x side; the y side adds p / m of its flops and is included) plus class "gemm_nn" of the X V data pass of
                          a U-only cmf_mu_step, on the same context.  Both kernels are unchanged, so (b) is the parent's number.
  (c) TFLOP/s at 4 m d k per pass and the share of the 157.3 TF/s fp32-MFMA peak
  (d) KL and Frobenius iterations per second (wall time of single steps, timing off)
CSR: C5's shape as bench.py defines it (m = 1e6, d = 1e5, p = 64, k = 256, 100 non-zeros per row), X generated like workload c5
(uniform columns) and c5z (Zipf(1.1) columns): one U-side and one V-side KL pass beside the parent's SpMM for X V / X^T U on the
same matrix.  The V-side "klmu" time holds the CSR pass over X^T AND the dense pass over Y (d p k, 0.06 % of the entries' work).
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
    """median over reps of the summed kernel ms of `classes` for one `call`; also every sample and the launches of the last one."""
    call()                                                  # warm-up (sizes every workspace)
    ctx.kernel_timing(True)
    out, launches = [], 0
    for _ in range(reps):
        ctx.kernel_timing_reset()
        call()
        t = [ctx.kernel_time(c) for c in classes]
        out.append(sum(x[0] for x in t))
        launches = sum(x[1] for x in t)
    ctx.kernel_timing(False)
    return statistics.median(out), out, launches


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
    rec = {"m": m, "d": d, "p": p, "k": k, "flops_4mdk": flops, "reps": reps, "fp32_mfma_peak_tflops": PEAK_TF}
    rec["kl_layout_shares_U_V_Z_scratch_bytes"] = list(ctx.mu_kl_layout())
    a, a_all, n = _timed(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, U_BIT), ["klmu"])
    assert n == 1, n
    rec["kl_pass_kernel_ms"], rec["kl_pass_kernel_ms_all"] = a, a_all
    reset()
    s, s_all, _ = _timed(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, 7), ["klmu", "elementwise"])
    rec["kl_step_kernel_ms"], rec["kl_step_kernel_ms_all"] = s, s_all
    reset()
    nt, nt_all, _ = _timed(ctx, reps, lambda: ctx.residual_sq(), ["gemm_nt"])
    nn, nn_all, nn_launches = _timed(ctx, reps, lambda: ctx.mu_step(0.0, 0.0, U_BIT), ["gemm_nn"])
    rec["parent_nt_error_kernel_ms"], rec["parent_nt_error_kernel_ms_all"] = nt, nt_all
    rec["parent_nn_data_pass_kernel_ms"], rec["parent_nn_data_pass_kernel_ms_all"], rec["parent_nn_launches"] = nn, nn_all, nn_launches
    rec["parent_note"] = "gemm_nt of one residual_sq: x side (2 m d k) plus the y side (%.2f %% of it); gemm_nn of a U-only mu_step: X V" % (100.0 * p / m)
    rec["parent_sum_kernel_ms"] = nt + nn
    rec["kl_pass_over_parent"] = a / (nt + nn)
    rec["within_25_percent_aim"] = bool(a <= 1.25 * (nt + nn))
    rec["kl_pass_tflops"] = flops / a * 1e-9
    rec["kl_pass_share_of_fp32_mfma_peak"] = flops / a * 1e-9 / PEAK_TF
    rec["parent_tflops_same_flops"] = flops / (nt + nn) * 1e-9
    reset()
    w, w_all = _wall(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, 7))
    rec["kl_step_wall_ms"], rec["kl_it_per_s"] = w, 1e3 / w
    reset()
    w, w_all = _wall(ctx, reps, lambda: ctx.mu_step(0.0, 0.0, 7))
    rec["frobenius_step_wall_ms"], rec["frobenius_it_per_s"] = w, 1e3 / w
    ctx.close()
    return rec


def _csr_matrix(kind, rows, d, npr):
    """X of bench.py's workloads c5 (uniform columns) / c5z (Zipf(1.1) columns, vocabulary in random order), values 1.0."""
    import scipy.sparse as sp
    rng = np.random.default_rng(42)
    if kind == "c5z":
        wgt = 1.0 / np.arange(1, d + 1, dtype=np.float64) ** 1.1
        cdf = np.cumsum(wgt)
        cdf /= cdf[-1]
        cols = np.empty(rows * npr, dtype=np.int32)
        step = 1 << 24
        for a in range(0, rows * npr, step):
            cols[a:a + step] = np.searchsorted(cdf, rng.random(min(step, rows * npr - a)), side="right").astype(np.int32)
        np.minimum(cols, d - 1, out=cols)
        cols = cols.reshape(rows, npr)
        cols.sort(axis=1)
        dup = np.zeros(cols.shape, dtype=bool)
        dup[:, 1:] = cols[:, 1:] == cols[:, :-1]
        cols[dup] = rng.integers(0, d, size=int(dup.sum()), dtype=np.int32)
        cols = np.random.default_rng(7).permutation(d).astype(np.int32)[cols].reshape(-1)
    else:
        cols = rng.integers(0, d, size=rows * npr, dtype=np.int32)
    return sp.csr_matrix((np.ones(rows * npr), cols, np.arange(0, rows * npr + 1, npr, dtype=np.int64)), shape=(rows, d))


def measure_csr(lib, kind, reps, rows):
    m, d, p, k, npr = rows, 100000, 64, 256, 100
    ctx = lib.Context(0)
    ctx.set_option("sparse_mode", 2)
    ctx.set_problem(m, d, p, k)
    ctx.set_data(0, _csr_matrix(kind, m, d, npr))
    ctx.fill_data_synthetic(1, 43)
    scale = (npr / d / k) ** 0.5

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    reset()
    nnz = float(m) * npr
    rec = {"workload": kind, "m": m, "d": d, "p": p, "k": k, "nnz": nnz, "reps": reps, "layout_x": list(ctx.data_layout(0)),
           "sparse_layout_x": list(ctx.sparse_layout(0)) if hasattr(ctx, "sparse_layout") else None}
    for name, bit in (("u_side", U_BIT), ("v_side", V_BIT)):
        reset()
        a, a_all, n = _timed(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, bit), ["klmu"])
        reset()
        b, b_all, nb = _timed(ctx, reps, lambda: ctx.mu_step(0.0, 0.0, bit), ["spmm"])
        rec[name] = {"kl_pass_kernel_ms": a, "kl_pass_kernel_ms_all": a_all, "kl_launches": n,
                     "parent_spmm_kernel_ms": b, "parent_spmm_kernel_ms_all": b_all, "parent_spmm_launches": nb,
                     "kl_over_parent_spmm": a / b if b else None,
                     "kl_gathered_GBps": nnz * (k * 4.0 + 16.0) / (a * 1e-3) / 1e9}
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kl_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["65536,256", "16384,128"])
    ap.add_argument("--csr", nargs="*", default=["c5", "c5z"])
    ap.add_argument("--csr-rows", type=int, default=1000000)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("kl_timing: no GPU visible (needs an MI355X)")
    out = {"what": "Kullback-Leibler quotient passes against the parent's kernels for the same flops; medians of device-timed repetitions",
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
