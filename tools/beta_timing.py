"""Time of the beta-divergence passes: the dual-output pass beside its two single-output twins and the KL quotient pass.

    python tools/beta_timing.py [--out profiles/beta_timing.json] [--reps 5] [--shapes 65536,256 16384,128]

For every shape (m = d, k), p = 256, synthetic |N(0,1)| data, after a warm-up call, median of `reps` device-timed repetitions,
profiler off, all in one process on one context:
  (a) dual_pass_kernel_ms     class "klmu" of a U-only cmf_mu_beta_step under option beta_route = 1: ONE launch forming num and den
                              (6 m d k flops).  null at a width whose dual kernel does not ship (its compile needs scratch).
  (b) twin_passes_kernel_ms   the same under beta_route = 2: the numerator-only and the denominator-only pass (two launches, 8 m d k)
  (c) kl_pass_kernel_ms       class "klmu" of a U-only cmf_mu_kl_step: the quotient pass (one launch, 4 m d k)
  (d) beta_step_kernel_ms     all kernels (classes "klmu" + "elementwise") of a whole step at beta = 0 and beta = 0.5 on the shipped
                              route, beside kl_step_kernel_ms, a whole KL step; every sample is kept (the spread of the KL step's
                              samples is the allowance of its comparison with the parent's build)
(a) and (b) are taken at beta = 0 (the reciprocal form) and at beta = 0.5 (log2 / exp2).
Before timing, 64 sampled rows of num and den of the U sweep from cmf_mu_beta_products are checked against float64 within the
bound of tests/beta_yardstick.py, at both betas and on both routes where there are two.
Fails without a GPU.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TF = 157.3
U_BIT = 1
EPS = 2.0 ** -23


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


def _check_rows(ctx, m, d, k, beta, rows):
    """worst |err| / bound of the sampled rows of num and den of the U sweep against float64."""
    import beta_yardstick as BY
    num, den = ctx.mu_beta_products(beta, 0)
    U, V = ctx.get_factor(0), ctx.get_factor(1)
    worst = 0.0
    for r in rows:
        x = ctx.get_data_block(0, int(r), 1, 0, d)[0].astype(np.float64)
        s = V @ U[r]
        p = np.maximum(s, EPS) ** (beta - 2.0)
        tol = BY.tau_products(k, d, beta, float(np.abs(np.log2(np.maximum(s, EPS))).max()))
        for got, ref in ((num[r, :k], (x * p) @ V), (den[r, :k], (s * p) @ V)):
            assert np.isfinite(got).all() and (ref > 0).all()
            worst = max(worst, float((np.abs(got - ref) / (tol * ref)).max()))
    assert worst <= 1.0, "sampled rows of cmf_mu_beta_products at beta = %g: worst |err| / bound = %.3f" % (beta, worst)
    return worst


def measure(lib, m, k, reps):
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
    mdk = float(m) * d * k
    rec = {"m": m, "d": d, "p": p, "k": k, "mdk": mdk, "reps": reps, "fp32_mfma_peak_tflops": PEAK_TF,
           "beta_layout_shares_U_V_Z_scratch_bytes": list(ctx.mu_beta_layout())}
    rows = np.random.RandomState(0).choice(m, 64, replace=False)
    for beta in (0.0, 0.5):
        tag = "beta_%g" % beta
        r = rec[tag] = {}
        for route, name in ((1, "dual"), (2, "twin")):
            ctx.set_option("beta_route", route)
            r["sampled_rows_worst_err_over_bound_%s" % name] = _check_rows(ctx, m, d, k, beta, rows)
            ms, samples, launches = _timed(ctx, reps, lambda: ctx.mu_beta_step(beta, 0.0, 0.0, U_BIT), ["klmu"])
            reset()
            if name == "dual" and launches != 1:          # this width does not ship the dual kernel: route 1 ran the twins
                r["dual_pass_kernel_ms"] = None
                continue
            assert launches == (1 if name == "dual" else 2), launches
            key = "dual_pass" if name == "dual" else "twin_passes"
            r[key + "_kernel_ms"], r[key + "_kernel_ms_all"] = ms, samples
            r[key + "_tflops"] = (6.0 if name == "dual" else 8.0) * mdk / ms * 1e-9
        ctx.set_option("beta_route", 0)
        if r["dual_pass_kernel_ms"] is not None:
            r["dual_over_twins"] = r["dual_pass_kernel_ms"] / r["twin_passes_kernel_ms"]
            r["dual_is_faster_than_the_twins"] = bool(r["dual_pass_kernel_ms"] < r["twin_passes_kernel_ms"])
        ms, samples, _ = _timed(ctx, reps, lambda: ctx.mu_beta_step(beta, 0.0, 0.0, 7), ["klmu", "elementwise"])
        reset()
        r["beta_step_kernel_ms"], r["beta_step_kernel_ms_all"] = ms, samples
    ms, samples, launches = _timed(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, U_BIT), ["klmu"])
    assert launches == 1, launches
    reset()
    rec["kl_pass_kernel_ms"], rec["kl_pass_kernel_ms_all"] = ms, samples
    rec["kl_pass_tflops"] = 4.0 * mdk / ms * 1e-9
    ms, samples, _ = _timed(ctx, reps, lambda: ctx.mu_kl_step(0.0, 0.0, 7), ["klmu", "elementwise"])
    rec["kl_step_kernel_ms"], rec["kl_step_kernel_ms_all"] = ms, samples
    rec["kl_step_kernel_ms_spread"] = max(samples) - min(samples)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beta_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["65536,256", "16384,128"])
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("beta_timing: no GPU visible (needs an MI355X)")
    out = {"what": "beta-divergence passes: the dual-output pass (6 m d k) against its two single-output twins (8 m d k) and the KL quotient "
                   "pass (4 m d k); whole steps at beta = 0 and 0.5 beside a KL step; medians of device-timed repetitions", "shapes": []}
    for s in a.shapes:
        m, k = (int(v) for v in s.split(","))
        rec = measure(_lib, m, k, a.reps)
        out["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
