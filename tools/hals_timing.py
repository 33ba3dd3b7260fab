"""Time of a HALS iteration beside an MU iteration of the same shape, and how many iterations each needs.

    python tools/hals_timing.py [--out profiles/hals_timing.json] [--reps 5] [--shapes 65536,256 16384,128] [--mu-iters 100]

A HALS iteration (cmf_hals_step) forms the products of an MU iteration (cmf_mu_step) -- X^T U + Y Z, X V, Y^T V and the k x k
Grams -- and replaces MU's F .* N ./ (F G) by the coordinate-descent sweep of csrc/cmf_hals.hip.h.  For every shape (m = d, k),
p = 256, synthetic |N(0,1)| data and factors, on one context, profiler off, after a warm-up call, median of `reps` repetitions
(all kept):
  mu_step_wall_ms / hals_step_wall_ms    host clock around one call between two stream syncs, kernel timing ON for both: neither
                                         is replayed from a graph, both pay the same event pairs
  hals_sweep_class_ms                    class "hals" of one cmf_hals_step: its three sweeps (V, U, Z)
  mu_update_class_ms                     class "gemm_small" + "elementwise" of one cmf_mu_step: Grams, slab sums and the three updates
  hals_over_mu                           ratio of the wall medians; aim (not gate) <= 1.15 at 65536^2, k = 256
  hals_sweep_share_of_step               hals_sweep_class_ms / sum of all classes of the HALS step; aim < 0.10
Convergence on the same data and start: the error 0.5 |X - U V^T|_F + 0.5 |Y - V Z^T|_F (cmf_residual_sq) every 10 MU iterations
up to --mu-iters; after each of the first 10 HALS iterations and then every 5, until it is below MU's last one: the count is
exact up to 10.
Fails without a GPU.
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


def _classes(lib):
    return list(lib.KERNEL_CLASSES) + list(lib.LATER_KERNEL_CLASSES)


def _measure_step(lib, ctx, reps, call):
    """(wall median, all walls, per-class median ms, launches per class) of `call` with kernel timing on."""
    call()                                                  # warm-up (sizes every workspace)
    ctx.kernel_timing(True)
    walls, per = [], {c: [] for c in _classes(lib)}
    launches = {}
    for _ in range(reps):
        ctx.kernel_timing_reset()
        ctx.sync()
        t0 = time.perf_counter()
        call()
        ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
        for c in per:
            t = ctx.kernel_time(c)
            per[c].append(t[0])
            launches[c] = t[1]
    ctx.kernel_timing(False)
    med = {c: statistics.median(v) for c, v in per.items() if launches[c]}
    return statistics.median(walls), walls, med, {c: n for c, n in launches.items() if n}


def measure(lib, m, k, reps, mu_iters):
    d, p = m, 256
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    ctx.fill_data_synthetic(0, 42)
    ctx.fill_data_synthetic(1, 43)
    scale = (0.7979 / k) ** 0.5

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)

    def err():
        ex2, ey2 = ctx.residual_sq()
        return 0.5 * ex2 ** 0.5 + 0.5 * ey2 ** 0.5
    rec = {"m": m, "d": d, "p": p, "k": k, "reps": reps, "sweep_flops_2_rows_k2": 2.0 * (m + d + p) * k * k,
           "data_pass_flops_4_passes": 4.0 * m * d * k + 4.0 * d * p * k}
    reset()
    w, w_all, cls, n = _measure_step(lib, ctx, reps, lambda: ctx.mu_step(0.0, 0.0, 7))
    rec.update(mu_step_wall_ms=w, mu_step_wall_ms_all=w_all, mu_step_class_ms=cls, mu_step_launches=n,
               mu_update_class_ms=cls.get("gemm_small", 0.0) + cls.get("elementwise", 0.0))
    reset()
    w, w_all, cls, n = _measure_step(lib, ctx, reps, lambda: ctx.hals_step(0.0, 0.0, 7))
    assert n.get("hals") == 3, n
    rec.update(hals_step_wall_ms=w, hals_step_wall_ms_all=w_all, hals_step_class_ms=cls, hals_step_launches=n,
               hals_sweep_class_ms=cls["hals"], hals_sweep_share_of_step=cls["hals"] / sum(cls.values()),
               hals_over_mu=w / rec["mu_step_wall_ms"])
    rec["hals_sweep_tflops"] = rec["sweep_flops_2_rows_k2"] / cls["hals"] * 1e-9
    # convergence from the same start
    reset()
    mu = [(0, err())]
    for it in range(1, mu_iters + 1):
        ctx.mu_step(0.0, 0.0, 7)
        if it % 10 == 0:
            mu.append((it, err()))
    reset()
    hals = [(0, err())]
    reached = None
    for it in range(1, mu_iters + 1):
        ctx.hals_step(0.0, 0.0, 7)
        if it <= 10 or it % 5 == 0:
            hals.append((it, err()))
            if hals[-1][1] <= mu[-1][1]:
                reached = it
                break
    rec.update(mu_error_trace=mu, hals_error_trace=hals, mu_iters=mu_iters, hals_iters_to_reach_mu_error=reached)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hals_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["65536,256", "16384,128"])
    ap.add_argument("--mu-iters", type=int, default=100)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("hals_timing: no GPU visible (needs an MI355X)")
    out = {"what": "one HALS iteration beside one MU iteration on the same context and factors (kernel timing on for both), the "
                   "class of the HALS sweeps, and the iterations each method needs for the same error", "shapes": []}
    for s in a.shapes:
        m, k = (int(v) for v in s.split(","))
        rec = measure(_lib, m, k, a.reps, a.mu_iters)
        out["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
