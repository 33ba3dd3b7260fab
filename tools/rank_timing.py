"""Time of the held-out rank call beside top-n at n = 10 on the same context, factors and build.

    python tools/rank_timing.py [--out profiles/rank_timing.json] [--reps 5] [--shapes 65536,256 16384,128]

For every shape (m = d, k), all rows in one call, 10 random held-out entries and an exclusion list of about 100 per row, after a
warm-up call, median of `reps` device-timed repetitions, profiler off:
  (a) rank_kernel_ms   kernel time of one Context.rank call (class "topk": extract + scan + finish kernels, device events)
  (b) topk_kernel_ms   the yardstick: kernel time of Context.topk at n = 10 with the same exclusion lists (scan + merge)
  (c) rank_wall_ms     end-to-end wall time of Context.rank (list checks, launch table, uploads, launches, read-back), timing off
The aim is (a) <= 2.5 (b).  Rates: algorithmic TFLOP/s = 2 m d k / kernel time.  Fails without a GPU.
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
HELD, EXCL = 10, 100


def lists(m, d, seed):
    """Per row HELD held-out and about EXCL excluded columns, disjoint, as two CSR pairs (repeated draws are dropped)."""
    rng = np.random.RandomState(seed)
    cols = np.sort(rng.randint(0, d, size=(m, HELD + EXCL)), axis=1)
    fresh = np.ones(cols.shape, dtype=bool)
    fresh[:, 1:] = cols[:, 1:] != cols[:, :-1]
    held = (rng.rand(*cols.shape).argsort(axis=1).argsort(axis=1) < HELD) & fresh
    out = []
    for mask in (held, fresh & ~held):
        indptr = np.concatenate(([0], np.cumsum(mask.sum(axis=1)))).astype(np.int64)
        out.append((indptr, cols[mask].astype(np.int32)))
    return out


def measure(lib, m, k, reps):
    d, p = m, 256
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    scale = (0.7979 / k) ** 0.5
    for w, seed in ((0, 101), (1, 102), (2, 103)):
        ctx.fill_factor_synthetic(w, seed, 0, scale)
    held, excl = lists(m, d, 7)
    flops = 2.0 * m * d * k
    rec = {"m": m, "d": d, "k": k, "flops_2mdk": flops, "reps": reps, "fp32_mfma_peak_tflops": PEAK_TF,
           "held_out_entries": int(held[0][-1]), "excluded_entries": int(excl[0][-1])}

    def timed(call):
        call()                                           # warm-up
        ctx.kernel_timing(True)
        ks = []
        for _ in range(reps):
            ctx.kernel_timing_reset()
            call()
            ks.append(ctx.kernel_time("topk")[0])
        ctx.kernel_timing(False)
        wall = []
        for _ in range(reps):
            ctx.sync()
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        return ks, wall

    tk, tw = timed(lambda: ctx.topk(lib.CMF_U, lib.CMF_V, 10, exclude=excl))
    rk, rw = timed(lambda: ctx.rank(lib.CMF_U, lib.CMF_V, held, exclude=excl))
    hb, split, chunk, scratch = ctx.rank_layout(m, lib.CMF_V, rec["held_out_entries"], rec["excluded_entries"])
    tms, rms = statistics.median(tk), statistics.median(rk)
    rec.update({
        "topk_n10_kernel_ms": tms, "topk_n10_kernel_ms_all": tk, "topk_n10_wall_ms": statistics.median(tw),
        "topk_n10_algorithmic_tflops": flops / tms * 1e-9,
        "rank_kernel_ms": rms, "rank_kernel_ms_all": rk, "rank_wall_ms": statistics.median(rw), "rank_wall_ms_all": rw,
        "rank_algorithmic_tflops": flops / rms * 1e-9, "rank_share_of_fp32_mfma_peak": flops / rms * 1e-9 / PEAK_TF,
        "rank_over_topk_n10_kernel": rms / tms, "within_2p5x_aim": bool(rms <= 2.5 * tms),
        "held_per_virtual_query": hb, "candidate_shares": split, "virtual_queries_per_launch": chunk, "scratch_bytes": scratch,
        "scratch_share_of_dense_product": scratch / (4.0 * m * d),
    })
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="*", default=["65536,256", "16384,128"])
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("rank_timing: no GPU visible (needs an MI355X)")
    out = {"what": "held-out ranks (all rows, one call, %d held-out and ~%d excluded entries per row) against top-n at n = 10 with the "
                   "same exclusion lists; medians of device-timed repetitions" % (HELD, EXCL), "shapes": []}
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
