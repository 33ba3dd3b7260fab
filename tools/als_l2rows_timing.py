"""Cost of the per-row l2 (cmf_set_l2_rows): the U sweep of every route with nothing bound and with ragged multipliers, in the same
process, and the unbound figures beside a build of the parent commit run in the same session before and after.

    python tools/als_l2rows_timing.py [--out profiles/als_l2rows_timing.json] [--reps 5] [--cases c5 a] [--parent-root DIR] [--append]

The protocol of tools/als_cg_timing.py: every case in a child process of its own under its own time limit (after a child that fails,
is killed or runs out of time nothing more is started); profiler off; after a warm-up call the median of `reps` device-timed
repetitions (every kernel class added up), every one from the same factors, all samples kept.  Cases and routes (U sweep, nn_mask 0
but for the non-negative route, l2 = 0.1):
  c5   C5's pattern as bench.py defines it: 1e6 x 1e5, 100 entries per row, uniform columns, k = 256 --
       exact (cmf_als_step), cg6 (cmf_als_cg_step, 6 steps), nncg3 (cmf_als_nncg_step, 3 steps), dual128 (cmf_als_dual_step)
  a    65536 rows x 1024 entries over 65536 columns, k = 256 -- exact
Per route: unbound_* (no multipliers: the LR = false kernel instances), bound_* (multipliers from {0.5, 1, 2, 4} in a fixed random
order: the LR = true instances), bound_over_unbound.  --parent-root names a checkout of the parent commit with its library built:
the same unbound calls are then run from that tree before and after this tree's (`parent_before`, `parent_after`), each case in a
process of its own; `unbound_vs_parent` puts the three medians side by side, with the kernel classes of each (the Cholesky solves
of class eigen and the normal equations of class rowhess are the parent's code: what they differ by between the trees is the
session's drift).  Without it the parent blocks are left out.  One call is one session; --append adds a session to the file.
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
from kl_timing import _csr_matrix  # noqa: E402  (and the same C5 pattern)

U_BIT = 1
CASES = ("c5", "a")
CHILD_LIMIT_S = 420
VALUES = (0.5, 1.0, 2.0, 4.0)


def measure(lib, case, reps):
    l2 = 0.1
    if case == "a":
        m, d, p, k, npr = 65536, 65536, 256, 256, 1024
        rng = np.random.default_rng(42)
        indices = rng.integers(0, d, size=m * npr, dtype=np.int32)
        indptr = np.arange(0, m * npr + 1, npr, dtype=np.int64)
        scale = (0.7979 / k) ** 0.5
    else:
        m, d, p, k, npr = 1000000, 100000, 64, 256, 100
        Xs = _csr_matrix("c5", m, d, npr)
        indptr, indices = Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32)
        del Xs
        scale = (npr / d / k) ** 0.5
    print("case %s: pattern ready" % case, flush=True)
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    nnz = indices.size
    ctx.set_weighted_csr(0, indptr, indices, np.random.default_rng(1 if case == "a" else 2).random(nnz) + 0.5, np.ones(nnz))
    del indices
    ctx.fill_data_synthetic(1, 43)
    print("case %s: bound" % case, flush=True)

    def reset():
        for w, seed in ((0, 101), (1, 102), (2, 103)):
            ctx.fill_factor_synthetic(w, seed, 0, scale)
    routes = [("exact", lambda: ctx.als_step(l2, 0, U_BIT))]
    if case == "c5":
        routes += [("cg6", lambda: ctx.als_cg_step(l2, 0, U_BIT, 6, 0)), ("nncg3", lambda: ctx.als_nncg_step(l2, U_BIT, U_BIT, 0, 3, 0)),
                   ("dual128", lambda: ctx.als_dual_step(l2, 0, U_BIT, 128))]
    can_bind = hasattr(ctx, "set_l2_rows")                   # (a build of the parent commit: the unbound figures only)
    mult = np.random.default_rng(5).permutation(np.resize(VALUES, m)).astype(np.float64)
    rec = {"case": case, "m": m, "d": d, "p": p, "k": k, "k_pad": ctx.geometry()[3], "entries_per_row": npr, "nnz": int(nnz), "reps": reps,
           "l2": l2, "multipliers": list(VALUES) if can_bind else None, "routes": {}}
    for tag, call in routes:
        r = {}
        for state in (("unbound", "bound") if can_bind else ("unbound",)):
            if can_bind:
                ctx.set_l2_rows(0, mult if state == "bound" else None)
            kms, k_all, classes = _timed(ctx, lib, reps, reset, call)
            r.update({state + "_kernel_ms": kms, state + "_kernel_ms_all": k_all, state + "_kernel_classes_ms": classes})
        if can_bind:
            ctx.set_l2_rows(0, None)
            r["bound_over_unbound"] = r["bound_kernel_ms"] / r["unbound_kernel_ms"]
        rec["routes"][tag] = r
        print("  %s: unbound %.2f ms%s" % (tag, r["unbound_kernel_ms"],
                                         ", bound %.2f ms (x %.4f)" % (r["bound_kernel_ms"], r["bound_over_unbound"]) if can_bind else ""), flush=True)
    ctx.close()
    return rec


def _run_cases(a, root, tag):
    """Every case of one tree, each in a child process of its own; the records."""
    out = []
    for case in a.cases:
        part = a.out + "." + tag + "." + case + ".part"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--out", part, "--reps", str(a.reps), "--root", root]
        try:
            status = subprocess.run(cmd, timeout=CHILD_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit("als_l2rows_timing: %s case %s ran out of its %d s; nothing more is started" % (tag, case, CHILD_LIMIT_S))
        if status != 0:
            raise SystemExit("als_l2rows_timing: %s case %s ended with status %d; nothing more is started" % (tag, case, status))
        with open(part) as f:
            out.append(json.load(f))
        os.remove(part)
    return out


def compare(ses):
    rows = []
    for i, rec in enumerate(ses["cases"]):
        for tag, r in rec["routes"].items():
            b, e = ses["parent_before"][i]["routes"][tag], ses["parent_after"][i]["routes"][tag]
            pb, pa = b["unbound_kernel_ms"], e["unbound_kernel_ms"]
            rows.append({"case": rec["case"], "route": tag, "parent_before_ms": pb, "unbound_ms": r["unbound_kernel_ms"], "parent_after_ms": pa,
                         "parent_runs_differ_ms": abs(pa - pb), "unbound_minus_slower_parent_ms": r["unbound_kernel_ms"] - max(pa, pb),
                         "classes_ms": {"parent_before": b["unbound_kernel_classes_ms"], "unbound": r["unbound_kernel_classes_ms"],
                                        "parent_after": e["unbound_kernel_classes_ms"]},
                         "bound_ms": r["bound_kernel_ms"], "bound_over_unbound": r["bound_over_unbound"]})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_l2rows_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=CASES)
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--parent-commit", default=None, help="its commit id, for the record")
    ap.add_argument("--append", action="store_true", help="keep the sessions the file holds and add this one")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:                                              # one case of one tree, in this process; the record goes to the file --out names
        sys.path.insert(0, os.path.abspath(a.root))          # (before this tree: the package of the tree that is measured)
        from pycmf_amd import _lib
        assert os.path.abspath(os.path.dirname(os.path.dirname(_lib.__file__))) == os.path.abspath(a.root)
        if _lib.device_count() < 1:
            raise SystemExit("als_l2rows_timing: no GPU visible (needs an MI355X)")
        rec = measure(_lib, a.child, a.reps)
        with open(a.out, "w") as f:
            json.dump(rec, f)
        return
    ses = {}
    out = {"what": "U sweep of the ALS row routes with no per-row l2 bound (LR = false kernel instances) and with ragged multipliers from {0.5, 1, 2, 4} "
                   "(LR = true), same process, pattern and factors; medians and all samples of device-timed repetitions (every kernel class added "
                   "up), every repetition from the same factors; parent_before / parent_after: the unbound calls from a build of the parent commit, "
                   "each case in a process of its own, in the same session before and after this tree's",
           "parent_commit": a.parent_commit, "sessions": []}
    if a.append and os.path.exists(a.out):
        with open(a.out) as f:
            out["sessions"] = json.load(f).get("sessions", [])
    out["sessions"].append(ses)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.parent_root:
        ses["parent_before"] = _run_cases(a, a.parent_root, "parent_before")
    ses["cases"] = _run_cases(a, ROOT, "this")
    if a.parent_root:
        ses["parent_after"] = _run_cases(a, a.parent_root, "parent_after")
        ses["unbound_vs_parent"] = rows = compare(ses)
        for row in rows:
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
