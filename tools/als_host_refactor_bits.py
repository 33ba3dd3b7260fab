"""Bits of every ALS entry point on a fixed list of small cases: one SHA-256 per case over the float32 bytes of U, V and Z (and of
the bias vectors where biases are bound) after TWO steps from the same start, so that the second step reads the first's output, with
the counters of cmf_als_cg_last / cmf_als_nncg_last / cmf_als_nncg_passes / cmf_als_dual_last behind it.  For any change that must
leave the results of the ALS routes as they are (a refactor of the host code or of the kernels): run on the commit before it and on
the commit with it, on the same GPU, the two records must be equal entry for entry.

    python tools/als_host_refactor_bits.py [--label parent|branch] [--out profiles/als_host_refactor_bits.json] [--digest F]

The record goes under its label into the file --out names, beside the other label's if that is there already; with both there the
tool compares them and fails on the first difference.  Without --label nothing is run (no GPU needed): the file is compared as it
stands.  --digest F writes what is small enough to keep in the repository when the record is not: per label and per kind of case
the number of cases and one SHA-256 over their lines, and the Huber deltas with the shares of the residuals above them.

The problem is tests/als_dual_cases.py::problem(k): 48 x 160 x 40, both relations observed, row lengths on both sides of 32 / 64 /
128, empty rows and rows of one entry; k = 3, 40, 100, 200 (k_pad 32, 64, 128, 256); once with als_piece = 32 and als_cg_piece = 16
(rows of several pieces, long CG rows) and once with the defaults.  A background weight (0.25 on X) needs every stored weight at or
above it: those cases bind max(w, 0.25) in place of the weights with stored zeros; they run the matrix-free steps too (the shared
term S x of every product, on rows with pieces).  The logistic cases bind the labels Y > 0.  The matrix-free row hooks run a second
time with "als_cg_lds" = 0 (every row streams) and a third time, with one step of each route, under per-row l2 multipliers
(cmf_set_l2_rows) on all three factors.

The entry passes (the reweighting passes and the losses, which walk the stored entries of row pieces) have kinds of their own, each
on that problem with the default pieces and on a LONG-ROW problem at k = 40 and 200: X 4 x 4097 with one row of 4097 stored entries
(three pieces of the passes' 2048, the last of ONE entry: a piece boundary and the clamped tail), one row of one entry and one empty
row, Y 4097 x 8 small and observed.
  huber        X under a Huber delta: the median of the stored |residuals| at the start, computed here in float64; the share of the
               residuals above it is recorded and must lie in 1/3 .. 2/3 (neither omega = 1 everywhere nor everything clipped)
  huber_bias   the same with biases on X, the bias sweeps included
  logit_pass   a logistic relation under cmf_set_logit_pass
  logit_fused  a logistic relation reweighted inside the normal-equation kernel
The logistic relation is Y on the tool's problem and X, the relation with the long row, on the long-row problem.  Each kind records
the SHA-256 of hw and of hp from the *_weights entry of both images (not logit_fused, which has none), the loss (cmf_als_huber_loss /
cmf_als_logistic_loss) as the hex of its double, and the factor hash after two steps of every route the kind allows: exact, nnls, cg,
nncg, dual.
Fails without a GPU."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import als_dual_cases as C  # noqa: E402

L2 = C.L2
KS = (3, 40, 100, 200)
BG = 0.25
ROWS = (3, 20)              # the row hooks: rows 3 .. 23


def _bind(ctx, which, T, W):
    if W is None:
        ctx.set_data(which, T)
        return
    r = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
    ctx.set_weighted_csr(which, W.indptr, W.indices, np.asarray(T)[r, W.indices], W.data)


def _context(lib, k, pieces, kind):
    """kind: '' both relations observed | 'bias' x biases on | 'bg' a background weight on X | 'logit' Y logistic | 'full' X unweighted."""
    X, Y, Wx, Wy, F = C.problem(k)
    ctx = lib.Context(0)
    if pieces:
        ctx.set_option("als_piece", 32)
        ctx.set_option("als_cg_piece", 16)
    ctx.set_problem(C.M, C.D, C.P, k)
    if kind == "bg":
        Wx = Wx.copy()
        Wx.data = np.maximum(Wx.data, BG)
    _bind(ctx, 0, X, None if kind == "full" else Wx)
    _bind(ctx, 1, (Y > 0).astype(np.float64) if kind == "logit" else Y, Wy)
    if kind == "bg":
        ctx.set_background_weight(0, BG)
    if kind == "bias":
        ctx.set_biases(0, True, 0.125, 0.5)
    if kind == "logit":
        ctx.set_relation_loss(1, "logistic")
    return ctx, F


def _reset(ctx, F, kind):
    for w in range(3):
        ctx.set_factor(w, F[w])
    if "bias" in kind:
        for axis, n in ((0, F[0].shape[0]), (1, F[1].shape[0])):
            ctx.set_bias(0, axis, np.zeros(n))


def _counters(ctx):
    return {"cg_last": [int(v) for v in ctx.als_cg_last()], "nncg_last": [int(v) for v in ctx.als_nncg_last()],
            "nncg_passes": [int(v) for v in ctx.als_nncg_passes()], "dual_last": [int(v) for v in ctx.als_dual_last()]}


def _state(ctx, kind):
    h = hashlib.sha256()
    for w in range(3):
        h.update(ctx.get_factor(w).astype(np.float32).tobytes())
    if "bias" in kind:
        for axis in (0, 1):
            h.update(ctx.get_bias(0, axis).astype(np.float32).tobytes())
    return dict(_counters(ctx), sha256=h.hexdigest())


DUAL = (("dual_max 128", (128, 0, 0)), ("dual_max 20", (20, 0, 0)), ("dual_max 0", (0, 0, 0)), ("nn_sweeps 2", (128, 2, 0)),
        ("nn_cg_steps 3", (128, 0, 3)))


def _steps(kind):
    """(name, call(ctx)) of the step cases on a context of that kind."""
    out = []
    if kind == "":
        out += [("als_step signed", lambda c: c.als_step(L2, 0, 7)), ("als_step nn 7", lambda c: c.als_step(L2, 7, 7)),
                ("als_nnls_step 2 nn 7", lambda c: c.als_nnls_step(L2, 7, 7, 2)), ("als_nnls_step 2 nn 2", lambda c: c.als_nnls_step(L2, 2, 7, 2)),
                ("als_cg_step 3 0 nn 5", lambda c: c.als_cg_step(L2, 5, 7, 3, 0)), ("als_cg_step 3 2 nn 5", lambda c: c.als_cg_step(L2, 5, 7, 3, 2)),
                ("als_nncg_step 0 3 0 nn 7", lambda c: c.als_nncg_step(L2, 7, 7, 0, 3, 0)),
                ("als_nncg_step 3 3 2 nn 5", lambda c: c.als_nncg_step(L2, 5, 7, 3, 3, 2)),
                ("als_nncg_step 3 3 0 nn 0", lambda c: c.als_nncg_step(L2, 0, 7, 3, 3, 0)),
                ("als_bias_step no biases cg 0", lambda c: c.als_bias_step(L2, 0, 7, 0, 0)),
                ("als_bias_step no biases cg 3", lambda c: c.als_bias_step(L2, 5, 7, 3, 2))]
    if kind == "bias":
        out += [("als_bias_step cg 0", lambda c: c.als_bias_step(L2, 0, 7, 0, 0)), ("als_bias_step cg 3", lambda c: c.als_bias_step(L2, 0, 7, 3, 0))]
    if kind == "bg":
        out += [("als_cg_step 3 0 nn 0", lambda c: c.als_cg_step(L2, 0, 7, 3, 0)), ("als_nncg_step 0 3 0 nn 7", lambda c: c.als_nncg_step(L2, 7, 7, 0, 3, 0))]
    if kind in ("", "bias", "bg"):
        for name, (dm, ns, ncg) in DUAL:
            if kind == "bias" and ncg:
                continue                                     # refused: nn_cg_steps with biases bound
            nn = 5 if ns or ncg else 0
            out.append(("als_dual_step " + name, lambda c, dm=dm, ns=ns, ncg=ncg, nn=nn: c.als_dual_step(L2, nn, 7, dm, ns, ncg)))
    if kind == "logit":
        out += [("als_step", lambda c: c.als_step(L2, 0, 7)), ("als_nnls_step 2 nn 7", lambda c: c.als_nnls_step(L2, 7, 7, 2))]
    if kind == "full":
        out += [("als_step", lambda c: c.als_step(L2, 0, 7))]
    return out


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def _matrix_free(ctx, F, tag, rec):
    """The CG and NNCG row hooks with every row streamed, then the hooks and one step of each route under per-row l2 multipliers."""
    def hooks(label):
        for w in range(3):
            for name, hook in (("als_cg_rows", ctx.als_cg_rows), ("als_nncg_rows", ctx.als_nncg_rows)):
                got = hook(w, ROWS[0], ROWS[1], L2, 3)
                rec["%s | %s | %s %s" % (tag, label, name, "UVZ"[w])] = dict(_counters(ctx), sha256=_sha(got))
    ctx.set_option("als_cg_lds", 0)
    hooks("als_cg_lds 0")
    ctx.set_option("als_cg_lds", -1)
    for w, n in enumerate((C.M, C.D, C.P)):
        ctx.set_l2_rows(w, 0.5 + 0.375 * (np.arange(n) % 7))
    hooks("l2 rows")
    for name, call in (("als_cg_step 3 0 nn 0", lambda c: c.als_cg_step(L2, 0, 7, 3, 0)),
                       ("als_nncg_step 0 3 0 nn 7", lambda c: c.als_nncg_step(L2, 7, 7, 0, 3, 0))):
        _reset(ctx, F, "")
        call(ctx)
        call(ctx)
        rec["%s | l2 rows | %s" % (tag, name)] = _state(ctx, "")
    for w in range(3):
        ctx.set_l2_rows(w, None)


ENTRY_KINDS = ("huber", "huber_bias", "logit_pass", "logit_fused")
LONG_D, LONG_P, LONG_KS = 4097, 8, (40, 200)
MU = 0.125


def _long_problem(k, seed=23):
    """(X, Y, Wx, Wy, [U, V, Z]): X 4 x 4097 with rows of 4097, 1, 0 and 5 stored entries; Y 4097 x 8 with three entries in every fifth
    row and one full row."""
    import scipy.sparse as sp
    rng = np.random.RandomState(1000 * seed + k)
    r = np.concatenate([np.zeros(LONG_D, dtype=np.int64), [1], np.full(5, 3)])
    c = np.concatenate([np.arange(LONG_D), [2048], [0, 7, 2047, 2048, 4096]])
    Wx = sp.csr_matrix((C.f32(0.5 + rng.rand(r.size)), (r, c)), shape=(4, LONG_D))
    fifth = np.arange(0, LONG_D, 5)
    ry = np.concatenate([np.repeat(fifth, 3), np.full(LONG_P, 1)])
    cy = np.concatenate([np.tile([0, 3, 6], fifth.size), np.arange(LONG_P)])
    Wy = sp.csr_matrix((C.f32(0.5 + rng.rand(ry.size)), (ry, cy)), shape=(LONG_D, LONG_P))
    for W in (Wx, Wy):
        W.sort_indices()
    X, Y = C.f32(rng.randn(4, LONG_D)), C.f32(rng.randn(LONG_D, LONG_P))
    F = [C.f32(rng.randn(n, k) / np.sqrt(k)) for n in (4, LONG_D, LONG_P)]
    return X, Y, Wx, Wy, F


def _huber_delta(X, Wx, F, mu):
    """(delta, share): the float32 median of |t - mu - u . v| over the stored entries of X at the start, in float64, and the share of
    those residuals above it."""
    r = np.repeat(np.arange(Wx.shape[0]), np.diff(Wx.indptr))
    res = np.abs(np.asarray(X, dtype=np.float64)[r, Wx.indices] - mu - np.einsum("ij,ij->i", F[0][r], F[1][Wx.indices]))
    delta = float(np.float32(np.median(res)))
    share = float(np.mean(res > delta))
    if not 1.0 / 3.0 <= share <= 2.0 / 3.0:
        raise SystemExit("als_host_refactor_bits: %.3f of the residuals exceed the Huber delta %g; the case needs 1/3 .. 2/3" % (share, delta))
    return delta, share


def _entry_routes(kind):
    """(name, call(ctx)) of the routes a kind allows."""
    if kind == "huber_bias":                                 # (nn_cg_steps is refused with biases bound)
        return [("exact", lambda c: c.als_bias_step(L2, 0, 7, 0, 0)), ("nnls", lambda c: c.als_bias_step(L2, 7, 7, 0, 2)),
                ("cg", lambda c: c.als_bias_step(L2, 0, 7, 3, 0)), ("dual", lambda c: c.als_dual_step(L2, 0, 7, 128, 0, 0))]
    out = [("exact", lambda c: c.als_step(L2, 0, 7)), ("nnls", lambda c: c.als_nnls_step(L2, 7, 7, 2))]
    if kind == "logit_fused":                                # (the routes without formed systems refuse a fused logistic relation)
        return out
    return out + [("cg", lambda c: c.als_cg_step(L2, 0, 7, 3, 0)), ("nncg", lambda c: c.als_nncg_step(L2, 7, 7, 0, 3, 0)),
                  ("dual", lambda c: c.als_dual_step(L2, 0, 7, 128, 0, 0))]


def _entry_case(lib, tag, prob, k, kind, logit_rel, rec):
    X, Y, Wx, Wy, F = prob
    ctx = lib.Context(0)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], k)
    T, W = [X, Y], [Wx, Wy]
    if kind.startswith("logit"):
        T[logit_rel] = (T[logit_rel] > 0).astype(np.float64)
    for which in (0, 1):
        _bind(ctx, which, T[which], W[which])
    head = "%s | %s | " % (tag, kind)
    if kind.startswith("huber"):
        mu = MU if kind == "huber_bias" else 0.0
        if kind == "huber_bias":
            ctx.set_biases(0, True, mu, 0.5)
        delta, share = _huber_delta(X, Wx, F, mu)
        ctx.set_huber_delta(0, delta)
        rec[head + "delta"] = {"delta": float(delta).hex(), "share_above": share}
        weights, which, loss = ctx.als_huber_weights, 0, lambda: ctx.als_huber_loss()[0]
    else:
        ctx.set_relation_loss(logit_rel, "logistic")
        ctx.set_logit_pass(logit_rel, kind == "logit_pass")
        weights, which, loss = (ctx.als_logit_weights if kind == "logit_pass" else None), logit_rel, lambda: ctx.als_logistic_loss()[logit_rel]
    _reset(ctx, F, kind)
    if weights:
        for t in (0, 1):
            hw, hp = weights(which, t, W[which].nnz)
            rec[head + "weights image %d" % t] = {"hw": _sha(hw), "hp": _sha(hp)}
    rec[head + "loss"] = {"loss": float(loss()).hex()}
    for name, call in _entry_routes(kind):
        _reset(ctx, F, kind)
        call(ctx)
        call(ctx)
        rec[head + name] = dict(_state(ctx, kind), loss=float(loss()).hex())
    ctx.close()


def _entry_passes(lib, rec):
    for kind in ENTRY_KINDS:
        for k in KS:
            _entry_case(lib, "k %d default pieces" % k, C.problem(k), k, kind, 1, rec)
        for k in LONG_KS:
            _entry_case(lib, "k %d long row" % k, _long_problem(k), k, kind, 0, rec)
        print("%s: done" % kind, flush=True)


def record(lib):
    rec = {}
    _entry_passes(lib, rec)
    for k in KS:
        for pieces in (True, False):
            tag = "k %d %s" % (k, "pieces 32/16" if pieces else "default pieces")
            for kind in ("", "bias", "bg", "logit", "full"):
                ctx, F = _context(lib, k, pieces, kind)
                for name, call in _steps(kind):
                    _reset(ctx, F, kind)
                    call(ctx)
                    call(ctx)
                    rec["%s | %s | %s" % (tag, kind or "observed", name)] = _state(ctx, kind)
                if kind == "":                               # the row hooks, rows 3 .. 23 of each factor, the factors at their start
                    _reset(ctx, F, kind)
                    for w in range(3):
                        hooks = (("als_cg_rows", lambda: ctx.als_cg_rows(w, ROWS[0], ROWS[1], L2, 3)),
                                 ("als_nncg_rows", lambda: ctx.als_nncg_rows(w, ROWS[0], ROWS[1], L2, 3)),
                                 ("als_dual_rows", lambda: ctx.als_dual_rows(w, ROWS[0], ROWS[1], L2, 128)),
                                 ("als_normal", lambda: ctx.als_normal(w, ROWS[0], ROWS[1], L2)))
                        for name, hook in hooks:
                            got = hook()
                            rec["%s | observed | %s %s" % (tag, name, "UVZ"[w])] = dict(
                                _counters(ctx), sha256=_sha(*got) if isinstance(got, tuple) else _sha(got))
                    _matrix_free(ctx, F, tag, rec)
                ctx.close()
            print("%s: done" % tag, flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", choices=("parent", "branch"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "als_host_refactor_bits.json"))
    ap.add_argument("--digest")
    a = ap.parse_args()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    if a.label:
        from pycmf_amd import _lib
        if _lib.device_count() < 1:
            raise SystemExit("als_host_refactor_bits: no GPU visible (needs an MI355X)")
        out[a.label] = record(_lib)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                          # one line per case
            f.write("{\n" + ",\n".join(' "%s": {\n%s\n }' % (label, ",\n".join('  %s: %s' % (json.dumps(n), json.dumps(rec[n], sort_keys=True))
                                                                           for n in sorted(rec))) for label, rec in sorted(out.items())) + "\n}\n")
        print("%s: %d cases" % (a.label, len(out[a.label])))
    if a.digest:
        dig = {}
        for label, rec in sorted(out.items()):
            kinds = {}
            for n in sorted(rec):                            # "tag | kind | what"
                kinds.setdefault(n.split(" | ")[1], []).append("%s: %s" % (json.dumps(n), json.dumps(rec[n], sort_keys=True)))
            dig[label] = dict({"cases": len(rec)}, **{k: {"cases": len(v), "sha256": hashlib.sha256("\n".join(v).encode()).hexdigest()}
                                                       for k, v in kinds.items()})
            dig[label].update({n: rec[n] for n in rec if n.endswith("| delta")})
        with open(a.digest, "w") as f:                       # one line per kind and per delta
            f.write("{\n" + ",\n".join(' "%s": {\n%s\n }' % (label, ",\n".join('  %s: %s' % (json.dumps(n), json.dumps(d[n], sort_keys=True)) for n in sorted(d)))
                                      for label, d in sorted(dig.items())) + "\n}\n")
    if "parent" in out and "branch" in out:
        if sorted(out["parent"]) != sorted(out["branch"]):
            raise SystemExit("als_host_refactor_bits: the two records hold different cases")
        bad = [n for n in sorted(out["parent"]) if out["parent"][n] != out["branch"][n]]
        for n in bad:
            print("DIFFERENT: %s\n  parent %s\n  branch %s" % (n, out["parent"][n], out["branch"][n]))
        if bad:
            raise SystemExit("als_host_refactor_bits: %d of %d cases differ" % (len(bad), len(out["parent"])))
        print("parent and branch are equal on all %d cases" % len(out["parent"]))


if __name__ == "__main__":
    main()
