"""The logistic loss of the ALS solver on every route on the device (cmf_set_logit_pass, cmf_als_logit_weights, every step and row
entry under the flag, CMF(als_logit_pass=True)) against the float64 yardsticks logit_pass_yardstick.py / logit_yardstick.py on
float32-rounded inputs.  Tolerance per comparison (als_yardstick.tolerance, the HALS rule): tol = max(4 max|y32 - y64|,
(k + 16) 2^-24 max|y64|), y32 the float32 run of the same yardstick.  The problem is als_dual_cases.py (X 48 x 160 with rows of 0, 1,
2, 31, 32, 33, 100 and 160 entries among others, stored exact-zero weights, Y observed too) with the labels X > 0, Y > 0, at k = 3,
40, 100, 200 (k_pad 32, 64, 128, 256), and one relation of 3 x 2100 whose full row is more than one piece of 2048.

Measured on an MI355X: the worst |err| / tol of each route is recorded in DESIGN section 29."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_dual_cases as C
import als_dual_yardstick as D
import als_yardstick as A
import logit_pass_yardstick as LP
import logit_yardstick as L
import nncg_yardstick as N
from test_gpu_als import _bind, _context, _f32

pytestmark = pytest.mark.gpu

NAMES = "UVZ"
BITS = {"U": A.U_BIT, "V": A.V_BIT, "Z": A.Z_BIT}
KS = [3, 40, 100, 200]
L2 = C.L2
BOTH = (True, True)


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _reset(ctx, F):
    for w in range(3):
        ctx.set_factor(w, F[w])


def _bits(ctx):
    return [ctx.get_factor(w).astype(np.float32).tobytes() for w in range(3)]


def _order(rel):
    """pattern order -> stored order of the transpose"""
    return np.lexsort((rel.r, rel.c))


def _labels(k):
    """als_dual_cases.problem(k) with the labels X > 0, Y > 0."""
    X, Y, Wx, Wy, F = C.problem(k)
    return (X > 0).astype(np.float64), (Y > 0).astype(np.float64), Wx, Wy, F


def _passed(lib, X, Y, F, Wx, Wy, which=(0, 1), **kw):
    """A context with the relations ``which`` logistic and their flag on."""
    ctx = _context(lib, X, Y, F, Wx, Wy, **kw)
    for w in which:
        ctx.set_relation_loss(w, "logistic")
        ctx.set_logit_pass(w, True)
    return ctx


def _check(what, got, y32, y64, k, worst):
    tol = A.tolerance(y32, y64, k)
    err = float(np.abs(got - y64).max())
    worst[what.split(":")[0]] = max(worst.get(what.split(":")[0], 0.0), err / tol)
    print("%s: |err| / tol %.3f (tol %.3e)" % (what, err / tol, tol))
    assert np.isfinite(got).all() and err <= tol, (what, err, tol)


# ------------------------------------------------------------------ 1. the pass, exactly
def _exact_problem(k, long_row=False):
    """Every score is 0: the rows of U and Z live on the first column, the rows of V on the others (some rows are zero).  Dyadic
    weights with the stored zeros kept, labels 0 / 1: w / 4 and w t - w / 2 are float32 numbers."""
    rng = np.random.RandomState(200 + k + (1000 if long_row else 0))
    if long_row:
        m, d, p = 3, 2100, 2
        Wx = np.zeros((m, d))
        Wx[0, :] = 1.0                                                    # the full row: 2100 entries, two pieces
        Wx[1, rng.choice(d, 40, replace=False)] = 1.0
        Wx[2, 5] = 1.0
        Wx = sp.csr_matrix(Wx)
        Wy = sp.csr_matrix((rng.rand(d, p) < 0.02) * 1.0)
    else:
        (Wx, Wy), (m, d, p) = C.patterns(), (C.M, C.D, C.P)
        Wx, Wy = Wx.copy(), Wy.copy()
    for W in (Wx, Wy):
        W.data = np.where(W.data == 0, 0.0, rng.choice([0.25, 0.5, 0.75, 1.0, 1.5, 3.0], W.nnz))   # (the stored zeros stay)
    F = [np.zeros((n, k)) for n in (m, d, p)]
    F[0][:, 0] = rng.randint(-3, 4, m)
    F[2][:, 0] = rng.randint(-3, 4, p)
    F[1][:, 1:] = rng.randint(-3, 4, (d, k - 1)) * (rng.rand(d, 1) < 0.9)
    X, Y = (rng.rand(m, d) < 0.5).astype(np.float64), (rng.rand(d, p) < 0.5).astype(np.float64)
    return X, Y, Wx, Wy, F


@pytest.mark.parametrize("k, long_row", [(k, False) for k in KS] + [(40, True)])
def test_the_pass_is_exact_where_every_score_is_zero(lib, k, long_row):
    X, Y, Wx, Wy, F = _exact_problem(k, long_row)
    ctx = _passed(lib, X, Y, F, Wx, Wy)
    for which, (T, W, Fa, Fb) in enumerate(((X, Wx, F[0], F[1]), (Y, Wy, F[1], F[2]))):
        assert ctx.get_logit_pass(which) is True
        rel = A.Relation(T, W)
        assert (LP.scores(rel, Fa, Fb) == 0).all() and np.abs(Fa).max() > 0 and np.abs(Fb).max() > 0
        hw, hp = rel.w / 4, rel.w * rel.t - rel.w / 2
        assert (np.float32(hw) == hw).all() and (np.float32(hp) == hp).all()      # the float64 values ARE float32 numbers
        got = {}
        for image, order in ((0, slice(None)), (1, _order(rel))):
            got_w, got_p = ctx.als_logit_weights(which, image, rel.w.size)
            assert (got_w == hw[order]).all() and (got_p == hp[order]).all(), (which, image)
            assert (got_w[rel.w[order] == 0] == 0).all() and (rel.w == 0).sum() == (0 if long_row else 25)
            again = ctx.als_logit_weights(which, image, rel.w.size)
            assert got_w.tobytes() == again[0].tobytes() and got_p.tobytes() == again[1].tobytes()
            got[image] = got_w.tobytes()
        lens = rel.row_lengths(False)
        if long_row and which == 0:
            assert lens[0] == 2100 > 2048                                         # across the piece boundary
        else:
            assert long_row or {0, 1, 2, 31, 32, 33, 100, 160} <= set(lens) or which == 1
        ctx.set_factor(which, -F[which])                                          # kappa is even: the negated row factor, the same bytes
        assert all(ctx.als_logit_weights(which, image, rel.w.size)[0].tobytes() == got[image] for image in (0, 1))
        ctx.set_factor(which, F[which])
        with pytest.raises(ValueError, match="the caller's buffers hold"):
            ctx.als_logit_weights(which, 0, rel.w.size + 1)
    ctx.close()


# ------------------------------------------------------------------ 2. the pass on random data
@pytest.mark.parametrize("k", KS)
def test_the_pass_on_random_data_and_the_loss_does_not_see_it(lib, k):
    X, Y, Wx, Wy, F = _labels(k)
    # the factors of als_dual_cases (entries of variance 1 / k, scores of variance 1 / k) scaled so that the SCORES are scaled to a
    # standard deviation of 3 at every k: |s| up to about 10, kappa from 1/4 down to about 0.05
    F = [_f32(np.sqrt(3.0) * k ** 0.25 * M) for M in F]
    ctx = _passed(lib, X, Y, F, Wx, Wy)
    worst = 0.0
    before = ctx.als_logistic_loss()
    for which, (T, W, Fa, Fb) in enumerate(((X, Wx, F[0], F[1]), (Y, Wy, F[1], F[2]))):
        rel = A.Relation(T, W)
        kap = L.kappa(LP.scores(rel, Fa, Fb))
        print("k %d relation %d: |s| up to %.1f, kappa in [%.4f, %.4f]" % (k, which, np.abs(LP.scores(rel, Fa, Fb)).max(), kap.min(), kap.max()))
        assert kap.max() >= 2 * kap.min()
        (w64, p64), (w32, p32) = (LP.weights(rel, Fa, Fb, dt) for dt in (np.float64, np.float32))
        for image, order in ((0, slice(None)), (1, _order(rel))):
            got_w, got_p = ctx.als_logit_weights(which, image, rel.w.size)
            for name, got, y32, y64 in (("w_eff", got_w, w32, w64), ("p_eff", got_p, p32, p64)):
                tol = A.tolerance(y32.astype(np.float64), y64, k)
                err = float(np.abs(got - y64[order]).max())
                worst = max(worst, err / tol)
                print("k %d relation %d image %d %s: |err| / tol %.3f (tol %.3e)" % (k, which, image, name, err / tol, tol))
                assert err <= tol, (which, image, name, err, tol)
            assert (got_w[rel.w[order] == 0] == 0).all()                          # a stored zero weight stays one
    print("k %d: pass worst |err| / tol %.3f" % (k, worst))
    assert ctx.als_logistic_loss() == before                                      # the bound arrays do not leak
    want = (L.loss(A.Relation(X, Wx), F[0], F[1]), L.loss(A.Relation(Y, Wy), F[1], F[2]))
    assert all(abs(g - w) <= 1e-6 * w for g, w in zip(before, want))
    ctx.als_step(L2, 0, 2)                                                        # ... nor after a sweep that had them bound
    _reset(ctx, F)
    assert ctx.als_logistic_loss() == before
    ctx.close()


# ------------------------------------------------------------------ 3. every route, one sweep at a time
ROUTES = {"exact": dict(), "nnls": dict(non_negative=True, nn_sweeps=3), "cg": dict(cg_steps=3), "dual": dict(dual_max=128)}


@pytest.mark.parametrize("k", KS)
def test_rows_of_every_route_against_the_yardstick(lib, k):
    """Row entries and single sweeps (masks 1, 2, 4), X and Y both logistic with the flag on."""
    X, Y, Wx, Wy, F = _labels(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    ctx = _passed(lib, X, Y, F, Wx, Wy)
    worst = {}
    for which in NAMES:
        w = NAMES.index(which)
        n = F[w].shape[0]
        for route, kw in ROUTES.items():
            nn = BITS[which] if kw.get("non_negative") else 0
            Fs = [np.abs(M) for M in F] if nn else F                              # (coordinate descent starts at a feasible row)
            _reset(ctx, Fs)
            y64, y32 = (LP.sweep(Rx, Ry, *Fs, which, L2, logit=BOTH, dtype=dt, **kw) for dt in (np.float64, np.float32))
            call = {"exact": lambda: ctx.als_step(L2, nn, BITS[which]), "nnls": lambda: ctx.als_nnls_step(L2, nn, BITS[which], 3),
                    "cg": lambda: ctx.als_cg_step(L2, nn, BITS[which], 3), "dual": lambda: ctx.als_dual_step(L2, nn, BITS[which], 128)}[route]
            call()
            stepped = ctx.get_factor(w)
            others = [ctx.get_factor(v).astype(np.float32).tobytes() == np.float32(Fs[v]).tobytes() for v in range(3) if v != w]
            _reset(ctx, F)
            assert all(others)
            _check("%s: k %d sweep %s (step)" % (route, k, which), stepped, y32, y64, k, worst)
            if route == "cg":
                got = ctx.als_cg_rows(w, 0, n, L2, 3)
                assert (got[:, k:] == 0).all()
                _check("cg: k %d sweep %s (rows)" % (k, which), got[:, :k], y32, y64, k, worst)
            if route == "dual":
                got = ctx.als_dual_rows(w, 0, n, L2, 128)
                assert (got[:, k:] == 0).all()
                assert got[:, :k].astype(np.float32).tobytes() == stepped.astype(np.float32).tobytes()   # the step writes what the entry returns
                last = ctx.als_dual_last()
                assert last == D.counts(D.plan(Rx, Ry, which, k, 128)), (which, last)
                if which == "U" and k >= 100:                                     # rows in every class below k_pad
                    assert all(last[q] > 0 for q in range(3) if (32 << q) < D.k_pad(k)), last
            if route == "exact":                                                  # cmf_als_normal: the majoriser's systems at the current rows
                Hd, gd = ctx.als_normal(w, 0, n, L2)
                (H64, g64), (H32, g32) = (L.systems(Rx, Ry, *F, which, L2, logit=BOTH, dtype=dt) for dt in (np.float64, np.float32))
                _check("normal: k %d sweep %s H" % (k, which), Hd[:, :k, :k], H32, H64, k, worst)
                _check("normal: k %d sweep %s g" % (k, which), gd[:, :k], g32, g64, k, worst)
        # projected CG on |F|: the rows whose float32 and float64 yardstick runs take the same decisions with a margin of at least
        # 1e-3 (the rule of test_gpu_als_nncg.py: a decision at its threshold is no parity case)
        Fa = [np.abs(M) for M in F]
        _reset(ctx, Fa)
        Rw = [(LP.reweighted(Rx, Fa[0], Fa[1], dt), LP.reweighted(Ry, Fa[1], Fa[2], dt)) for dt in (np.float64, np.float32)]
        (y64, t64, m64, _), (y32, t32, m32, _) = (N.rows(*Rw[i], *Fa, which, L2, 3, dtype=dt) for i, dt in enumerate((np.float64, np.float32)))
        sel = np.array([a == b for a, b in zip(t64, t32)]) & (np.minimum(m64, m32) >= 1e-3)
        got = ctx.als_nncg_rows(w, 0, n, L2, 3)[:, :k]
        print("nncg: k %d sweep %s: %d of %d rows are parity cases" % (k, which, int(sel.sum()), n))
        assert sel.sum() >= n // 4 and (got >= 0).all()
        _check("nncg: k %d sweep %s (rows)" % (k, which), got[sel], y32[sel], y64[sel], k, worst)
        ctx.als_nncg_step(L2, BITS[which], BITS[which], 0, 3)                     # the same sweep as a step: masks 1, 2, 4
        stepped = ctx.get_factor(w)
        _reset(ctx, F)
        _check("nncg: k %d sweep %s (step)" % (k, which), stepped[sel], y32[sel], y64[sel], k, worst)
    print("k %d: worst |err| / tol per route: %s" % (k, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    ctx.close()


# ------------------------------------------------------------------ 4. CG rows cut into pieces
@pytest.mark.parametrize("k", [40, 200])
def test_cg_rows_cut_into_pieces(lib, k):
    X, Y, Wx, Wy, F = _labels(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    ctx = _passed(lib, X, Y, F, Wx, Wy)
    ctx.set_option("als_cg_piece", 64)
    worst = {}
    for which in NAMES:
        w = NAMES.index(which)
        y64, y32 = (LP.sweep(Rx, Ry, *F, which, L2, logit=BOTH, cg_steps=3, dtype=dt) for dt in (np.float64, np.float32))
        got = ctx.als_cg_rows(w, 0, F[w].shape[0], L2, 3)
        nlong, npieces = ctx.als_cg_last()
        print("k %d sweep %s: %d long rows in %d pieces" % (k, which, nlong, npieces))
        assert nlong >= 3 and npieces > nlong                                     # (the rows of 100 and more entries are cut)
        _check("cg pieces: k %d sweep %s" % (k, which), got[:, :k], y32, y64, k, worst)
    ctx.als_cg_step(L2, 0, 1, 3)                                                  # the sweep through the step, cut in the same way
    y64, y32 = (LP.sweep(Rx, Ry, *F, "U", L2, logit=BOTH, cg_steps=3, dtype=dt) for dt in (np.float64, np.float32))
    _check("cg pieces: k %d step U" % k, ctx.get_factor(0), y32, y64, k, worst)
    ctx.close()


# ------------------------------------------------------------------ 5. whole steps, mask 7
STEPS = {"cg": (dict(cg_steps=3), 0, lambda c: c.als_cg_step(L2, 0, 7, 3)), "nnls": (dict(nn_sweeps=3), 7, lambda c: c.als_nnls_step(L2, 7, 7, 3)),
         "dual": (dict(dual_max=128), 0, lambda c: c.als_dual_step(L2, 0, 7, 128))}


@pytest.mark.parametrize("route", sorted(STEPS))
def test_whole_steps_with_x_passed_and_y_frobenius(lib, route):
    """Mask 7 (V, U, Z, each sweep behind its own pass at the factors the sweeps before it left): X logistic with the flag on, Y
    observed Frobenius."""
    k = 40
    X, _, Wx, Wy, F = _labels(k)
    Y = C.problem(k)[1]
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    kw, nn, call = STEPS[route]
    Fs = [np.abs(M) for M in F] if nn else F
    ctx = _passed(lib, X, Y, Fs, Wx, Wy, which=(0,))
    ctx.set_logit_pass(1, True)                                                   # (on a Frobenius relation the flag does nothing)
    ref = {dt: LP.step(Rx, Ry, *Fs, L2, logit=(True, False), nn_mask=nn, dtype=dt, **kw) for dt in (np.float64, np.float32)}
    call(ctx)
    worst = {}
    for w in range(3):
        _check("%s: mask 7 factor %s" % (route, NAMES[w]), ctx.get_factor(w), ref[np.float32][w], ref[np.float64][w], k, worst)
    ctx.close()


@pytest.mark.parametrize("route", ["exact", "nnls", "dual"])
def test_whole_steps_with_x_passed_and_y_fused(lib, route):
    """Mask 7 and the V sweep alone, X logistic with the flag on, Y logistic with it off: the V sweep reads the arrays of the pass
    on its X side and reweights its Y side inside the normal-equation kernel, in one launch.  (The CG steps refuse the fused Y as
    they always did; under dual_max the sweeps that read Y keep the exact rows, U goes dual.)"""
    k = 40
    X, Y, Wx, Wy, F = _labels(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    nn = 7 if route == "nnls" else 0
    Fs = [np.abs(M) for M in F] if nn else F
    ctx = _passed(lib, X, Y, Fs, Wx, Wy, which=(0,))
    ctx.set_relation_loss(1, "logistic")
    assert (ctx.get_logit_pass(0), ctx.get_logit_pass(1)) == (True, False)
    call = {"exact": lambda m: ctx.als_step(L2, 0, m), "nnls": lambda m: ctx.als_nnls_step(L2, 7, m, 3),
            "dual": lambda m: ctx.als_dual_step(L2, 0, m, 128)}[route]

    def sweep(Fc, which, dt):
        if which == "U":
            kw = dict(non_negative=True, nn_sweeps=3) if nn else (dict(dual_max=128) if route == "dual" else dict())
            return LP.sweep(Rx, Ry, *Fc, "U", L2, logit=(True, False), dtype=dt, **kw)
        return L.sweep(LP.reweighted(Rx, Fc[0], Fc[1], dt), Ry, *Fc, which, L2, logit=(False, True), non_negative=bool(nn), nn_sweeps=3 if nn else 0,
                       dtype=dt)
    worst = {}
    for mask in (2, 7):
        ref = {}
        for dt in (np.float64, np.float32):
            Fc = [np.array(M, dtype=dt) for M in Fs]
            for which in "VUZ":
                if mask & BITS[which]:
                    Fc[NAMES.index(which)] = sweep(Fc, which, dt)
            ref[dt] = Fc
        call(mask)
        for w in range(3):
            _check("%s: Y fused mask %d factor %s" % (route, mask, NAMES[w]), ctx.get_factor(w), ref[np.float32][w], ref[np.float64][w], k, worst)
        _reset(ctx, Fs)
    for refused in (lambda: ctx.als_cg_step(L2, 0, 7, 3), lambda: ctx.als_cg_rows(1, 0, 5, L2, 3)):
        with pytest.raises(NotImplementedError, match="Y has a logistic loss; the conjugate-gradient rows have no reweighting pass"):
            refused()
    with pytest.raises(NotImplementedError, match="Y has a logistic loss; the non-negative conjugate-gradient rows"):
        ctx.als_nncg_step(L2, 7, 7, 0, 3)
    with pytest.raises(ValueError, match="not eligible: a logistic relation"):
        ctx.als_dual_rows(2, 0, 5, L2, 128)
    ctx.als_cg_rows(0, 0, 5, L2, 3)                                               # the U sweep reads the passed X alone
    ctx.close()


# ------------------------------------------------------------------ 6. pass against fused
@pytest.mark.parametrize("k", KS)
def test_the_exact_route_with_the_pass_and_fused(lib, k):
    """Both forms of the exact step within tolerance of logit_yardstick.sweep; they need not share bits (the score is summed over
    other lane groups)."""
    X, Y, Wx, Wy, F = _labels(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    fused = _context(lib, X, Y, F, Wx, Wy)
    for w in (0, 1):
        fused.set_relation_loss(w, "logistic")
    passed = _passed(lib, X, Y, F, Wx, Wy)
    worst = {}
    for which in NAMES:
        w = NAMES.index(which)
        y64, y32 = (L.sweep(Rx, Ry, *F, which, L2, logit=BOTH, dtype=dt) for dt in (np.float64, np.float32))
        for name, ctx in (("fused", fused), ("pass", passed)):
            ctx.als_step(L2, 0, BITS[which])
            _check("%s: k %d sweep %s" % (name, k, which), ctx.get_factor(w), y32, y64, k, worst)
            _reset(ctx, F)
    print("k %d: worst |err| / tol: %s" % (k, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    fused.close()
    passed.close()


# ------------------------------------------------------------------ 7. nothing moves without the flag
def _calls(ctx, k):
    """name -> bytes of what every step and row entry gives from the start factors (Frobenius relations)"""
    F = C.problem(k)[4]
    out = {}
    steps = {"als_step": lambda: ctx.als_step(L2, 0, 7), "als_step nn": lambda: ctx.als_step(L2, 7, 7),
             "als_nnls_step": lambda: ctx.als_nnls_step(L2, 7, 7, 3), "als_cg_step": lambda: ctx.als_cg_step(L2, 0, 7, 3),
             "als_nncg_step": lambda: ctx.als_nncg_step(L2, 5, 7, 2, 3), "als_dual_step": lambda: ctx.als_dual_step(L2, 0, 7, 128)}
    for name, call in steps.items():
        _reset(ctx, F)
        call()
        out[name] = _bits(ctx)
    _reset(ctx, F)
    for w in range(3):
        n = F[w].shape[0]
        out["cg rows %d" % w] = ctx.als_cg_rows(w, 0, n, L2, 3).tobytes()
        out["nncg rows %d" % w] = ctx.als_nncg_rows(w, 0, n, L2, 3).tobytes()
        out["dual rows %d" % w] = ctx.als_dual_rows(w, 0, n, L2, 128).tobytes()
        out["normal %d" % w] = b"".join(a.tobytes() for a in ctx.als_normal(w, 1, n - 2, L2))
    return out


def _fused_calls(ctx, k):
    """... with X and Y fused-logistic: the entry points that take them"""
    F = C.problem(k)[4]
    out = {}
    steps = {"als_step": lambda: ctx.als_step(L2, 0, 7), "als_nnls_step": lambda: ctx.als_nnls_step(L2, 7, 7, 3),
             "als_dual_step": lambda: ctx.als_dual_step(L2, 0, 7, 128)}
    for name, call in steps.items():
        _reset(ctx, F)
        call()
        out[name] = _bits(ctx)
    _reset(ctx, F)
    for w in range(3):
        out["normal %d" % w] = b"".join(a.tobytes() for a in ctx.als_normal(w, 1, F[w].shape[0] - 2, L2))
    out["loss"] = ctx.als_logistic_loss()
    return out


def _same(got, want):
    assert sorted(got) == sorted(want) and all(got[n] == want[n] for n in want), [n for n in want if got[n] != want[n]]


@pytest.mark.parametrize("k", [3, 100])
def test_nothing_moves_without_the_flag(lib, k):
    X, Y, Wx, Wy, F = C.problem(k)
    Xl, Yl = _labels(k)[:2]
    plain = _context(lib, X, Y, F, Wx, Wy)                                        # a context that never hears of the flag
    want = _calls(plain, k)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    for which in (0, 1):                                                          # the flag on Frobenius relations: every bit as without it
        ctx.set_logit_pass(which, True)
        assert ctx.get_logit_pass(which) is True and ctx.get_relation_loss(which) == 0
    _same(_calls(ctx, k), want)
    for which in (0, 1):                                                          # made logistic the flag acts (set before the loss) ...
        ctx.set_relation_loss(which, "logistic")
    _reset(ctx, F)
    ctx.als_cg_step(L2, 0, 7, 3)
    assert _bits(ctx) != want["als_cg_step"]
    for which in (0, 1):                                                          # ... and with both taken back nothing is left of it
        ctx.set_logit_pass(which, False)
        ctx.set_relation_loss(which, "frobenius")
        assert ctx.get_logit_pass(which) is False
    _same(_calls(ctx, k), want)
    for which in (0, 1):                                                          # arrays and piece lists built and used, then set_problem:
        ctx.set_relation_loss(which, "logistic")                                  # the flags are cleared, and the same context bound again
        ctx.set_logit_pass(which, True)                                           # is one that never heard of them
    ctx.als_step(L2, 0, 7)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], k)
    assert not ctx.get_logit_pass(0) and not ctx.get_logit_pass(1)
    _bind(ctx, 0, X, Wx)
    _bind(ctx, 1, Y, Wy)
    _reset(ctx, F)
    _same(_calls(ctx, k), want)
    ctx.close()
    plain.close()
    # fused logistic relations: a context that had the flag and gave it back against one that never set it
    plain = _context(lib, Xl, Yl, F, Wx, Wy)
    ctx = _context(lib, Xl, Yl, F, Wx, Wy)
    for which in (0, 1):
        plain.set_relation_loss(which, "logistic")
        ctx.set_relation_loss(which, "logistic")
        ctx.set_logit_pass(which, True)
    ctx.als_cg_step(L2, 0, 7, 3)
    for which in (0, 1):
        ctx.set_logit_pass(which, 0)
    want = _fused_calls(plain, k)
    _same(_fused_calls(ctx, k), want)
    for refused in (lambda: ctx.als_cg_step(L2, 0, 7, 3), lambda: ctx.als_cg_rows(0, 0, 5, L2, 3)):
        with pytest.raises(NotImplementedError, match="conjugate-gradient"):
            refused()
    for refused in (lambda: ctx.als_nncg_step(L2, 7, 7, 0, 3), lambda: ctx.als_dual_step(L2, 7, 7, 128, 0, 3)):
        with pytest.raises(NotImplementedError, match="X has a logistic loss; the non-negative conjugate-gradient rows"):
            refused()
    with pytest.raises(ValueError, match="not eligible: a logistic relation"):
        ctx.als_dual_rows(0, 0, 5, L2, 128)
    with pytest.raises(ValueError, match="cmf_set_logit_pass first"):
        ctx.als_logit_weights(0, 0, Wx.nnz)
    r = np.repeat(np.arange(Wx.shape[0]), np.diff(Wx.indptr))
    ctx.set_logit_pass(0, True)
    ctx.set_weighted_csr(0, Wx.indptr, Wx.indices, Xl[r, Wx.indices], Wx.data)   # binding the weights again keeps the flag
    assert ctx.get_logit_pass(0) is True
    _reset(ctx, F)
    ctx.als_cg_step(L2, 0, 1, 3)
    ctx.close()
    plain.close()


def test_refusals_that_stay_by_their_message(lib):
    k = 40
    X, Y, Wx, Wy, F = _labels(k)
    Wp = Wx.copy()
    Wp.data = np.where(Wp.data == 0, 0.75, Wp.data)
    ctx = _passed(lib, X, Y, F, Wp, Wy, which=(0,))
    for bad in (2, -1):
        with pytest.raises(ValueError, match="which must be 0"):
            ctx.set_logit_pass(bad, True)
        with pytest.raises(ValueError, match="which must be 0"):
            ctx.get_logit_pass(bad)
    with pytest.raises(ValueError, match="Y has no logistic loss"):
        ctx.als_logit_weights(1, 0, Wy.nnz)
    with pytest.raises(ValueError, match="kind must be"):
        ctx.set_relation_loss(0, 2)
    every = [lambda: ctx.als_step(L2, 0, 7), lambda: ctx.als_cg_step(L2, 0, 1, 3), lambda: ctx.als_nncg_step(L2, 7, 2, 0, 3),
             lambda: ctx.als_dual_step(L2, 0, 7, 128), lambda: ctx.als_cg_rows(0, 0, 5, L2, 3), lambda: ctx.als_normal(1, 0, 5, L2),
             lambda: ctx.als_logit_weights(0, 0, Wp.nnz)]
    with pytest.raises(NotImplementedError, match="a swept relation has a logistic loss .*; biases under a logit link are not built"):
        ctx.als_bias_step(L2, 0, 7)
    ctx.set_biases(0, True, 0.5, 0.1)
    for call in every + [lambda: ctx.als_bias_step(L2, 0, 7)]:
        with pytest.raises(NotImplementedError, match="X has a logistic loss and biases; biases under a logit link are not built"):
            call()
    ctx.set_biases(0, False)
    ctx.set_background_weight(0, 0.25)
    for call in every:
        with pytest.raises(NotImplementedError, match="X has a logistic loss and a background weight"):
            call()
    ctx.als_step(L2, 0, 4)                                                        # the Z sweep does not read X
    ctx.set_background_weight(0, 0.0)
    ctx.set_huber_delta(0, 1.0)
    for call in every:
        with pytest.raises(NotImplementedError, match="X has a Huber loss and a logistic loss"):
            call()
    ctx.set_huber_delta(0, 0)
    ctx.set_data(0, X)
    ctx.set_weight(0, np.asarray(Wp.toarray() > 0, dtype=np.float64))             # a dense weight
    for call in every[:-1]:
        with pytest.raises(NotImplementedError, match="X has a logistic loss .* and no CSR weights bound"):
            call()
    _bind(ctx, 0, X, Wp)
    _reset(ctx, F)
    ctx.als_cg_step(L2, 0, 7, 3)                                                  # usable, and under the loss
    assert all(np.isfinite(ctx.get_factor(w)).all() for w in range(3))
    ctx.close()


# ------------------------------------------------------------------ 8. descent on the device
DESCENT = {"cg": (4, 0, dict(cg_steps=3), lambda c, l2, nn: c.als_cg_step(l2, nn, 7, 3)),
           "nncg": (4, 7, dict(nn_cg_steps=3, nn_sweeps=4), lambda c, l2, nn: c.als_nncg_step(l2, nn, 7, 0, 3, 4)),
           "dual": (40, 0, dict(dual_max=128), lambda c, l2, nn: c.als_dual_step(l2, nn, 7, 128))}


@pytest.mark.parametrize("route", sorted(DESCENT))
def test_ten_device_iterations_never_raise_the_objective(lib, route):
    """logit_yardstick.planted(3), X logistic with the flag on, Y full: the float64 objective of the downloaded factors satisfies
    J' <= J + (k + 16) 2^-24 |J|; after 10 iterations the CG objective is within 1e-3 relative of the yardstick's after 10."""
    k, nn, kw, call = DESCENT[route]
    pr = L.planted(3)
    Rx, Ry = L.Relation(pr["T"], pr["Wsp"]), L.Relation(_f32(pr["Y"]), None)
    if k == pr["k"]:
        F = [_f32(np.abs(M) if nn else M) for M in pr["start"]]
    else:
        rng = np.random.RandomState(3 + 100)
        F = [_f32(0.1 * rng.randn(n, k)) for n in (pr["m"], pr["d"], pr["p"])]
    ctx = _passed(lib, pr["T"], _f32(pr["Y"]), F, pr["Wsp"], None, which=(0,))
    trace = [LP.objective(Rx, Ry, *F, pr["l2"])]
    for _ in range(10):
        call(ctx, pr["l2"], nn)
        trace.append(LP.objective(Rx, Ry, *[ctx.get_factor(w) for w in range(3)], pr["l2"]))
    ctx.close()
    print("device objective (%s): %s" % (route, " ".join("%.2f" % v for v in trace)))
    for a, b in zip(trace, trace[1:]):
        assert b <= a + (k + 16) * 2.0 ** -24 * abs(a)
    assert trace[-1] < 0.8 * trace[0]
    if route == "cg":
        ref = []
        LP.fit(Rx, Ry, *F, 10, pr["l2"], trace=ref, **kw)
        print("yardstick objective (cg): %s" % " ".join("%.2f" % v for v in ref))
        assert abs(trace[-1] - ref[-1]) <= 1e-3 * ref[-1]


# ------------------------------------------------------------------ 9. the estimator
def test_estimator_against_the_yardstick(lib):
    from pycmf_amd import CMF
    from pycmf_amd.factor_init import init_custom
    pr = L.planted(3)
    T, Y, W = pr["T"], _f32(pr["Y"]), pr["Wsp"]
    Rx, Ry = L.Relation(T, W), L.Relation(Y, None)
    start = [_f32(M) for M in pr["start"]]
    kw = dict(n_components=pr["k"], solver="als", loss="logistic", x_link="logit", l2_reg=pr["l2"], max_iter=15, tol=0.0, x_init="custom",
              y_init="custom", random_state=0, U_non_negative=False, V_non_negative=False, Z_non_negative=False)
    model = CMF(als_logit_pass=True, als_cg_steps=6, **kw)
    U, V, Z = model.fit_transform(T, Y, U=start[0].copy(), V=start[1].copy(), Z=start[2].copy(), x_entry_weights=W)
    ref = LP.fit(Rx, Ry, *start, 15, pr["l2"], cg_steps=6)
    want = L.loss(Rx, ref[0], ref[1]) + np.sqrt(A.residual_sq(Ry, ref[1], ref[2]))
    print("reconstruction_err_ %.6f, yardstick %.6f, relative %.2e" % (model.reconstruction_err_, want, abs(model.reconstruction_err_ - want) / want))
    assert model.n_iter_ == 15 and abs(model.reconstruction_err_ - want) <= 1e-4 * want
    lx, ly = model.logistic_loss_
    assert ly == 0.0 and abs(lx - L.loss(Rx, U, V)) <= 1e-6 * lx
    exact = CMF(**kw)
    Ue, Ve, _ = exact.fit_transform(T, Y, U=start[0].copy(), V=start[1].copy(), Z=start[2].copy(), x_entry_weights=W)
    got, base = L.agreement(U, V, pr), L.agreement(Ue, Ve, pr)
    print("agreement on the unobserved cells: pass + 6 CG steps %.3f, exact fused %.3f" % (got, base))
    assert abs(got - base) <= 0.01
    # fold-in of held-out rows against the fitted V under the option: the yardstick's fold-in from transform's own start
    sel = np.arange(0, pr["m"], 4)
    Xn, Wn = T[sel], sp.csr_matrix(W[sel])
    model.set_params(max_iter=5)
    Un, Vn, Zn = model.transform(Xn, None, x_entry_weights=Wn)
    assert (Vn == V).all() and (Zn == Z).all()
    Rn = L.Relation(Xn, Wn)
    U0 = _f32(init_custom(None, Xn, pr["k"], 0, non_negative=False, random_state=0))
    y64, y32 = (LP.fit(Rn, Ry, U0, _f32(V), _f32(Z), 5, pr["l2"], mask=A.U_BIT, cg_steps=6, dtype=dt)[0] for dt in (np.float64, np.float32))
    tol = A.tolerance(y32, y64, pr["k"])
    err = float(np.abs(Un - y64).max())
    print("transform |err| / tol %.3f (tol %.3e)" % (err / tol, tol))
    assert err <= tol
