"""The Huber loss of the ALS solver on the device (cmf_set_huber_delta, cmf_als_huber_weights, cmf_als_huber_loss, every step and row
entry under a delta, CMF(x_huber_delta=...)) against the float64 yardstick huber_yardstick.py on float32-rounded inputs.  Tolerance
per comparison (als_yardstick.tolerance, the HALS rule): tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|), y32 the float32 run of
the same yardstick.  The problem is als_dual_cases.py (X 48 x 160 with rows of 0, 1, 2, 31, 32, 33, 100 and 160 entries among others,
stored exact-zero weights, Y observed too) at k = 3, 40, 100, 200 (k_pad 32, 64, 128, 256), and one relation of 3 x 2100 whose full
row is more than one piece of 2048.

Measured on an MI355X: the worst |err| / tol of each route is recorded in DESIGN section 28."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_bias_yardstick as B
import als_dual_cases as C
import als_yardstick as A
import huber_yardstick as H
import nncg_yardstick as N
from test_gpu_als import _bind, _context, _f32

pytestmark = pytest.mark.gpu

NAMES = "UVZ"
BITS = {"U": A.U_BIT, "V": A.V_BIT, "Z": A.Z_BIT}
KS = [3, 40, 100, 200]
L2 = C.L2


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


# ------------------------------------------------------------------ 1. the pass, exactly
def _exact_problem(k, long_row=False):
    """Integer factors, weights with few mantissa bits and targets t = s + r with |r| in {0, d / 4, d / 2, d, 2 d, 4 d, 8 d}, d = 1/2:
    scores, residuals, omega = d / |r| and the products with it are exact in float32."""
    rng = np.random.RandomState(100 + k + (1000 if long_row else 0))
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
    F = [rng.randint(-2, 3, (n, k)).astype(np.float64) for n in (m, d, p)]
    delta = 0.5
    out = []
    for W, Fa, Fb in ((Wx, F[0], F[1]), (Wy, F[1], F[2])):
        r = delta * rng.choice([0.0, 0.25, 0.5, 1.0, 1.0, 2.0, 4.0, 8.0], W.shape) * rng.choice([-1.0, 1.0], W.shape)
        out.append(Fa @ Fb.T + r)
    return out[0], out[1], Wx, Wy, F, delta


@pytest.mark.parametrize("k, long_row", [(k, False) for k in KS] + [(40, True)])
def test_the_pass_is_exact_on_dyadic_residuals(lib, k, long_row):
    X, Y, Wx, Wy, F, delta = _exact_problem(k, long_row)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    seen = set()
    for which, (T, W, Fa, Fb) in enumerate(((X, Wx, F[0], F[1]), (Y, Wy, F[1], F[2]))):
        ctx.set_huber_delta(which, delta)
        assert ctx.get_huber_delta(which) == delta
        rel = A.Relation(T, W)
        r = H.residuals(rel, Fa, Fb)
        seen |= set(np.abs(r) / delta)
        om = H.omega(r, delta)
        hw = rel.w * om
        hp = (np.float32(rel.w) * np.float32(rel.t)).astype(np.float64) * om
        assert (np.float32(hw) == hw).all() and (np.float32(hp) == hp).all()      # the float64 values ARE float32 numbers
        for image, order in ((0, slice(None)), (1, _order(rel))):
            got_w, got_p = ctx.als_huber_weights(which, image, rel.w.size)
            assert (got_w == hw[order]).all() and (got_p == hp[order]).all(), (which, image)
            again = ctx.als_huber_weights(which, image, rel.w.size)
            assert got_w.tobytes() == again[0].tobytes() and got_p.tobytes() == again[1].tobytes()
        lens = rel.row_lengths(False)
        if long_row and which == 0:
            assert lens[0] == 2100 > 2048                                         # across the piece boundary
        else:
            assert long_row or {0, 1, 2, 31, 32, 33, 100, 160} <= set(lens) or which == 1
        with pytest.raises(ValueError, match="the caller's buffers hold"):
            ctx.als_huber_weights(which, 0, rel.w.size + 1)
    assert {0.0, 0.5, 1.0, 2.0, 8.0} <= seen                                      # r = 0, |r| below, AT and above delta
    ctx.close()


# ------------------------------------------------------------------ 2. the pass on random data
@pytest.mark.parametrize("k", KS)
def test_the_pass_and_the_loss_on_random_data(lib, k):
    X, Y, Wx, Wy, F = C.problem(k)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    worst = 0.0
    for which, (T, W, Fa, Fb, delta) in enumerate(((X, Wx, F[0], F[1], 1.0), (Y, Wy, F[1], F[2], 0.75))):
        ctx.set_huber_delta(which, delta)
        rel = A.Relation(T, W)
        w64, w32 = (H.reweighted(rel, Fa, Fb, delta, dt).w for dt in (np.float64, np.float32))
        assert 0.1 < (w64 != rel.w).mean() < 0.9                                  # both branches of omega
        p64 = w64 * rel.t
        p32 = (np.float32(w32) * np.float32(rel.t)).astype(np.float64)
        for image, order in ((0, slice(None)), (1, _order(rel))):
            got_w, got_p = ctx.als_huber_weights(which, image, rel.w.size)
            for name, got, y32, y64 in (("w_eff", got_w, w32, w64), ("p_eff", got_p, p32, p64)):
                tol = A.tolerance(y32, y64, k)
                err = float(np.abs(got - y64[order]).max())
                worst = max(worst, err / tol)
                print("k %d relation %d image %d %s: |err| / tol %.3f (tol %.3e)" % (k, which, image, name, err / tol, tol))
                assert err <= tol, (which, image, name, err, tol)
            assert (got_w[rel.w[order] == 0] == 0).all()                          # a stored zero weight stays one
    want = (H.loss(A.Relation(X, Wx), F[0], F[1], 1.0), H.loss(A.Relation(Y, Wy), F[1], F[2], 0.75))
    got = ctx.als_huber_loss()
    print("k %d: loss %r against %r, relative %.2e %.2e; pass worst |err| / tol %.3f" % (k, got, want, abs(got[0] - want[0]) / want[0],
                                                                                     abs(got[1] - want[1]) / want[1], worst))
    assert all(abs(g - w) <= 1e-6 * w for g, w in zip(got, want))
    assert ctx.als_huber_loss() == got and ctx.als_huber_loss(True, False) == (got[0], 0.0)
    ctx.set_huber_delta(1, 0)
    assert ctx.als_huber_loss() == (got[0], 0.0) and ctx.get_huber_delta(1) == 0.0
    ctx.close()


# ------------------------------------------------------------------ 3. a delta no residual reaches changes no bit
def _calls(ctx, k, biased=False):
    """name -> bytes of what every step and row entry gives from the start factors"""
    F = C.problem(k)[4]
    out = {}
    steps = {"als_step": lambda: ctx.als_step(L2, 0, 7), "als_step nn": lambda: ctx.als_step(L2, 7, 7),
             "als_nnls_step": lambda: ctx.als_nnls_step(L2, 7, 7, 3), "als_cg_step": lambda: ctx.als_cg_step(L2, 0, 7, 3),
             "als_nncg_step": lambda: ctx.als_nncg_step(L2, 5, 7, 2, 3), "als_dual_step": lambda: ctx.als_dual_step(L2, 0, 7, 128)}
    if biased:
        steps = {"als_bias_step": lambda: ctx.als_bias_step(L2, 0, 7), "als_bias_step cg": lambda: ctx.als_bias_step(L2, 0, 7, 3),
                 "als_dual_step": lambda: ctx.als_dual_step(L2, 0, 7, 128)}
    for name, call in steps.items():
        _reset(ctx, F)
        if biased:
            for axis in (0, 1):
                ctx.set_bias(0, axis, np.zeros((C.M, C.D)[axis]))
        call()
        out[name] = _bits(ctx) + ([ctx.get_bias(0, axis).tobytes() for axis in (0, 1)] if biased else [])
    _reset(ctx, F)
    if biased:
        out["bias rows"] = [ctx.als_bias_rows(0, axis).tobytes() for axis in (0, 1)]
        return out
    for w in range(3):
        n = F[w].shape[0]
        out["cg rows %d" % w] = ctx.als_cg_rows(w, 0, n, L2, 3).tobytes()
        out["nncg rows %d" % w] = ctx.als_nncg_rows(w, 0, n, L2, 3).tobytes()
        out["dual rows %d" % w] = ctx.als_dual_rows(w, 0, n, L2, 128).tobytes()
        out["normal %d" % w] = b"".join(a.tobytes() for a in ctx.als_normal(w, 1, n - 2, L2))
    return out


@pytest.mark.parametrize("k", [3, 100])
def test_a_delta_no_residual_reaches_keeps_every_bit(lib, k):
    X, Y, Wx, Wy, F = C.problem(k)
    plain = _context(lib, X, Y, F, Wx, Wy)
    want = _calls(plain, k)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    for which in (0, 1):
        ctx.set_huber_delta(which, 1e30)
    got = _calls(ctx, k)
    assert sorted(got) == sorted(want) and all(got[n] == want[n] for n in want), [n for n in want if got[n] != want[n]]
    ctx.set_huber_delta(0, 1.0)                                                   # a delta that acts does change the step ...
    ctx.als_step(L2, 0, 7)
    assert _bits(ctx) != want["als_step"]
    for which in (0, 1):                                                          # ... and taken back, nothing is left of it
        ctx.set_huber_delta(which, 0)
    got = _calls(ctx, k)
    assert all(got[n] == want[n] for n in want), [n for n in want if got[n] != want[n]]
    for which in (0, 1):                                                          # both relations under a delta that acts, their arrays,
        ctx.set_huber_delta(which, 1.0)                                           # piece lists and transposed targets built and used ...
    ctx.als_step(L2, 0, 7)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], k)               # ... then set_problem: the deltas are cleared, and the
    assert ctx.get_huber_delta(0) == 0.0 and ctx.get_huber_delta(1) == 0.0       # same context bound again is one that never heard of them
    _bind(ctx, 0, X, Wx)
    _bind(ctx, 1, Y, Wy)
    _reset(ctx, F)
    got = _calls(ctx, k)
    assert sorted(got) == sorted(want) and all(got[n] == want[n] for n in want), [n for n in want if got[n] != want[n]]
    ctx.close()
    ctx = _context(lib, X, Y, F, Wx, Wy)
    ctx.set_huber_delta(0, 1.0)
    r = np.repeat(np.arange(Wx.shape[0]), np.diff(Wx.indptr))
    ctx.set_weighted_csr(0, Wx.indptr, Wx.indices, X[r, Wx.indices], Wx.data)    # binding the weights again keeps it
    assert ctx.get_huber_delta(0) == 1.0
    ctx.als_step(L2, 0, 7)
    assert _bits(ctx) != want["als_step"]
    ctx.set_huber_delta(0, 0)
    _reset(ctx, F)
    ctx.als_step(L2, 0, 7)
    assert _bits(ctx) == want["als_step"]
    ctx.close()
    plain.close()


def test_a_delta_no_residual_reaches_keeps_every_bit_under_biases(lib):
    k = 40
    X, Y, Wx, Wy, F = C.problem(k)
    out = []
    for delta in (None, 1e30):
        ctx = _context(lib, X, Y, F, Wx, Wy)
        ctx.set_biases(0, True, 0.125, 0.5)
        if delta:
            ctx.set_huber_delta(0, delta)
            ctx.set_huber_delta(1, delta)
        out.append(_calls(ctx, k, biased=True))
        ctx.close()
    assert all(out[0][n] == out[1][n] for n in out[0]), [n for n in out[0] if out[0][n] != out[1][n]]


# ------------------------------------------------------------------ 4. each route at delta = 1 against the yardstick
def _check(what, got, y32, y64, k, worst):
    tol = A.tolerance(y32, y64, k)
    err = float(np.abs(got - y64).max())
    worst[what.split(":")[0]] = max(worst.get(what.split(":")[0], 0.0), err / tol)
    print("%s: |err| / tol %.3f (tol %.3e)" % (what, err / tol, tol))
    assert np.isfinite(got).all() and err <= tol, (what, err, tol)


ROUTES = {"exact": dict(), "nnls": dict(non_negative=True, nn_sweeps=3), "cg": dict(cg_steps=3),
          "dual": dict(dual_max=128)}


@pytest.mark.parametrize("k", KS)
def test_rows_of_every_route_against_the_yardstick(lib, k):
    """Row entries and single sweeps (masks 1, 2, 4) under delta = 1 on X and 0.75 on Y, both observed."""
    X, Y, Wx, Wy, F = C.problem(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    deltas = (1.0, 0.75)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    for which in (0, 1):
        ctx.set_huber_delta(which, deltas[which])
    worst = {}
    for which in NAMES:
        w = NAMES.index(which)
        n = F[w].shape[0]
        for route, kw in ROUTES.items():
            nn = BITS[which] if kw.get("non_negative") else 0
            Fs = [np.abs(M) for M in F] if nn else F                              # (coordinate descent starts at a feasible row)
            _reset(ctx, Fs)
            y64, y32 = (H.sweep(Rx, Ry, *Fs, which, L2, deltas=deltas, dtype=dt, **kw) for dt in (np.float64, np.float32))
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
            if route == "exact":                                                  # cmf_als_normal: the majoriser's systems at the current rows
                Hd, gd = ctx.als_normal(w, 0, n, L2)
                Rxw, Ryw = H.reweighted(Rx, F[0], F[1], deltas[0]), H.reweighted(Ry, F[1], F[2], deltas[1])
                H64, g64 = A.systems(Rxw, Ryw, *F, which, L2)
                Rxw, Ryw = H.reweighted(Rx, F[0], F[1], deltas[0], np.float32), H.reweighted(Ry, F[1], F[2], deltas[1], np.float32)
                H32, g32 = A.systems(Rxw, Ryw, *F, which, L2, dtype=np.float32)
                _check("normal: k %d sweep %s H" % (k, which), Hd[:, :k, :k], H32, H64, k, worst)
                _check("normal: k %d sweep %s g" % (k, which), gd[:, :k], g32, g64, k, worst)
        # projected CG: the rows whose float32 and float64 yardstick runs take the same decisions with a margin of at least 1e-3 (the
        # rule of test_gpu_als_nncg.py: a decision at its threshold is no parity case)
        Rw = [(H.reweighted(Rx, F[0], F[1], deltas[0], dt), H.reweighted(Ry, F[1], F[2], deltas[1], dt)) for dt in (np.float64, np.float32)]
        (y64, t64, m64, _), (y32, t32, m32, _) = (N.rows(*Rw[i], *F, which, L2, 3, dtype=dt) for i, dt in enumerate((np.float64, np.float32)))
        sel = np.array([a == b for a, b in zip(t64, t32)]) & (np.minimum(m64, m32) >= 1e-3)
        got = ctx.als_nncg_rows(w, 0, n, L2, 3)[:, :k]
        print("nncg: k %d sweep %s: %d of %d rows are parity cases" % (k, which, int(sel.sum()), n))
        assert sel.sum() >= n // 4 and (got >= 0).all()                          # (at k = 200 the margin rule leaves 21, 47 and 23 rows)
        _check("nncg: k %d sweep %s (rows)" % (k, which), got[sel], y32[sel], y64[sel], k, worst)
        ctx.als_nncg_step(L2, BITS[which], BITS[which], 0, 3)                     # the same sweep as a step: masks 1, 2, 4
        stepped = ctx.get_factor(w)
        _reset(ctx, F)
        _check("nncg: k %d sweep %s (step)" % (k, which), stepped[sel], y32[sel], y64[sel], k, worst)
    print("k %d: worst |err| / tol per route: %s" % (k, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    ctx.close()


@pytest.mark.parametrize("route", ["cg", "nnls", "dual"])
def test_whole_steps_of_the_other_routes(lib, route):
    """Mask 7 (V, U, Z, each sweep behind its own pass at the factors the sweeps before it left) through cmf_als_cg_step,
    cmf_als_nnls_step and cmf_als_dual_step, delta = 1 on X and 0.75 on Y."""
    k = 40
    X, Y, Wx, Wy, F = C.problem(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    kw, nn, call = {"cg": (dict(cg_steps=3), 0, lambda c: c.als_cg_step(L2, 0, 7, 3)),
                    "nnls": (dict(nn_sweeps=3), 7, lambda c: c.als_nnls_step(L2, 7, 7, 3)),
                    "dual": (dict(dual_max=128), 0, lambda c: c.als_dual_step(L2, 0, 7, 128))}[route]
    Fs = [np.abs(M) for M in F] if nn else F
    ctx = _context(lib, X, Y, Fs, Wx, Wy)
    ctx.set_huber_delta(0, 1.0)
    ctx.set_huber_delta(1, 0.75)
    ref = {dt: H.step(Rx, Ry, *Fs, L2, deltas=(1.0, 0.75), nn_mask=nn, dtype=dt, **kw) for dt in (np.float64, np.float32)}
    call(ctx)
    worst = {}
    for w in range(3):
        _check("%s: mask 7 factor %s" % (route, NAMES[w]), ctx.get_factor(w), ref[np.float32][w], ref[np.float64][w], k, worst)
    ctx.close()


@pytest.mark.parametrize("yform", ["observed", "full", "logistic"])
def test_whole_steps_with_x_huber_beside_every_form_of_y(lib, yform):
    """Mask 7 (V, U, Z) and the V sweep alone, X under delta = 1: Y observed Frobenius, full, and logistic."""
    import logit_yardstick as L
    k = 40
    X, Y, Wx, Wy, F = C.problem(k)
    if yform == "full":
        Wy = None
    if yform == "logistic":
        Y = (Y > 0).astype(float)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    ctx.set_huber_delta(0, 1.0)
    worst = {}
    if yform == "logistic":
        ctx.set_relation_loss(1, "logistic")

        def sweep(Fc, which, dt):
            return L.sweep(H.reweighted(Rx, Fc[0], Fc[1], 1.0, dt), Ry, *Fc, which, L2, logit=(False, True), dtype=dt)
    else:
        def sweep(Fc, which, dt):
            return H.sweep(Rx, Ry, *Fc, which, L2, deltas=(1.0, None), dtype=dt)
    for mask in (2, 7):
        ref = {}
        for dt in (np.float64, np.float32):
            Fc = [np.array(M, dtype=dt) for M in F]
            for which in "VUZ":
                if mask & BITS[which]:
                    Fc[NAMES.index(which)] = sweep(Fc, which, dt)
            ref[dt] = Fc
        ctx.als_step(L2, 0, mask)
        for w in range(3):
            _check("step: Y %s mask %d factor %s" % (yform, mask, NAMES[w]), ctx.get_factor(w), ref[np.float32][w], ref[np.float64][w], k, worst)
        _reset(ctx, F)
    ctx.close()


def test_rows_and_bias_blocks_under_x_biases(lib):
    k = 40
    X, Y, Wx, Wy, F = C.problem(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    rng = np.random.RandomState(5)
    bx = (0.125, _f32(0.3 * rng.randn(C.M)), _f32(0.3 * rng.randn(C.D)))
    lb = 0.5
    ctx = _context(lib, X, Y, F, Wx, Wy)
    ctx.set_biases(0, True, bx[0], lb)
    for axis in (0, 1):
        ctx.set_bias(0, axis, bx[1 + axis])
    ctx.set_huber_delta(0, 1.0)
    worst = {}
    for which, rows in (("U", lambda: ctx.als_cg_rows(0, 0, C.M, L2, 3)), ("V", lambda: ctx.als_dual_rows(1, 0, C.D, L2, 128))):
        kw = dict(cg_steps=3) if which == "U" else dict(dual_max=128)
        y64, y32 = (H.sweep(Rx, Ry, *F, which, L2, deltas=(1.0, None), bx=bx, dtype=dt, **kw) for dt in (np.float64, np.float32))
        _check("biases: sweep %s rows" % which, rows()[:, :k], y32, y64, k, worst)
    for axis in (0, 1):
        y64, y32 = (H.bias_sweep(Rx, F[0], F[1], bx, lb, axis, 1.0, dt) for dt in (np.float64, np.float32))
        _check("biases: bias block, axis %d" % axis, ctx.als_bias_rows(0, axis), y32, y64, k, worst)
    ref = {dt: H.step(Rx, Ry, *F, L2, deltas=(1.0, None), bx=bx, lb=lb, dtype=dt) for dt in (np.float64, np.float32)}
    ctx.als_bias_step(L2, 0, 7)
    for w in range(3):
        _check("biases: step, factor %s" % NAMES[w], ctx.get_factor(w), ref[np.float32][w], ref[np.float64][w], k, worst)
    for axis in (0, 1):
        _check("biases: step, bias axis %d" % axis, ctx.get_bias(0, axis), ref[np.float32][3][1 + axis], ref[np.float64][3][1 + axis], k, worst)
    # the residual and the loss read the images as they were bound, whatever the last sweep left in the Huber arrays
    got = [ctx.get_factor(w) for w in range(3)]
    bnow = (bx[0], ctx.get_bias(0, 0), ctx.get_bias(0, 1))
    want = A.residual_sq(B.adjusted(Rx, bnow), got[0], got[1])
    assert abs(ctx.als_residual_sq(True, False)[0] - want) <= 1e-5 * want
    want = H.loss(B.adjusted(Rx, bnow), got[0], got[1], 1.0)
    assert abs(ctx.als_huber_loss(True, False)[0] - want) <= 1e-5 * want
    ctx.close()


# ------------------------------------------------------------------ 5. descent on the device
DESCENT = {"exact": (3, 0, lambda c, l2, nn: c.als_step(l2, nn, 7)), "cg": (3, 0, lambda c, l2, nn: c.als_cg_step(l2, nn, 7, 3)),
           "dual": (40, 0, lambda c, l2, nn: c.als_dual_step(l2, nn, 7, 128)), "nnls": (3, 7, lambda c, l2, nn: c.als_nnls_step(l2, nn, 7, 4)),
           "nncg": (3, 7, lambda c, l2, nn: c.als_nncg_step(l2, nn, 7, 0, 3, 4))}


@pytest.mark.parametrize("route", sorted(DESCENT))
def test_ten_device_iterations_never_raise_the_objective(lib, route):
    """planted(3), delta = 1 on X: the float64 objective of the downloaded factors satisfies J' <= J + (k + 16) 2^-24 |J| (the rule of
    test_gpu_als_logit.py)."""
    k, nn, call = DESCENT[route]
    P = H.planted(3, k)
    F = [_f32(np.abs(M) if nn else M) for M in (P.U, P.V, P.Z)]
    Rx, Ry = A.Relation(_f32(P.X), P.W), A.Relation(_f32(P.Y), None)
    ctx = _context(lib, _f32(P.X), _f32(P.Y), F, P.W, None)
    ctx.set_huber_delta(0, 1.0)
    trace = [H.objective(Rx, Ry, *F, P.l2, deltas=(1.0, None))]
    for _ in range(10):
        call(ctx, P.l2, nn)
        trace.append(H.objective(Rx, Ry, *[ctx.get_factor(w) for w in range(3)], P.l2, deltas=(1.0, None)))
    ctx.close()
    print("device objective (%s): %s" % (route, " ".join("%.2f" % v for v in trace)))
    for a, b in zip(trace, trace[1:]):
        assert b <= a + (k + 16) * 2.0 ** -24 * abs(a)
    assert trace[-1] < trace[0]


# ------------------------------------------------------------------ 6. the estimator
@pytest.mark.parametrize("seed", [3, 5, 7])
def test_estimator_against_the_yardstick(lib, seed):
    from pycmf_amd import CMF
    P = H.planted(seed)
    X, Y = _f32(P.X), _f32(P.Y)
    Rx, Ry = A.Relation(X, P.W), A.Relation(Y, None)
    start = [_f32(M) for M in (P.U, P.V, P.Z)]
    kw = dict(n_components=3, solver="als", l2_reg=P.l2, max_iter=P.max_iter, tol=0.0, x_init="custom", y_init="custom", U_non_negative=False,
              V_non_negative=False, Z_non_negative=False)
    model = CMF(x_huber_delta=1.0, **kw)
    U, V, Z = model.fit_transform(X, Y, U=start[0].copy(), V=start[1].copy(), Z=start[2].copy(), x_entry_weights=P.W)
    ref = H.fit(Rx, Ry, *start, P.max_iter, P.l2, deltas=(1.0, None))[:3]
    want = sum(H.errors(Rx, Ry, *ref, deltas=(1.0, None)))
    print("seed %d: reconstruction_err_ %.6f, yardstick %.6f, relative %.2e" % (seed, model.reconstruction_err_, want,
                                                                                abs(model.reconstruction_err_ - want) / want))
    assert abs(model.reconstruction_err_ - want) <= 1e-4 * want
    lx, ly = model.huber_loss_
    assert ly == 0.0 and abs(lx - H.loss(Rx, U, V, 1.0)) <= 1e-6 * lx
    ctx = _context(lib, X, Y, [U, V, Z], P.W, None)
    ctx.set_huber_delta(0, 1.0)
    assert ctx.als_huber_loss() == (lx, ly)                                       # huber_loss_ is cmf_als_huber_loss at the fitted factors
    ctx.close()
    plain = CMF(**kw)
    Uf, Vf, _ = plain.fit_transform(X, Y, U=start[0].copy(), V=start[1].copy(), Z=start[2].copy(), x_entry_weights=P.W)
    assert plain.huber_loss_ is None
    frob, huber = P.heldout_rmse(Uf, Vf), P.heldout_rmse(U, V)
    print("seed %d: RMSE on the clean unobserved cells, Frobenius %.3f, Huber %.3f" % (seed, frob, huber))
    assert huber < 0.5 * frob
    # fold-in of 10 new rows against the fitted V, one of them carrying an outlier: the yardstick's fold-in from transform's own start
    from pycmf_amd.factor_init import init_custom
    Xn, Wn = X[:10].copy(), P.W[:10].copy()
    j = Wn[0].indices[0]
    Xn[0, j] = _f32(Xn[0, j] + 25.0)
    Rn, Rnone = A.Relation(Xn, Wn), A.Relation(np.zeros((V.shape[0], Z.shape[0])), None)
    model.set_params(max_iter=5, random_state=0)
    Un = model.transform(Xn, None, x_entry_weights=Wn)[0]
    U0 = _f32(init_custom(None, Xn, 3, 0, non_negative=False, random_state=0))
    y64, y32 = (H.fit(Rn, Rnone, U0, V, Z, 5, P.l2, deltas=(1.0, None), mask=A.U_BIT, dtype=dt)[0] for dt in (np.float64, np.float32))
    tol = A.tolerance(y32, y64, 3)
    err = float(np.abs(Un - y64).max())
    print("seed %d: transform |err| / tol %.3f (tol %.3e)" % (seed, err / tol, tol))
    assert err <= tol
    frob_fold = A.sweep(Rn, Rnone, U0, V, Z, "U", P.l2)
    clean_fold = A.sweep(A.Relation(X[:10], Wn), Rnone, U0, V, Z, "U", P.l2)
    print("seed %d: the row with the outlier moves by %.3f under the Huber fold-in, by %.3f under the Frobenius one"
          % (seed, float(np.abs(Un[0] - clean_fold[0]).max()), float(np.abs(frob_fold[0] - clean_fold[0]).max())))
    assert np.abs(Un[0] - clean_fold[0]).max() < np.abs(frob_fold[0] - clean_fold[0]).max()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_by_their_message_and_the_context_stays_usable(lib):
    k = 40
    X, Y, Wx, Wy, F = C.problem(k)
    Wp = Wx.copy()
    Wp.data = np.where(Wp.data == 0, 0.75, Wp.data)
    ctx = _context(lib, X, Y, F, Wp, None)
    for bad in (-1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="delta must be finite and > 0"):
            ctx.set_huber_delta(0, bad)
    with pytest.raises(ValueError, match="which must be 0"):
        ctx.set_huber_delta(2, 1.0)
    ctx.set_huber_delta(1, 1.0)                                                   # Y is full
    entries = [lambda: ctx.als_step(L2, 0, 7), lambda: ctx.als_nnls_step(L2, 7, 6, 3), lambda: ctx.als_cg_step(L2, 0, 2, 3),
               lambda: ctx.als_dual_step(L2, 0, 4, 64), lambda: ctx.als_huber_loss(), lambda: ctx.als_huber_weights(1, 0, 10)]
    for call in entries:
        with pytest.raises((NotImplementedError, RuntimeError, ValueError), match="Y has a Huber loss .* and no CSR weights bound"):
            call()
    ctx.als_step(L2, 0, 1)                                                        # the U sweep does not read Y
    ctx.set_huber_delta(1, 0)
    ctx.set_huber_delta(0, 1.0)
    ctx.set_background_weight(0, 0.25)
    for call in (lambda: ctx.als_step(L2, 0, 1), lambda: ctx.als_cg_rows(0, 0, 5, L2, 3), lambda: ctx.als_normal(1, 0, 5, L2),
                 lambda: ctx.als_huber_loss(True, False)):
        with pytest.raises((NotImplementedError, RuntimeError, ValueError), match="X has a Huber loss and a background weight"):
            call()
    ctx.als_step(L2, 0, 4)                                                        # the Z sweep does not read X
    ctx.set_background_weight(0, 0.0)
    ctx.set_relation_loss(0, "logistic")
    for call in (lambda: ctx.als_step(L2, 0, 2), lambda: ctx.als_nnls_step(L2, 1, 1, 3), lambda: ctx.als_huber_weights(0, 1, Wp.nnz)):
        with pytest.raises((NotImplementedError, RuntimeError, ValueError), match="X has a Huber loss and a logistic loss"):
            call()
    ctx.set_relation_loss(0, "frobenius")
    with pytest.raises(ValueError, match="Y has no Huber loss"):
        ctx.als_huber_weights(1, 0, 0)
    _reset(ctx, F)
    ctx.als_step(L2, 0, 7)                                                        # usable, and under the delta
    stepped = _bits(ctx)
    ctx.set_huber_delta(0, 0)
    _reset(ctx, F)
    ctx.als_step(L2, 0, 7)
    assert _bits(ctx) != stepped and all(np.isfinite(ctx.get_factor(w)).all() for w in range(3))
    ctx.close()
