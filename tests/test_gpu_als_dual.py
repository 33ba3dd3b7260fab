"""The dual form of the exact ALS rows on the device (cmf_als_dual_rows, cmf_als_dual_step, cmf_als_dual_last, CMF(als_dual_max=n))
against the float64 yardstick als_yardstick.sweep -- the PRIMAL rows -- on float32-rounded inputs.  Tolerance per comparison
(als_yardstick.tolerance, the HALS rule): tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|) with y32 the float32 run of the dual
yardstick (als_dual_yardstick.dual_rows, routed as the planner routes).  The problem is als_dual_cases.py: row lengths on both sides
of every class edge, stored zero weights, two observed sides.

Measured on an MI355X (worst |err| / tol of each group): see DESIGN section 24."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_dual_cases as C
import als_dual_yardstick as D
import als_yardstick as A
from test_gpu_als import _context, _f32

pytestmark = pytest.mark.gpu

NAMES = "UVZ"
BITS = {"U": A.U_BIT, "V": A.V_BIT, "Z": A.Z_BIT}
L2 = C.L2
_refs = {}


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _relations(k):
    X, Y, Wx, Wy, F = C.problem(k)
    return A.Relation(X, Wx), A.Relation(Y, Wy)


def _primal(k, which):
    """float64 primal rows of the sweep: computed once, shared."""
    if (k, which) not in _refs:
        Rx, Ry = _relations(k)
        _refs[(k, which)] = A.sweep(Rx, Ry, *C.problem(k)[4], which, L2)
    return _refs[(k, which)]


def _dual32(k, which, dual_max):
    if (k, which, dual_max) not in _refs:
        Rx, Ry = _relations(k)
        _refs[(k, which, dual_max)] = D.dual_rows(Rx, Ry, *C.problem(k)[4], which, L2, dual_max, dtype=np.float32)
    return _refs[(k, which, dual_max)]


def _ctx(lib, k):
    X, Y, Wx, Wy, F = C.problem(k)
    return _context(lib, X, Y, F, Wx, Wy)


def _reset(ctx, F):
    for w in range(3):
        ctx.set_factor(w, F[w])


# ------------------------------------------------------------------ 1. rows against the yardstick, and which route ran
@pytest.mark.parametrize("k", [40, 100, 200])
def test_rows_against_the_yardstick(lib, k):
    """U, V and Z rows under dual_max = 128, 64 and 20: every row of every sweep is compared, the counts of cmf_als_dual_last are
    the Python planner's, the padding stays zero and the factors are left alone."""
    F = C.problem(k)[4]
    Rx, Ry = _relations(k)
    ctx = _ctx(lib, k)
    worst = 0.0
    for which in NAMES:
        w = NAMES.index(which)
        y64 = _primal(k, which)
        for dual_max in (128, 64, 20):
            tol = A.tolerance(_dual32(k, which, dual_max), y64, k)
            got = ctx.als_dual_rows(w, 0, F[w].shape[0], L2, dual_max)
            routes = D.plan(Rx, Ry, which, k, dual_max)
            assert ctx.als_dual_last() == D.counts(routes), (which, dual_max)
            err = float(np.abs(got[:, :k] - y64).max())
            worst = max(worst, err / tol)
            print("k %d sweep %s dual_max %d: routes %s, |err| / tol %.3f (tol %.3e)" % (k, which, dual_max, D.counts(routes), err / tol, tol))
            assert np.isfinite(got).all() and err <= tol, (which, dual_max, err, tol)
            assert (got[:, k:] == 0).all()
            assert (got[[r == D.ZERO for r in routes]] == 0).all()
    print("k %d: worst |err| / tol %.3f" % (k, worst))
    assert all((ctx.get_factor(w) == F[w]).all() for w in range(3))               # the hook leaves the factors alone
    part = ctx.als_dual_rows(0, 3, 20, L2, 128)                                   # a range inside: the same rows
    assert (part == ctx.als_dual_rows(0, 0, C.M, L2, 128)[3:23]).all()
    ctx.close()


def test_k_pad_32_never_goes_dual_and_keeps_the_bits_of_the_exact_step(lib):
    k = 3
    F = C.problem(k)[4]
    ctx = _ctx(lib, k)
    for which in NAMES:
        w = NAMES.index(which)
        got = ctx.als_dual_rows(w, 0, F[w].shape[0], L2, 128)
        last = ctx.als_dual_last()
        assert last[:3] == (0, 0, 0) and last[3] + last[4] == F[w].shape[0] and last[3] > 0
        _reset(ctx, F)
        ctx.als_step(L2, 0, BITS[which])
        assert got[:, :k].tobytes() == ctx.get_factor(w).astype(np.float32).tobytes(), which
        _reset(ctx, F)
        ctx.als_dual_step(L2, 0, BITS[which], 128)
        assert got[:, :k].tobytes() == ctx.get_factor(w).astype(np.float32).tobytes(), which
        _reset(ctx, F)
    ctx.close()


# ------------------------------------------------------------------ 2. formed rows keep their bits; determinism
def test_formed_rows_of_a_mixed_sweep_keep_the_bits_of_the_exact_step(lib):
    k, dual_max = 200, 64
    F = C.problem(k)[4]
    Rx, Ry = _relations(k)
    ctx = _ctx(lib, k)
    for which in NAMES:
        w = NAMES.index(which)
        routes = D.plan(Rx, Ry, which, k, dual_max)
        formed = np.array([r == D.FORMED for r in routes])
        dual = np.array([r in (32, 64, 128) for r in routes])
        assert formed.sum() >= 3 and dual.sum() >= 3, which                       # a mixed sweep
        got = ctx.als_dual_rows(w, 0, F[w].shape[0], L2, dual_max)
        ctx.als_dual_step(L2, 0, BITS[which], dual_max)
        stepped = ctx.get_factor(w).astype(np.float32)
        assert ctx.als_dual_last() == D.counts(routes)
        assert stepped.tobytes() == got[:, :k].tobytes(), which                   # the step writes what the hook returns
        _reset(ctx, F)
        ctx.als_step(L2, 0, BITS[which])
        exact = ctx.get_factor(w).astype(np.float32)
        _reset(ctx, F)
        assert got[formed][:, :k].tobytes() == exact[formed].tobytes(), which
        assert (got[~formed & ~dual] == 0).all() and (exact[~formed & ~dual] == 0).all()
    ctx.close()


def test_calls_repeat_to_the_bit_and_a_row_does_not_depend_on_its_neighbours_route(lib):
    k = 200
    F = C.problem(k)[4]
    Rx, Ry = _relations(k)
    ctx = _ctx(lib, k)
    for which in NAMES:
        w = NAMES.index(which)
        n = F[w].shape[0]
        got = {dm: ctx.als_dual_rows(w, 0, n, L2, dm) for dm in (128, 64, 20, 0)}
        for dm, rows in got.items():
            assert rows.tobytes() == ctx.als_dual_rows(w, 0, n, L2, dm).tobytes(), (which, dm)
        routes = {dm: D.plan(Rx, Ry, which, k, dm) for dm in got}
        pairs = 0
        for a, b in ((128, 64), (128, 20), (64, 20), (20, 0), (64, 0)):
            same = np.array([ra == rb for ra, rb in zip(routes[a], routes[b])])       # dual in both (same class), formed in both, zero
            changed = int((~same).sum())
            assert changed > 0 and same.sum() > 0, (which, a, b)                      # neighbours did change route
            assert got[a][same].tobytes() == got[b][same].tobytes(), (which, a, b)
            pairs += 1
        assert pairs == 5
        lo, hi = n // 3, 2 * n // 3                                                   # a sub-range: other neighbours, other slots
        assert ctx.als_dual_rows(w, lo, hi - lo, L2, 128).tobytes() == got[128][lo:hi].tobytes(), which
    ctx.close()


# ------------------------------------------------------------------ 3. sweeps that are not eligible keep today's bits
def _factors_after(ctx, F, call):
    _reset(ctx, F)
    call()
    out = [ctx.get_factor(w).astype(np.float32).tobytes() for w in range(3)]
    _reset(ctx, F)
    return out


def test_sweeps_that_are_not_eligible_keep_the_bits_of_the_exact_step(lib):
    k = 100
    X, Y, Wx, Wy, F = C.problem(k)
    Wp = Wx.copy()
    Wp.data = np.where(Wp.data == 0, 0.75, Wp.data)                               # (a background needs w >= c0 on every stored entry)
    labels = (X > 0).astype(float)
    cases = (("Y full: V has a shared term, Z no observed relation", _context(lib, X, Y, F, Wx, None), A.V_BIT | A.Z_BIT, None),
             ("a background weight on X: U and V have a shared term", _context(lib, X, Y, F, Wp, Wy), A.U_BIT | A.V_BIT, "bg"),
             ("a logistic X: U and V read it", _context(lib, labels, Y, F, Wx, Wy), A.U_BIT | A.V_BIT, "logit"))
    for what, ctx, mask, extra in cases:
        if extra == "bg":
            ctx.set_background_weight(0, 0.25)
        if extra == "logit":
            ctx.set_relation_loss(0, "logistic")
        before = ctx.als_dual_last()
        exact = _factors_after(ctx, F, lambda: ctx.als_step(L2, 0, mask))
        dual = _factors_after(ctx, F, lambda: ctx.als_dual_step(L2, 0, mask, 128))
        assert dual == exact, what
        assert ctx.als_dual_last() == before, what                                # no dual sweep ran
        # the whole iteration under dual_max = 0 is the exact iteration; under 128 the eligible sweep differs from it only in rounding
        assert _factors_after(ctx, F, lambda: ctx.als_dual_step(L2, 0, 7, 0)) == _factors_after(ctx, F, lambda: ctx.als_step(L2, 0, 7)), what
        ctx.als_dual_step(L2, 0, 7, 128)
        assert sum(ctx.als_dual_last()[:3]) > 0, what                             # the eligible sweep of the iteration did go dual
        ctx.close()


# ------------------------------------------------------------------ 4. projection, biases
def test_a_non_negative_factor_without_sweeps_gets_the_dual_rows_projected(lib):
    k = 100
    F = C.problem(k)[4]
    ctx = _ctx(lib, k)
    for which in NAMES:
        w = NAMES.index(which)
        y64 = np.maximum(_primal(k, which), 0.0)
        tol = A.tolerance(np.maximum(_dual32(k, which, 128), 0.0), y64, k)
        ctx.als_dual_step(L2, 7, BITS[which], 128, 0, 0)
        got = ctx.get_factor(w)
        assert sum(ctx.als_dual_last()[:3]) > 0
        err = float(np.abs(got - y64).max())
        print("projected sweep %s: |err| / tol %.3f" % (which, err / tol))
        assert (got >= 0).all() and (got == 0).any() and err <= tol, which
        _reset(ctx, F)
    ctx.close()


def test_rows_under_biases_read_the_adjusted_targets(lib):
    """x_biases bound with non-zero row and column biases: the U and V rows against the yardstick fed the bias-corrected targets
    the device holds (cmf_als_bias_targets: t - mu - r_i - c_j in float32)."""
    k = 100
    X, Y, Wx, Wy, F = C.problem(k)
    rng = np.random.RandomState(7)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    ctx.set_biases(0, True, 0.3, 0.05)
    ctx.set_bias(0, 0, _f32(0.5 * rng.randn(C.M)))
    ctx.set_bias(0, 1, _f32(0.5 * rng.randn(C.D)))
    bt, _ = ctx.als_bias_targets(0, 0, Wx.nnz)
    r = np.repeat(np.arange(C.M), np.diff(Wx.indptr))
    Xb = np.zeros((C.M, C.D))
    Xb[r, Wx.indices] = bt
    assert np.abs(Xb - X * (Xb != 0)).max() > 0.1                                 # the targets did move
    Rx, Ry = A.Relation(Xb, Wx), A.Relation(Y, Wy)
    for which in "UV":
        w = NAMES.index(which)
        y64 = A.sweep(Rx, Ry, *F, which, L2)
        tol = A.tolerance(D.dual_rows(Rx, Ry, *F, which, L2, 128, dtype=np.float32), y64, k)
        got = ctx.als_dual_rows(w, 0, F[w].shape[0], L2, 128)
        assert sum(ctx.als_dual_last()[:3]) > 0
        err = float(np.abs(got[:, :k] - y64).max())
        print("biased sweep %s: |err| / tol %.3f" % (which, err / tol))
        assert err <= tol, which
    # the step with biases bound: the factor sweeps in dual form, then the bias blocks of cmf_als_bias_step
    rows = ctx.als_dual_rows(0, 0, C.M, L2, 128)
    ctx.als_dual_step(L2, 0, A.U_BIT, 128)
    assert ctx.get_factor(0).astype(np.float32).tobytes() == rows[:, :k].tobytes()
    assert np.abs(ctx.get_bias(0, 0)).max() > 0 and np.isfinite(ctx.get_bias(0, 0)).all()
    ctx.close()


# ------------------------------------------------------------------ 5. a fit through CMF, and the fold-in
def _planted():
    """120 x 150, planted rank 12, 50 % observed (rates from 10 % to 90 % along the rows of X and the columns of Y, so every class
    and the formed route take rows), k = 100."""
    r = np.random.RandomState(5)
    m, d, p, k = 120, 150, 30, 100
    Ut, Vt, Zt = (r.randn(n, 12) / 12 ** 0.25 for n in (m, d, p))
    X, Y = _f32(Ut @ Vt.T + .1 * r.randn(m, d)), _f32(Vt @ Zt.T + .1 * r.randn(d, p))
    Wx = (r.rand(m, d) < np.linspace(0.1, 0.9, m)[:, None]).astype(float)
    Wy = (r.rand(d, p) < np.linspace(0.1, 0.9, p)[None, :]).astype(float)
    U, V, Z = (_f32(0.1 * r.randn(n, k)) for n in (m, d, p))
    Xn = _f32(r.randn(10, 12) / 12 ** 0.25 @ Vt.T + .1 * r.randn(10, d))
    Wn = (r.rand(10, d) < np.linspace(0.02, 0.3, 10)[:, None]).astype(float)
    return X, Y, Wx, Wy, U, V, Z, Xn, Wn


def test_fit_and_fold_in_match_the_float64_yardstick(lib):
    """10 signed iterations through CMF(als_dual_max=128).  The objective after every iteration (from the device's factors, in
    float64) never rises beyond the rounding of the float32 factors, (k + 16) 2^-24 relative, and agrees with als_yardstick.fit's
    trace under the bound test_gpu_als.py puts on its exact fit's error, 1e-4 relative; so does reconstruction_err_.  (The
    factors themselves are not compared: at k = 100 over a rank-12 plant the FLOAT32 PRIMAL yardstick is 1.7e-3 max|R| from the
    float64 one after 10 iterations, beyond that test's 1e-3.)  transform() on 10 new rows of 3 .. 45 entries is one dual U sweep."""
    from pycmf_amd import CMF
    X, Y, Wx, Wy, U, V, Z, Xn, Wn = _planted()
    k, l2, iters = 100, 0.05, 10
    Wxs, Wys = sp.csr_matrix(Wx), sp.csr_matrix(Wy)
    assert abs(Wx.mean() - 0.5) < 0.02
    trace = []
    Ur, Vr, Zr, n_iter, _ = A.fit(X, Y, Wxs, Wys, U, V, Z, iters, l2, trace=trace)
    ctx = _context(lib, X, Y, [U, V, Z], Wxs, Wys)
    prev = A.objective(X, Y, Wxs, Wys, U, V, Z, l2)
    classes = np.zeros(5, dtype=np.int64)
    for it in range(iters):
        ctx.als_dual_step(l2, 0, 7, 128)
        classes += np.array(ctx.als_dual_last())                                  # (the Z sweep's, the last of the iteration)
        cur = A.objective(X, Y, Wxs, Wys, *[ctx.get_factor(w) for w in range(3)], l2)
        print("iteration %d: objective %.9g, yardstick %.9g, relative %.2e" % (it + 1, cur, trace[it], abs(cur - trace[it]) / trace[it]))
        assert cur <= prev * (1 + (k + 16) * 2.0 ** -24), (it, prev, cur)
        assert abs(cur - trace[it]) <= 1e-4 * trace[it], (it, cur, trace[it])
        prev = cur
    ctx.close()
    assert classes[0] > 0 and classes[1] > 0 and classes[3] > 0                   # classes 32 and 64 and the formed route all took rows
    kw = dict(n_components=k, l2_reg=l2, tol=0, x_init="custom", y_init="custom", U_non_negative=False, V_non_negative=False, Z_non_negative=False)
    model = CMF(solver="als", max_iter=iters, als_dual_max=128, **kw)
    Xi, Yi = sp.csr_matrix(X * Wx), sp.csr_matrix(Y * Wy)
    assert Xi.nnz == Wxs.nnz and Yi.nnz == Wys.nnz
    Ug, Vg, Zg = model.fit_transform(Xi, Yi, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights="observed", y_entry_weights="observed")
    ref = sum(A.errors(X, Y, Wxs, Wys, Ur, Vr, Zr))
    print("fit: reconstruction_err_ %.9g, yardstick %.9g, relative %.2e" % (model.reconstruction_err_, ref, abs(model.reconstruction_err_ - ref) / ref))
    assert model.n_iter_ == n_iter == iters and abs(model.reconstruction_err_ - ref) <= 1e-4 * ref
    assert abs(A.objective(X, Y, Wxs, Wys, Ug, Vg, Zg, l2) - prev) <= 1e-6 * prev  # the estimator ran the steps above
    # the fold-in: V and Z fixed, the new rows' U by one sweep over their observed entries
    Wns = sp.csr_matrix(Wn)
    Xni = sp.csr_matrix(Xn * Wn)
    assert Xni.nnz == Wns.nnz
    U2, V2, Z2 = model.transform(Xni, None, x_entry_weights="observed")
    assert V2.tobytes() == model.components.tobytes() and Z2.tobytes() == model.y_weights.tobytes()
    Rn = A.Relation(Xn, Wns)
    routes = D.plan(Rn, None, "U", k, 128)
    assert all(r in (32, 64) for r in routes) and len(routes) == 10
    U0 = np.zeros((10, k))
    y64 = A.sweep(Rn, None, U0, Vg, Zg, "U", l2)
    tol = A.tolerance(D.dual_rows(Rn, None, U0, Vg, Zg, "U", l2, 128, dtype=np.float32), y64, k)
    err = float(np.abs(U2 - y64).max())
    print("fold-in: |err| / tol %.3f" % (err / tol))
    assert U2.shape == (10, k) and err <= tol


# ------------------------------------------------------------------ 6. errors
def test_refusals_leave_the_context_usable(lib):
    k = 100
    X, Y, Wx, Wy, F = C.problem(k)
    ctx = lib.Context(0)
    ctx.set_problem(C.M, C.D, C.P, 300)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.als_dual_step(L2, 0, 7, 64)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.als_dual_rows(0, 0, 1, L2, 64)
    ctx.close()
    ctx = _context(lib, X, Y, F, Wx, None)                                        # Y full
    for bad in (-1, 129):
        with pytest.raises(ValueError, match="dual_max must be 0 .. 128"):
            ctx.als_dual_step(L2, 0, 7, bad)
        with pytest.raises(ValueError, match="dual_max must be 0 .. 128"):
            ctx.als_dual_rows(0, 0, C.M, L2, bad)
    with pytest.raises(ValueError, match="l2 must be positive"):
        ctx.als_dual_step(0.0, 0, 7, 64)
    with pytest.raises(ValueError, match="nn_sweeps must be 0 .. 1024"):
        ctx.als_dual_step(L2, 7, 7, 64, -1, 0)
    with pytest.raises(ValueError, match="nn_cg_steps must be 0 .. 1024"):
        ctx.als_dual_step(L2, 7, 7, 64, 0, 1025)
    with pytest.raises(ValueError, match="rows out of range"):
        ctx.als_dual_rows(0, C.M - 1, 2, L2, 64)
    with pytest.raises(ValueError, match="not eligible: no observed relation"):
        ctx.als_dual_rows(2, 0, C.P, L2, 64)
    with pytest.raises(ValueError, match="not eligible: a shared term"):
        ctx.als_dual_rows(1, 0, C.D, L2, 64)
    y64 = _primal(k, "U")                                                         # the U sweep reads X alone: the shared reference
    got = ctx.als_dual_rows(0, 0, C.M, L2, 128)
    assert np.abs(got[:, :k] - y64).max() <= A.tolerance(_dual32(k, "U", 128), y64, k)
    ctx.close()
    ctx = _context(lib, (X > 0).astype(float), Y, F, Wx, Wy)
    ctx.set_relation_loss(0, "logistic")
    for w in (0, 1):
        with pytest.raises(ValueError, match="not eligible: a logistic relation"):
            ctx.als_dual_rows(w, 0, 1, L2, 64)
    y64 = _primal(k, "Z")                                                         # the Z sweep reads Y alone
    got = ctx.als_dual_rows(2, 0, C.P, L2, 128)
    assert np.abs(got[:, :k] - y64).max() <= A.tolerance(_dual32(k, "Z", 128), y64, k)
    ctx.close()
