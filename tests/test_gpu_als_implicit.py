"""ALS with a background weight on the device (cmf_set_background_weight, cmf_als_residual_sq, the three step entry points,
CMF(solver="als", x_background_weight=...)) against the float64 yardstick of als_yardstick.py (cx / cy) on float32-rounded inputs.
Shapes and cases are the ones of test_gpu_als.py; its weights lie in [0.25, 4], so c0 = 0.25 satisfies w >= c0 as they stand.
Tolerance of every comparison of factors, per factor: tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|) with y32 the float32 run
of the same formulas, and its first term may not exceed 1e-3 max|y64| (``_tol`` asserts it; on the CPU it is at most 1.2e-5 max|y64|
for the exact route, 5.2e-5 for 3 CG steps, 6e-6 for 4 coordinate-descent sweeps; cond(H_i) <= 270 on all four shapes).
Measured on an MI355X (worst |err| / tol of each group): see DESIGN section 18."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
import click_problem as K
import wmu_yardstick as WM
from test_gpu_als import NAMES, SHAPES, U_, V_, Z_, _case, _context, _exact_factor, _f32

pytestmark = pytest.mark.gpu

CAP = 1e-3
L2 = 0.1
C0 = 0.25
WHICH = ("U", "V", "Z")


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _tol(y32, y64, k, what=""):
    """The rule's tolerance; its float32-against-float64 term is capped at 1e-3 max|y64|."""
    spread = 4.0 * float(np.max(np.abs(np.asarray(y32, np.float64) - np.asarray(y64, np.float64))))
    cap = spread / (CAP * float(np.max(np.abs(y64))))
    assert cap <= 1.0, "%s: 4 max|y32 - y64| is %.3f of the cap 1e-3 max|y64|" % (what, cap)
    return A.tolerance(y32, y64, k), cap


def _background(ctx, cx, cy):
    if cx:
        ctx.set_background_weight(0, cx)
    if cy:
        ctx.set_background_weight(1, cy)
    return ctx


# ------------------------------------------------------------------ 1. exact arithmetic
def _bg_pattern(lengths, cols, rng):
    """A pattern with the given row lengths: weights in {3/4, 3/2, 9/2} (excess over c0 = 1/2 in {1/4, 1, 4}: exact square roots),
    integer data."""
    W = np.zeros((len(lengths), cols))
    T = np.zeros((len(lengths), cols))
    for i, n in enumerate(lengths):
        c = rng.permutation(cols)[:n]
        W[i, c] = rng.choice([0.75, 1.5, 4.5], size=n)
        T[i, c] = rng.choice([-4.0, 1.0, 2.0, 3.0], size=n)
    return T, sp.csr_matrix(W)


def _check_systems(ctx, Rx, Ry, F, which, l2, cx, cy, k, what):
    n = F[which].shape[0]
    H, g = ctx.als_normal(which, 0, n, l2)
    Hr, gr = A.systems(Rx, Ry, *F, WHICH[which], l2, cx=cx, cy=cy)
    kp = H.shape[1]
    assert (H[:, :k, :k] == Hr).all() and (g[:, :k] == gr).all(), what
    assert all((H[i] == H[i].T).all() for i in range(n)), what
    pad = H.copy()
    pad[:, :k, :k] = 0
    idx = np.arange(k, kp)
    assert (pad[:, idx, idx] == 1).all() and pad.sum() == n * (kp - k) and (g[:, k:] == 0).all(), what
    return H, g


@pytest.mark.parametrize("k", [7, 40, 128, 256])
def test_normal_equations_with_a_background_are_exact_on_exact_inputs(lib, k):
    """Every product and every partial sum is exactly representable in float32 (c0 = 1/2, excess weights 1/4, 1, 4, integer targets,
    l2 = 1/4, one-hot and power-of-two factor rows), so H and g equal the float64 yardstick with ==: rows of 0, 1, 31, 32, 33 and 70
    entries; the U sweep, the V sweep with a background on X beside full dense Y, the V sweep with backgrounds on both sides, the Z
    sweep."""
    rng = np.random.RandomState(100 + k)
    lengths = [0, 1, 31, 32, 33, 70]
    l2, c0 = 0.25, 0.5
    # U sweep: X is 6 x 80 with those row lengths
    m, d, p = 6, 80, 9
    X, Wx = _bg_pattern(lengths, d, rng)
    Y = np.zeros((d, p))
    F = [_exact_factor(m, k, 1), _exact_factor(d, k, 3), _exact_factor(p, k, 5)]
    ctx = _background(_context(lib, X, Y, F, Wx, None), c0, 0)
    assert ctx.get_background_weight(0) == c0 and ctx.get_background_weight(1) == 0
    H, g = _check_systems(ctx, A.Relation(X, Wx), A.Relation(Y, None), F, U_, l2, c0, 0, k, "U sweep, k = %d" % k)
    assert (H[0, :k, :k] == c0 * (F[1].T @ F[1]) + l2 * np.eye(k)).all() and (g[0] == 0).all()       # the row without stored entries
    part = ctx.als_normal(U_, 2, 3, l2)                                                                # a range inside: the same rows
    assert (part[0] == H[2:5]).all() and (part[1] == g[2:5]).all()
    ctx.close()
    # V sweep: X is 80 x 6 (its TRANSPOSE has those row lengths) with a background, beside full dense Y with small integers
    m, d, p = 80, 6, 50
    Xt, Wxt = _bg_pattern(lengths, m, rng)
    X, Wx = Xt.T.copy(), sp.csr_matrix(Wxt.T)
    F = [_exact_factor(m, k, 1), _exact_factor(d, k, 3), _exact_factor(p, k, 5)]
    Yd = rng.randint(-2, 3, size=(d, p)).astype(np.float64)
    ctx = _background(_context(lib, X, Yd, F, Wx, None), c0, 0)
    _check_systems(ctx, A.Relation(X, Wx), A.Relation(Yd, None), F, V_, l2, c0, 0, k, "V sweep beside full Y, k = %d" % k)
    ctx.close()
    # V sweep with backgrounds on both sides (Y observed, 6 x 50, its own lengths), and the Z sweep on Y's transposed image
    Y, Wy = _bg_pattern([33, 0, 1, 50, 32, 7], p, rng)
    ctx = _background(_context(lib, X, Y, F, Wx, Wy), c0, c0)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    H, g = _check_systems(ctx, Rx, Ry, F, V_, l2, c0, c0, k, "V sweep, two backgrounds, k = %d" % k)
    assert (H[1, :k, :k] != l2 * np.eye(k)).any()
    _check_systems(ctx, Rx, Ry, F, Z_, l2, c0, c0, k, "Z sweep, k = %d" % k)
    ctx.close()


# ------------------------------------------------------------------ 2. full steps against the yardstick
YFORMS = {"dense": 0.0, "observed": C0}          # Y full dense | Y observed with cy = 0.25


def _reference(shape, yform, mask, nn, nn_sweeps, cg):
    """(start, y64, y32) of one step, sweep by sweep (V, U, Z; the new V used for U and Z), every sweep computed once per input state
    and shared among the tests."""
    X, Y, Wx, Wy, F, store = _case(shape, yform)
    start = [np.abs(F[w]) if nn & (1 << w) else F[w] for w in range(3)]      # a non-negative factor starts as one
    key = ("implicit", nn)
    rels = store.setdefault(("implicit", "relations"), (A.Relation(X, Wx), A.Relation(Y, Wy)))
    state = {np.float64: list(start), np.float32: list(start)}
    tag = "start"
    for w, bit in ((V_, 2), (U_, 1), (Z_, 4)):
        if not mask & bit:
            continue
        route = dict(non_negative=bool(nn & bit), nn_sweeps=nn_sweeps, cg_steps=cg)
        ck = key + (w, tuple(route.values()), tag)
        if ck not in store:
            store[ck] = tuple(A.sweep(*rels, *state[dt], WHICH[w], L2, cx=C0, cy=YFORMS[yform], **route, dtype=dt) for dt in (np.float64, np.float32))
        state[np.float64][w], state[np.float32][w] = store[ck]
        if w == V_:
            tag = ("afterV", tuple(route.values()))
    return start, state[np.float64], state[np.float32]


def _run(ctx, nn, mask, nn_sweeps, cg):
    if cg:
        ctx.als_cg_step(L2, nn, mask, cg, nn_sweeps)
    elif nn_sweeps:
        ctx.als_nnls_step(L2, nn, mask, nn_sweeps)
    else:
        ctx.als_step(L2, nn, mask)


ROUTES = [("exact", 0, 7, 0, 0), ("exact", 0, 1, 0, 0), ("exact", 0, 2, 0, 0), ("exact", 0, 4, 0, 0), ("projected", 7, 7, 0, 0),
          ("nnls4", 7, 7, 4, 0), ("cg3", 0, 7, 0, 3), ("cg3+nnls4", 2, 7, 4, 3)]


@pytest.mark.parametrize("name, nn, mask, nn_sweeps, cg", ROUTES, ids=["%s-nn%d-mask%d" % r[:3] for r in ROUTES])
@pytest.mark.parametrize("yform", sorted(YFORMS))
@pytest.mark.parametrize("shape", SHAPES)
def test_full_step_with_a_background(lib, shape, yform, name, nn, mask, nn_sweeps, cg):
    m, d, p, k = shape
    X, Y, Wx, Wy, _, _ = _case(shape, yform)
    start, y64, y32 = _reference(shape, yform, mask, nn, nn_sweeps, cg)
    ctx = _background(_context(lib, X, Y, start, Wx, Wy), C0, YFORMS[yform])
    ctx.newton_clamp_stats(reset=True)
    before = [ctx.get_factor(w).tobytes() for w in range(3)]
    _run(ctx, nn, mask, nn_sweeps, cg)
    got = [ctx.get_factor(w) for w in range(3)]
    clamped = ctx.newton_clamp_stats()[0]
    ctx.close()
    report = []
    for w in range(3):
        if not mask & (1 << w):
            assert got[w].tobytes() == before[w], "factor %s was not swept and changed" % NAMES[w]
            continue
        tol, cap = _tol(y32[w], y64[w], k, "%s Y %s %s factor %s" % (shape, yform, name, NAMES[w]))
        err = float(np.abs(got[w] - y64[w]).max())
        report.append("%s %.3f (cap %.3f)" % (NAMES[w], err / tol, cap))
        assert np.isfinite(got[w]).all() and err <= tol, "%s: |err| / tol = %.3f (tol %.3e)" % (NAMES[w], err / tol, tol)
        if nn & (1 << w):
            assert (got[w] >= 0).all()
    if mask & 1:        # the row of U without stored entries is an ordinary row: the background gives it a system
        tol, _ = _tol(y32[0], y64[0], k)
        assert np.diff(Wx.indptr)[m // 3] == 0 and np.abs(got[0][m // 3] - y64[0][m // 3]).max() <= tol
    print("%s Y %s %s nn %d mask %d: |err| / tol %s; clamped rows %d" % (shape, yform, name, nn, mask, " ".join(report), clamped))
    assert clamped == 0, "the spectral clamp acted on %d rows" % clamped


# ------------------------------------------------------------------ 3. pieces and determinism
@pytest.mark.parametrize("k", [40, 256])
def test_rows_cut_into_pieces_with_a_background(lib, k):
    """The case of test_rows_cut_into_pieces (rows of 64 .. 500 entries) under c0 = 0.25, "als_piece" = 32 and the default: within
    (L + 16) 2^-24 sum|terms| per element of the yardstick's H and g, bit for bit the same when repeated."""
    rng = np.random.RandomState(11 + k)
    m, d, p, l2 = 5, 600, 4, 0.1
    lengths = [200, 333, 500, 257, 64]
    W = np.zeros((m, d))
    for i, n in enumerate(lengths):
        W[i, rng.permutation(d)[:n]] = _f32(0.25 + 3.75 * rng.rand(n))
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    Wx = sp.csr_matrix(W)
    Hr, gr = A.systems(A.Relation(X, Wx), A.Relation(Y, None), *F, "U", l2, cx=C0)
    Ha, ga = A.systems(A.Relation(np.abs(X), Wx), A.Relation(Y, None), F[0], np.abs(F[1]), F[2], "U", l2, cx=C0)    # sum |terms|
    for piece in (32, 0):
        ctx = _background(_context(lib, X, Y, F, Wx, None, piece=piece), C0, 0)
        lay = ctx.als_layout()
        H, g = ctx.als_normal(U_, 0, m, l2)
        H2, g2 = ctx.als_normal(U_, 0, m, l2)
        assert H.tobytes() == H2.tobytes() and g.tobytes() == g2.tobytes()
        assert lay[1] == (sum((n + 31) // 32 for n in lengths) if piece else m), lay
        worst = 0.0
        for i, n in enumerate(lengths):
            bound = (n + 16) * 2.0 ** -24
            worst = max(worst, float((np.abs(H[i, :k, :k] - Hr[i]) / (bound * Ha[i])).max()), float((np.abs(g[i, :k] - gr[i]) / (bound * ga[i])).max()))
        print("k %d piece %d: layout %s, worst |err| / bound %.4f" % (k, piece, lay, worst))
        assert worst <= 1.0
        ctx.close()


@pytest.mark.parametrize("yform", sorted(YFORMS))
def test_a_repeated_step_with_a_background_is_bit_identical(lib, yform):
    """All three routes, twice from the same factors; and the CG rows do not depend on "als_cg_lds"."""
    shape = (70, 333, 129, 40)
    X, Y, Wx, Wy, F, _ = _case(shape, yform)
    start = [np.abs(f) for f in F]
    ctx = _background(_context(lib, X, Y, start, Wx, Wy, piece=32), C0, YFORMS[yform])
    assert ctx.als_layout()[1] > shape[0]
    runs = {}
    for lds in (-1, 0):
        ctx.set_option("als_cg_lds", lds)
        for rep in range(2):
            out = []
            for nn, nn_sweeps, cg in ((0, 0, 0), (5, 0, 0), (7, 4, 0), (0, 0, 3), (2, 4, 3)):
                for w in range(3):
                    ctx.set_factor(w, start[w])
                _run(ctx, nn, 7, nn_sweeps, cg)
                out.append([ctx.get_factor(w).tobytes() for w in range(3)])
            runs[(lds, rep)] = out
    assert runs[(-1, 0)] == runs[(-1, 1)] == runs[(0, 0)] == runs[(0, 1)]
    ctx.close()


# ------------------------------------------------------------------ 4. c0 = 0 is the code without a background
def test_a_cleared_background_leaves_the_parents_bytes(lib):
    shape = (70, 333, 129, 40)
    X, Y, Wx, Wy, F, _ = _case(shape, "observed")
    start = [np.abs(f) for f in F]
    a, b = _context(lib, X, Y, start, Wx, Wy), _context(lib, X, Y, start, Wx, Wy)
    for which in (0, 1):
        b.set_background_weight(which, C0)
        assert b.get_background_weight(which) == C0
    with_bg = b.als_residual_sq()
    for which in (0, 1):
        b.set_background_weight(which, 0)
        assert b.get_background_weight(which) == 0
    for nn, nn_sweeps, cg in ((0, 0, 0), (7, 4, 0), (0, 0, 3)):
        for ctx in (a, b):
            for w in range(3):
                ctx.set_factor(w, start[w])
            _run(ctx, nn, 7, nn_sweeps, cg)
        assert [a.get_factor(w).tobytes() for w in range(3)] == [b.get_factor(w).tobytes() for w in range(3)], (nn, nn_sweeps, cg)
        ea, eb, ew = a.als_residual_sq(), b.als_residual_sq(), a.weighted_residual_sq()
        assert np.array(ea).tobytes() == np.array(eb).tobytes() == np.array(ew).tobytes()
    assert with_bg[0] > 0 and with_bg[1] > 0
    # rebinding or clearing the weights clears the background
    r = np.repeat(np.arange(Wx.shape[0]), np.diff(Wx.indptr))
    b.set_background_weight(0, C0)
    b.set_weighted_csr(0, Wx.indptr, Wx.indices, X[r, Wx.indices], Wx.data)
    assert b.get_background_weight(0) == 0
    b.set_background_weight(1, C0)
    b.clear_weight(1)
    assert b.get_background_weight(1) == 0
    for ctx in (a, b):
        ctx.clear_weight(1)
        ctx.set_data(1, Y)
        for w in range(3):
            ctx.set_factor(w, start[w])
        ctx.als_step(L2, 0, 7)
    assert [a.get_factor(w).tobytes() for w in range(3)] == [b.get_factor(w).tobytes() for w in range(3)]
    a.close()
    b.close()


# ------------------------------------------------------------------ 5. the error
def _error_tol(k, rel, Af, Bf, c0):
    """wmu_yardstick.resid_tol of the pattern term, the same rule applied to c0 sum_O s^2 (weights 1, targets 0: both of its sums
    are sum s^2), and 1e-12 of c0 <A^T A, B^T B> for the float64 trace term."""
    s = np.einsum("ij,ij->i", Af[rel.r], Bf[rel.c])
    e = rel.t - s
    E, wes = float((rel.w * e * e).sum()), float((rel.w * np.abs(e) * np.abs(s)).sum())
    q = float((s * s).sum())
    dot = float(((Af.T @ Af) * (Bf.T @ Bf)).sum())
    return WM.resid_tol(k, wes, E) + c0 * WM.resid_tol(k, q, q) + 1e-12 * c0 * dot


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[3]], ids=["k7", "k40", "k256"])
def test_error_with_a_background(lib, shape):
    k = shape[3]
    X, Y, Wx, Wy, F, _ = _case(shape, "observed")
    ctx = _background(_context(lib, X, Y, F, Wx, Wy), C0, C0)
    got = ctx.als_residual_sq()
    assert np.array(got).tobytes() == np.array(ctx.als_residual_sq()).tobytes()
    assert ctx.als_residual_sq(True, False) == (got[0], 0.0) and ctx.als_residual_sq(False, True) == (0.0, got[1])
    pattern_only = ctx.weighted_residual_sq()
    ctx.close()
    for name, rel, Af, Bf, g, po in (("X", A.Relation(X, Wx), F[0], F[1], got[0], pattern_only[0]), ("Y", A.Relation(Y, Wy), F[1], F[2], got[1], pattern_only[1])):
        ref = A.residual_sq(rel, Af, Bf, C0)
        tol = _error_tol(k, rel, Af, Bf, C0)
        print("%s %s: E %.9g, yardstick %.9g, |err| / tol %.3f (tol / E %.2e); pattern term alone %.9g" % (shape, name, g, ref, abs(g - ref) / tol, tol / ref, po))
        assert abs(g - ref) <= tol and g > po


def test_error_on_a_pattern_that_holds_every_cell(lib):
    """The two large terms cancel: E is the weighted residual, within the same bound."""
    m, d, p, k = 37, 53, 29, 40
    rng = np.random.RandomState(8)
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    Wx = sp.csr_matrix(_f32(0.25 + 3.75 * rng.rand(m, d)))
    assert Wx.nnz == m * d
    ctx = _background(_context(lib, X, Y, F, Wx, None), C0, 0)
    got = ctx.als_residual_sq(True, False)[0]
    ctx.close()
    rel = A.Relation(X, Wx)
    ref = A.residual_sq(rel, F[0], F[1])
    tol = _error_tol(k, rel, F[0], F[1], C0)
    print("full pattern: E %.9g, weighted residual %.9g, |err| / tol %.3f" % (got, ref, abs(got - ref) / tol))
    assert abs(got - ref) <= tol


# ------------------------------------------------------------------ 6. other solvers untouched, refusals
def test_other_solvers_are_untouched_by_background_steps(lib):
    """Context b runs ALS steps under a background in between (all three routes) and then drops the background and the weights, its
    factors reset afterwards; context a never hears of it.  cmf_mu_step, cmf_newton_step (per-row Hessians: a logit link),
    cmf_mu_weighted_step (the weights bound, the background cleared) and cmf_hals_step agree byte for byte."""
    m, d, p, k = 200, 300, 90, 12
    rng = np.random.RandomState(41)
    X, Y = _f32(np.abs(rng.randn(m, d))), _f32(1.0 / (1.0 + np.exp(-rng.randn(d, p))))
    F = [_f32(np.abs(rng.randn(n, k)) * 0.3 + 0.01) for n in (m, d, p)]
    Wx = sp.csr_matrix(_f32(rng.rand(m, d) + 0.5) * (rng.rand(m, d) < 0.2))
    a, b = _context(lib, X, Y, F, None, None), _context(lib, X, Y, F, None, None)
    r = np.repeat(np.arange(m), np.diff(Wx.indptr))

    def reset(ctx):
        for w in range(3):
            ctx.set_factor(w, F[w])

    def factors(ctx):
        return [ctx.get_factor(w).tobytes() for w in range(3)]

    def background_steps(ctx):
        ctx.set_weighted_csr(0, Wx.indptr, Wx.indices, X[r, Wx.indices], Wx.data)
        ctx.set_background_weight(0, 0.5)
        ctx.als_step(0.1, 0, 7)
        ctx.als_nnls_step(0.1, 7, 7, 2)
        ctx.als_cg_step(0.1, 0, 7, 2, 0)
        ctx.als_residual_sq(True, False)

    def newton(ctx):
        ctx.newton_step(0.4, 0.0, 0.05, "linear", "logit", 0, 7, 0.2, 1.0, None, None, None, None)
    for ctx in (a, b):
        ctx.newton_clamp_stats(reset=True)
    for step in (lambda c: c.mu_step(0.0, 0.0, 7), newton, lambda c: c.mu_step(0.01, 0.02, 7)):
        background_steps(b)
        b.clear_weight(0)
        reset(a)
        reset(b)
        step(a)
        step(b)
        assert factors(a) == factors(b)
    assert a.newton_clamp_stats(full=True) == b.newton_clamp_stats(full=True)
    assert a.newton_clamp_routes() == b.newton_clamp_routes()
    background_steps(b)                                       # weighted MU: the same weights, the background cleared again
    b.set_background_weight(0, 0)
    a.set_weighted_csr(0, Wx.indptr, Wx.indices, X[r, Wx.indices], Wx.data)
    reset(a)
    reset(b)
    a.mu_weighted_step(0.0, 0.01, 7)
    b.mu_weighted_step(0.0, 0.01, 7)
    assert factors(a) == factors(b)
    background_steps(b)
    for ctx in (a, b):
        ctx.clear_weight(0)
        reset(ctx)
        ctx.hals_step(0.01, 0.02, 7)
    assert factors(a) == factors(b)
    a.close()
    b.close()


def test_background_refusals_leave_the_context_usable(lib):
    m, d, p, k = 40, 50, 30, 6
    rng = np.random.RandomState(2)
    X, Y = _f32(np.abs(rng.randn(m, d))), _f32(np.abs(rng.randn(d, p)))
    F = [_f32(np.abs(rng.randn(n, k))) for n in (m, d, p)]
    Ws = sp.csr_matrix(_f32(0.5 + rng.rand(m, d)) * (rng.rand(m, d) < 0.5))
    ctx = _context(lib, X, Y, F, None, None)
    with pytest.raises(ValueError, match="no CSR weights bound"):
        ctx.set_background_weight(0, 0.5)
    ctx.set_weight(0, Ws.toarray())
    with pytest.raises(ValueError, match="no CSR weights bound"):              # dense weights have no pattern to be outside of
        ctx.set_background_weight(0, 0.5)
    with pytest.raises(ValueError, match="no CSR weights bound"):
        ctx.als_residual_sq(True, False)
    ctx.clear_weight(0)
    r = np.repeat(np.arange(m), np.diff(Ws.indptr))
    ctx.set_weighted_csr(0, Ws.indptr, Ws.indices, X[r, Ws.indices], Ws.data)
    with pytest.raises(ValueError, match="which must be"):
        ctx.set_background_weight(2, 0.5)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            ctx.set_background_weight(0, bad)
        assert ctx.get_background_weight(0) == 0
    with pytest.raises(ValueError, match="below the background weight"):
        ctx.set_background_weight(0, float(Ws.data.min()) + 0.125)
    assert ctx.get_background_weight(0) == 0
    with pytest.raises(ValueError, match="no CSR weights bound"):              # Y is full: its error is cmf_residual_sq's
        ctx.als_residual_sq(True, True)
    ctx.set_background_weight(0, 0.5)
    with pytest.raises(ValueError, match="below the background weight"):       # a refused value leaves the one in effect
        ctx.set_background_weight(0, 2.0)
    assert ctx.get_background_weight(0) == 0.5
    with pytest.raises(NotImplementedError, match=r"cmf_set_background_weight\(ctx, 0, 0\)"):
        ctx.mu_weighted_step(0.0, 0.01, 7)
    with pytest.raises(NotImplementedError, match="background weight"):
        ctx.mu_weighted_step(0.0, 0.01, 1)
    ctx.mu_weighted_step(0.0, 0.01, 4)                                         # the Z sweep does not read X
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.als_step(0.1, 0, 7)
    Rx, Ry = A.Relation(X, Ws), A.Relation(Y, None)
    y64, y32 = (A.step(Rx, Ry, None, None, *F, 0.1, cx=0.5, dtype=dt) for dt in (np.float64, np.float32))
    for w in range(3):
        assert np.abs(ctx.get_factor(w) - y64[w]).max() <= _tol(y32[w], y64[w], k)[0]
    ctx.set_background_weight(0, 0)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.mu_weighted_step(0.0, 0.01, 7)
    assert all(np.isfinite(ctx.get_factor(w)).all() for w in range(3))
    ctx.close()


# ------------------------------------------------------------------ 7. fit through CMF
_fit = {}


def _click_case():
    if not _fit:
        counts, train, test, Y, U0, V0, Z0 = K.clicks(7)
        P, W = K.click_relations(counts, train)
        ones = sp.csr_matrix(train.astype(np.float64))
        Ur, Vr, Zr, _, _ = A.fit(P, Y, W, None, U0, V0, Z0, 15, 2.0, cx=1.0)
        Uo, Vo, _, _, _ = A.fit(P, Y, ones, None, U0, V0, Z0, 15, 2.0)
        _fit.update(counts=counts, train=train, test=test, Y=Y, start=(U0, V0, Z0), ref=(Ur, Vr, Zr),
                    err=sum(A.errors(P, Y, W, None, Ur, Vr, Zr, cx=1.0)),
                    bar=1.3 * max(K.recall_at(Uo @ Vo.T, train, test),
                                  K.recall_at(np.broadcast_to(train.sum(axis=0)[None].astype(np.float64), train.shape), train, test)))
    return _fit


SIGNED = dict(U_non_negative=False, V_non_negative=False, Z_non_negative=False)


@pytest.mark.parametrize("route", ["exact", "cg6", "nnls4"])
def test_fit_on_the_planted_clicks(lib, route):
    """clicks(7) through implicit_confidence, c0 = 1, l2 = 2, k = 8, 15 iterations from the yardstick's start: reconstruction_err_
    within 1e-4 of the yardstick's (the exact route), recall@10 of the held-out clicks above 1.3 x the host's observed-only and
    popularity figures (every route)."""
    import pycmf_amd
    from pycmf_amd import CMF
    c = _click_case()
    R_train, R_test = sp.csr_matrix(c["counts"] * c["train"]), sp.csr_matrix(c["test"].astype(np.float64))
    P, W = pycmf_amd.implicit_confidence(R_train, alpha=1.0)
    kw = dict(n_components=8, solver="als", l2_reg=2.0, max_iter=15, tol=0, x_init="custom", y_init="custom")
    extra = {"exact": SIGNED, "cg6": dict(als_cg_steps=6, **SIGNED), "nnls4": dict(als_nn_sweeps=4)}[route]
    U0, V0, Z0 = (np.abs(f) if route == "nnls4" else f.copy() for f in c["start"])
    model = CMF(**kw, **extra)
    model.fit(P, c["Y"], U=U0, V=V0, Z=Z0, x_entry_weights=W, x_background_weight=1.0)
    assert model.n_iter_ == 15 and np.isfinite(model.reconstruction_err_)
    recall = model.evaluate(R_test, n=(10,), exclude=R_train)["recall@10"]
    print("%s: reconstruction_err_ %.9g (yardstick, exact route: %.9g), recall@10 %.3f against the bar %.3f" % (route, model.reconstruction_err_, c["err"], recall, c["bar"]))
    assert recall > c["bar"]
    if route == "nnls4":
        assert min(model.x_weights.min(), model.components.min(), model.y_weights.min()) >= 0
    if route != "exact":
        return
    assert abs(model.reconstruction_err_ - c["err"]) <= 1e-4 * c["err"]
    for G, R in zip((model.x_weights, model.components, model.y_weights), c["ref"]):
        assert np.abs(G - R).max() <= 1e-3 * np.abs(R).max()
    # fold-in: the U sweep of 10 new users against the fixed V
    P_new, W_new = P[:10], W[:10]
    U2, V2, Z2 = model.transform(P_new, None, x_entry_weights=W_new, x_background_weight=1.0)
    assert V2.tobytes() == model.components.tobytes() and U2.shape == (10, 8)
    Rx, Ry = A.Relation(P_new, W_new), A.Relation(np.zeros((V2.shape[0], 1)), None)
    y64, y32 = (A.sweep(Rx, Ry, np.zeros((10, 8)), V2, np.zeros((1, 8)), "U", 2.0, cx=1.0, dtype=dt) for dt in (np.float64, np.float32))
    tol, _ = _tol(y32, y64, 8, "fold-in")
    print("fold-in: |err| / tol %.3f" % (np.abs(U2 - y64).max() / tol))
    assert np.abs(U2 - y64).max() <= tol


def test_fit_with_a_background_stops_at_the_yardsticks_iteration(lib):
    """clicks(8), tol = 1e-3: the yardstick's ratio (previous - error) / error_at_init at its checks is 4.739e-01, 1.931e-03 and
    1.572e-04 -- 473 tol, 0.93 tol and 0.84 tol away from tol -- so it stops at iteration 30 and rounding cannot decide the test.
    (Seeds 1 .. 8 on the CPU: smallest distances 0.29, 0.17, 0.33, 0.70, 0.30, 0.08, 0.05, 0.84 tol.)"""
    from pycmf_amd import CMF
    tol = 1e-3
    counts, train, _, Y, U0, V0, Z0 = K.clicks(8)
    P, W = K.click_relations(counts, train)
    _, _, _, n_ref, ratios = A.fit(P, Y, W, None, U0, V0, Z0, 200, 2.0, tol=tol, cx=1.0)
    margin = min(abs(r - tol) for r in ratios) / tol
    assert margin >= 0.3 and n_ref == 30, (n_ref, ratios)
    model = CMF(n_components=8, solver="als", l2_reg=2.0, max_iter=200, tol=tol, x_init="custom", y_init="custom", **SIGNED)
    model.fit(P, Y, U=U0.copy(), V=V0.copy(), Z=Z0.copy(), x_entry_weights=W, x_background_weight=1.0)
    print("stops at %d (yardstick %d), smallest distance to tol %.3f tol" % (model.n_iter_, n_ref, margin))
    assert model.n_iter_ == n_ref
