"""ALS on the device (cmf_als_step, cmf_als_normal, cmf_als_layout, CMF(solver="als")) against the float64 yardstick of
als_yardstick.py on float32-rounded inputs.  Tolerance of a full step, per factor (als_yardstick.tolerance, the HALS rule):
tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|) with y32 the float32 run of the same formulas."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
import wmu_yardstick as WM
from test_gpu_wmu import fit_inputs

pytestmark = pytest.mark.gpu

U_, V_, Z_ = 0, 1, 2
NAMES = "UVZ"


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _bind(ctx, which, T, W, native=False):
    """CSR weights carry the data on their pattern (the data slot stays unset); a full relation dense or as native CSR."""
    if W is not None:
        W = sp.csr_matrix(W)
        r = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
        ctx.set_weighted_csr(which, W.indptr, W.indices, np.asarray(T)[r, W.indices], W.data)
        return
    if native:
        ctx.set_option("sparse_mode", 2)
        ctx.set_data(which, sp.csr_matrix(T))
        ctx.set_option("sparse_mode", 0)
        assert ctx.data_layout(which) == (False, True)
        return
    ctx.set_data(which, T)


def _context(lib, X, Y, F, Wx, Wy, piece=0, native_y=False):
    ctx = lib.Context(0)
    if piece:
        ctx.set_option("als_piece", piece)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], F[0].shape[1])
    _bind(ctx, 0, X, Wx)
    _bind(ctx, 1, Y, Wy, native_y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    return ctx


# ------------------------------------------------------------------ 1. exact arithmetic
def _exact_factor(rows, k, salt):
    """One-hot and power-of-two rows, asymmetric: row j holds 2^((j % 4) - 1) at column (7 j + salt) % k, -2^(j % 3) at column
    (3 j + 2) % k (where that is another column) and 1 at column j % k (likewise)."""
    F = np.zeros((rows, k))
    for j in range(rows):
        F[j, j % k] = 1.0
        F[j, (3 * j + 2) % k] = -2.0 ** (j % 3)
        F[j, (7 * j + salt) % k] = 2.0 ** ((j % 4) - 1)
    return F


def _exact_pattern(lengths, cols, rng):
    """A pattern with the given row lengths over ``cols`` columns, weights in {1/4, 1, 4, 16} (exact square roots), data in
    {-4, 1/2, 1, 2}."""
    W = np.zeros((len(lengths), cols))
    T = np.zeros((len(lengths), cols))
    for i, n in enumerate(lengths):
        c = rng.permutation(cols)[:n]
        W[i, c] = rng.choice([0.25, 1.0, 4.0, 16.0], size=n)
        T[i, c] = rng.choice([-4.0, 0.5, 1.0, 2.0], size=n)
    return T, sp.csr_matrix(W)


@pytest.mark.parametrize("k", [7, 40, 128, 256])
def test_normal_equations_are_exact_on_exact_inputs(lib, k):
    """Every product and every partial sum is exactly representable in float32, so H and g are compared with ==: rows of 0, 1, 31,
    32, 33 and 70 entries, the row image (U sweep) and the transposed image beside a second observed side (V sweep)."""
    rng = np.random.RandomState(k)
    lengths = [0, 1, 31, 32, 33, 70]
    l2 = 0.5
    # U sweep: X is 6 x 80 with those row lengths
    m, d, p = 6, 80, 9
    X, Wx = _exact_pattern(lengths, d, rng)
    Y = np.zeros((d, p))
    F = [_exact_factor(m, k, 1), _exact_factor(d, k, 3), _exact_factor(p, k, 5)]
    ctx = _context(lib, X, Y, F, Wx, None)
    H, g = ctx.als_normal(U_, 0, m, l2)
    Hr, gr = A.systems(A.Relation(X, Wx), A.Relation(Y, None), *F, "U", l2)
    kp = H.shape[1]
    assert (H[:, :k, :k] == Hr).all() and (g[:, :k] == gr).all(), "U sweep, k = %d" % k
    pad = H.copy()
    pad[:, :k, :k] = 0
    idx = np.arange(k, kp)
    assert (pad[:, idx, idx] == 1).all() and pad.sum() == m * (kp - k) and (g[:, k:] == 0).all()
    assert (H[0, :k, :k] == l2 * np.eye(k)).all() and (g[0] == 0).all()         # the empty row
    part = ctx.als_normal(U_, 2, 3, l2)                                         # a range inside: the same rows
    assert (part[0] == H[2:5]).all() and (part[1] == g[2:5]).all()
    ctx.close()
    # V sweep: X is 80 x 6 (its TRANSPOSE has those row lengths), Y observed too (6 x 50, its own lengths)
    m, d, p = 80, 6, 50
    Xt, Wxt = _exact_pattern(lengths, m, rng)
    X, Wx = Xt.T.copy(), sp.csr_matrix(Wxt.T)
    Y, Wy = _exact_pattern([33, 0, 1, 50, 32, 7], p, rng)
    F = [_exact_factor(m, k, 1), _exact_factor(d, k, 3), _exact_factor(p, k, 5)]
    ctx = _context(lib, X, Y, F, Wx, Wy)
    H, g = ctx.als_normal(V_, 0, d, l2)
    Hr, gr = A.systems(A.Relation(X, Wx), A.Relation(Y, Wy), *F, "V", l2)
    assert (H[:, :k, :k] == Hr).all() and (g[:, :k] == gr).all(), "V sweep, k = %d" % k
    assert all((H[i] == H[i].T).all() for i in range(d))
    H2, g2 = ctx.als_normal(Z_, 0, p, l2)                                       # the transposed image of Y
    Hr, gr = A.systems(A.Relation(X, Wx), A.Relation(Y, Wy), *F, "Z", l2)
    assert (H2[:, :k, :k] == Hr).all() and (g2[:, :k] == gr).all(), "Z sweep, k = %d" % k
    ctx.close()


# ------------------------------------------------------------------ 2. piece split
@pytest.mark.parametrize("k", [40, 256])
def test_rows_cut_into_pieces(lib, k):
    """Rows of 200 .. 500 entries with "als_piece" = 64: within (L + 16) 2^-24 sum|terms| per element of the yardstick's H and g, bit
    for bit the same when repeated, and more pieces than rows."""
    rng = np.random.RandomState(11 + k)
    m, d, p, l2 = 5, 600, 4, 0.1
    lengths = [200, 333, 500, 257, 64]
    W = np.zeros((m, d))
    for i, n in enumerate(lengths):
        W[i, rng.permutation(d)[:n]] = _f32(0.25 + 3.75 * rng.rand(n))
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    Wx = sp.csr_matrix(W)
    Hr, gr = A.systems(A.Relation(X, Wx), A.Relation(Y, None), *F, "U", l2)
    Ha, ga = A.systems(A.Relation(np.abs(X), Wx), A.Relation(Y, None), F[0], np.abs(F[1]), F[2], "U", l2)    # sum |terms|
    for piece in (64, 0):
        ctx = _context(lib, X, Y, F, Wx, None, piece=piece)
        lay = ctx.als_layout()
        H, g = ctx.als_normal(U_, 0, m, l2)
        H2, g2 = ctx.als_normal(U_, 0, m, l2)
        assert H.tobytes() == H2.tobytes() and g.tobytes() == g2.tobytes()
        if piece:
            assert lay[0] == 64 and lay[1] == sum((n + 63) // 64 for n in lengths) > m and lay[3] == 0, lay
        else:
            assert lay[1] == m, lay
        worst = 0.0
        for i, n in enumerate(lengths):
            bound = (n + 16) * 2.0 ** -24
            worst = max(worst, float((np.abs(H[i, :k, :k] - Hr[i]) / (bound * Ha[i])).max()), float((np.abs(g[i, :k] - gr[i]) / (bound * ga[i])).max()))
        print("k %d piece %d: layout %s, worst |err| / bound %.4f" % (k, piece, lay, worst))
        assert worst <= 1.0
        ctx.close()


# ------------------------------------------------------------------ 2b. rows in more than one chunk
def test_rows_on_both_sides_of_a_chunk_boundary(lib):
    """k = 200 (k_pad = 256: chunks of 2 GiB / 256 KiB = 8192 rows) and 8492 rows of U, so the U sweep runs a chunk of 8192 rows and
    one of 300, each with its own slice of the piece list and of the piece index.  Rows i and i + 8192 (i < 300) carry the same
    pattern, weights and data, lengths cycling through 0, 1, 31, 32, 33, 70; rows 300 .. 8191 hold one entry.  Y is full and zero:
    no shared matrix, so the piece index is what tells a row without information.  A row's arithmetic does not depend on its chunk:
    after the sweep the two blocks are equal with ==, and both agree with the yardstick (als_yardstick.tolerance on those 600
    rows) -- by the exact solves, and by 2 coordinate-descent sweeps from a non-negative start, where the rows of length 0 on
    either side of the boundary are exact zeros."""
    m, d, p, k, twin, cut, l2 = 8492, 80, 4, 200, 300, 8192, 0.1
    rng = np.random.RandomState(17)
    lengths = np.ones(m, dtype=np.int64)
    lengths[:twin] = lengths[cut:] = np.resize([0, 1, 31, 32, 33, 70], twin)
    W, X = np.zeros((m, d)), np.zeros((m, d))
    for i in range(cut):
        c = rng.permutation(d)[:lengths[i]]
        W[i, c], X[i, c] = _f32(0.25 + 3.75 * rng.rand(len(c))), _f32(rng.randn(len(c)))
    W[cut:], X[cut:] = W[:twin], X[:twin]
    Wx, Y = sp.csr_matrix(W), np.zeros((d, p))
    assert (np.diff(Wx.indptr) == lengths).all()
    U0 = _f32(rng.randn(m, k))
    U0[cut:] = U0[:twin]
    rows = np.concatenate((np.arange(twin), np.arange(cut, m)))
    empty = lengths[rows] == 0
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, None)
    for name, nn_sweeps in (("exact", 0), ("nnls", 2)):
        F = [np.abs(U0) if nn_sweeps else U0, _f32(rng.randn(d, k)), _f32(rng.randn(p, k))]
        route = dict(non_negative=bool(nn_sweeps), nn_sweeps=nn_sweeps, rows=rows)
        y64, y32 = (A.sweep(Rx, Ry, *F, "U", l2, **route, dtype=dt) for dt in (np.float64, np.float32))
        ctx = _context(lib, X, Y, F, Wx, None)
        assert ctx.geometry()[3] == 256 and ctx.als_layout()[1] == int((lengths > 0).sum())
        if nn_sweeps:
            ctx.als_nnls_step(l2, A.U_BIT, A.U_BIT, nn_sweeps)
        else:
            ctx.als_step(l2, 0, A.U_BIT)
        got = ctx.get_factor(U_)
        ctx.close()
        tol = A.tolerance(y32, y64, k)
        err = float(np.abs(got[rows] - y64).max())
        print("%s: rows 0 .. 299 and 8192 .. 8491 against the yardstick: |err| / tol %.3f (tol %.3e)" % (name, err / tol, tol))
        assert (got[cut:] == got[:twin]).all(), "%s: %d rows differ from their twins in the other chunk" % (name, int((got[cut:] != got[:twin]).any(axis=1).sum()))
        assert np.isfinite(got).all() and err <= tol
        assert empty.sum() == 100 and (y64[empty] == 0).all() and (got[rows][empty] == 0).all()
        if nn_sweeps:
            assert (got >= 0).all()


# ------------------------------------------------------------------ 3, 5. one full step against the yardstick
SHAPES =[(257, 1031, 77, 7), (128, 3000, 150, 128), (70, 333, 129, 40), (300, 1200, 130, 256)]
_cases = {}


def _case(shape, yform):
    """Signed float32-rounded data and factors.  X observed with a per-row density drawn from [k / 4, 2 k] / d (rows with fewer and
    with more than k entries), non-unit weights, an empty row and an empty column.  Y: 'dense' full, 'csr' full (70 % zeros, held
    as native CSR), 'observed' with non-unit weights, an empty row and an empty column."""
    if (shape, yform) in _cases:
        return _cases[(shape, yform)]
    m, d, p, k = shape
    rng = np.random.RandomState(m + k)
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    dens = rng.uniform(0.25 * k / d, min(0.6, 2.0 * k / d), size=(m, 1))
    Wx = _f32(0.25 + 3.75 * rng.rand(m, d)) * (rng.rand(m, d) < dens)
    Wx[m // 3] = 0
    Wx[:, d // 2] = 0
    Wx = sp.csr_matrix(Wx)
    Wy = None
    if yform == "csr":
        Y = Y * (rng.rand(d, p) < 0.3)
    elif yform == "observed":
        Wy = _f32(0.25 + 3.75 * rng.rand(d, p)) * (rng.rand(d, p) < 0.4)
        Wy[d // 2] = 0
        Wy[:, p // 4] = 0
        Wy = sp.csr_matrix(Wy)
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    _cases[(shape, yform)] = (X, Y, Wx, Wy, F, {})
    return _cases[(shape, yform)]


def _reference(case, l2, mask, nn):
    X, Y, Wx, Wy, F, refs = case
    if (l2, mask, nn) not in refs:
        Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
        refs[(l2, mask, nn)] = tuple(A.step(Rx, Ry, None, None, *F, l2, mask=mask, nn_mask=nn, dtype=dt) for dt in (np.float64, np.float32))
    return refs[(l2, mask, nn)]


def _step_case(lib, shape, yform, mask, nn, piece=0):
    m, d, p, k = shape
    l2 = 0.1
    case = _case(shape, yform)
    X, Y, Wx, Wy, F, _ = case
    y64, y32 = _reference(case, l2, mask, nn)
    ctx = _context(lib, X, Y, F, Wx, Wy, piece=piece, native_y=(yform == "csr"))
    ctx.newton_clamp_stats(reset=True)
    before = [ctx.get_factor(w).tobytes() for w in range(3)]
    ctx.als_step(l2, nn, mask)
    got = [ctx.get_factor(w) for w in range(3)]
    lens = np.diff(Wx.indptr)
    report = []
    for w in range(3):
        if not mask & (1 << w):
            assert got[w].tobytes() == before[w], "factor %s was not swept and changed" % NAMES[w]
            continue
        tol = A.tolerance(y32[w], y64[w], k)
        err = float(np.abs(got[w] - y64[w]).max())
        report.append("%s %.3f" % (NAMES[w], err / tol))
        assert np.isfinite(got[w]).all() and err <= tol, "%s: |err| / tol = %.3f (tol %.3e)" % (NAMES[w], err / tol, tol)
        zero_rows = (y64[w] == 0).all(axis=1)
        assert (got[w][zero_rows] == 0).all(), "%s: rows without observations must stay exact zeros" % NAMES[w]
        if nn & (1 << w):
            assert (got[w] >= 0).all()
    if mask & 1:
        assert (y64[0][m // 3] == 0).all()                       # the unobserved row of X is such a row of U
    clamped = ctx.newton_clamp_stats()[0]
    print("%s Y %s mask %d nn %d: the observed rows of X hold %d .. %d entries (k = %d), %d rows none; |err| / tol %s; clamped rows %d"
          % (shape, yform, mask, nn, lens[lens > 0].min(), lens.max(), k, int((lens == 0).sum()), " ".join(report), clamped))
    assert lens[lens > 0].min() < k < lens.max()
    assert clamped == 0, "the spectral clamp acted on %d rows" % clamped
    return ctx, got


@pytest.mark.parametrize("yform", ["dense", "csr", "observed"])
@pytest.mark.parametrize("shape", SHAPES)
def test_full_step_signed(lib, shape, yform):
    ctx, _ = _step_case(lib, shape, yform, 7, 0)
    ctx.close()


@pytest.mark.parametrize("mask, nn", [(7, 7), (1, 0), (1, 7), (2, 0), (2, 7), (4, 0), (4, 7)])
@pytest.mark.parametrize("shape, yform", [((257, 1031, 77, 7), "observed"), ((70, 333, 129, 40), "dense")])
def test_masks_and_projection(lib, shape, yform, mask, nn):
    ctx, _ = _step_case(lib, shape, yform, mask, nn)
    ctx.close()


@pytest.mark.parametrize("shape, yform", [((128, 3000, 150, 128), "observed"), ((300, 1200, 130, 256), "csr")])
def test_full_step_projected_wide(lib, shape, yform):
    ctx, _ = _step_case(lib, shape, yform, 7, 7)
    ctx.close()


def test_unweighted_step_takes_the_shared_inverse(lib):
    """No observed side at all: every sweep is F = (T B)(G + l2 I)^-1 with the one inverse formed in float64."""
    m, d, p, k = 257, 1031, 77, 7
    rng = np.random.RandomState(2)
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    ctx = _context(lib, X, Y, F, None, None)
    assert ctx.als_layout()[1:] == (0, 0, 0)
    ctx.als_step(0.1, 0, 7)
    y64, y32 = A.step(X, Y, None, None, *F, 0.1), A.step(X, Y, None, None, *F, 0.1, dtype=np.float32)
    for w in range(3):
        assert np.abs(ctx.get_factor(w) - y64[w]).max() <= A.tolerance(y32[w], y64[w], k)
    with pytest.raises(ValueError, match="no observed relation"):
        ctx.als_normal(U_, 0, 1, 0.1)
    ctx.close()


# ------------------------------------------------------------------ 4. repeat
@pytest.mark.parametrize("piece", [0, 32])
def test_a_repeated_step_is_bit_identical(lib, piece):
    shape = (70, 333, 129, 40)
    X, Y, Wx, Wy, F, _ = _case(shape, "observed")
    ctx = _context(lib, X, Y, F, Wx, Wy, piece=piece)
    if piece:
        assert ctx.als_layout()[1] > shape[0]
    runs = []
    for _ in range(2):
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.als_step(0.1, 0, 7)
        ctx.als_step(0.1, 5, 7)
        runs.append([ctx.get_factor(w).tobytes() for w in range(3)])
    assert runs[0] == runs[1]
    ctx.close()


# ------------------------------------------------------------------ 6. fit through CMF
def test_fit_matches_the_float64_yardstick(lib):
    from pycmf_amd import CMF
    X, Y, Wx, _, U, V, Z = fit_inputs(3, m=120, d=150, p=20, k=3, obs=.3)
    l2, iters = 0.05, 10
    Xi, Wref = sp.csr_matrix(X * Wx), sp.csr_matrix(Wx)
    assert Xi.nnz == Wref.nnz
    kw = dict(n_components=3, l2_reg=l2, tol=0, x_init="custom", y_init="custom")
    signed = dict(U_non_negative=False, V_non_negative=False, Z_non_negative=False)
    model = CMF(solver="als", max_iter=iters, **signed, **kw)
    Ug, Vg, Zg = model.fit_transform(Xi, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights="observed")
    Ur, Vr, Zr, n_iter, _ = A.fit(X, Y, Wref, None, U, V, Z, iters, l2)
    assert model.n_iter_ == n_iter == iters
    ref = sum(A.errors(X, Y, Wref, None, Ur, Vr, Zr))
    print("fit: reconstruction_err_ %.9g, yardstick %.9g, relative %.2e" % (model.reconstruction_err_, ref, abs(model.reconstruction_err_ - ref) / ref))
    assert abs(model.reconstruction_err_ - ref) <= 1e-4 * ref
    for G, R in ((Ug, Ur), (Vg, Vr), (Zg, Zr)):
        assert np.isfinite(G).all() and np.abs(G - R).max() <= 1e-3 * np.abs(R).max()
    # the weighted objective step by step through the C ABI: non-increasing up to twice the residual tolerance of the error pass
    ctx = _context(lib, X, Y, [U, V, Z], Wref, None)

    def objective():
        F = [ctx.get_factor(w) for w in range(3)]
        e = ctx.weighted_residual_sq(True, False)[0] + ctx.residual_sq()[1]
        tol = sum(WM.resid_tol(3, *WM.residual_terms(T, W, P, Q)[::-1]) for T, W, P, Q in ((X, Wref, F[0], F[1]), (Y, None, F[1], F[2])))
        return 0.5 * e + 0.5 * l2 * sum((G ** 2).sum() for G in F), tol
    prev, _ = objective()
    for it in range(iters):
        ctx.als_step(l2, 0, 7)
        cur, tol = objective()
        assert cur <= prev + 2 * tol, (it, prev, cur, tol)
        prev = cur
    ctx.close()
    # better than the multiplicative updates after 300 iterations, on the cells it never saw (float64: 0.066 against 0.084)
    unobserved = Wx == 0
    mu = CMF(solver="mu", max_iter=300, **kw)
    Um, Vm, _ = mu.fit_transform(Xi, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights="observed")
    rmse = [float(np.sqrt((((X - P @ Q.T) ** 2)[unobserved]).mean())) for P, Q in ((Ug, Vg), (Um, Vm))]
    print("RMSE on the unobserved cells: ALS after %d iterations %.4f, weighted MU after 300 %.4f" % (iters, rmse[0], rmse[1]))
    assert rmse[0] < rmse[1]
    # transform: V and Z fixed, U re-fitted on the observed entries of new rows
    U2, V2, Z2 = model.transform(Xi[:50], None, x_entry_weights="observed")
    assert V2.tobytes() == model.components.tobytes() and Z2.tobytes() == model.y_weights.tobytes()
    assert U2.shape == (50, 3) and np.isfinite(U2).all()
    # held-out evaluation on the fitted model
    X_test = sp.csr_matrix(X * (1 - Wx) * (X > np.percentile(X, 95)))
    res = model.evaluate(X_test, exclude=Xi)
    assert np.isfinite(res["auc"]) and 0.0 <= res["auc"] <= 1.0


# ------------------------------------------------------------------ 7. stopping test
@pytest.mark.parametrize("tol, seed, n_listed", [(1e-3, 3, 20), (1e-4, 6, 30), (3e-4, 7, 30)])
def test_fit_stops_at_the_yardsticks_iteration(lib, tol, seed, n_listed):
    from pycmf_amd import CMF
    X, Y, Wx, Wy, U, V, Z = fit_inputs(seed)
    _, _, _, n_ref, ratios = A.fit(X, Y, Wx, Wy, U, V, Z, 200, 0.05, tol=tol, alpha=0.5)
    # the yardstick alone must be far from the crossing at every check, or rounding would decide the test
    margin = min(abs(r - tol) for r in ratios) / tol
    assert margin >= 0.2 and n_ref == n_listed, (n_ref, margin)
    model = CMF(n_components=5, solver="als", l2_reg=0.05, max_iter=200, tol=tol, x_init="custom", y_init="custom",
                U_non_negative=False, V_non_negative=False, Z_non_negative=False)
    model.fit(X, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights=Wx, y_entry_weights=Wy)
    print("tol %g seed %d: stops at %d (yardstick %d), smallest distance to tol %.3f tol" % (tol, seed, model.n_iter_, n_ref, margin))
    assert model.n_iter_ == n_ref


# ------------------------------------------------------------------ 8. other paths untouched, refusals
def test_other_solvers_are_untouched_by_als_steps(lib):
    """Context b runs ALS steps in between (per-row route with CSR weights bound, then the shared route without), its factors reset
    afterwards; context a never hears of ALS.  cmf_mu_step, cmf_newton_step (per-row Hessians: a logit link) and cmf_hals_step
    agree byte for byte, and so do the clamp statistics of the Newton steps."""
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

    def newton(ctx):
        ctx.newton_step(0.4, 0.0, 0.05, "linear", "logit", 0, 7, 0.2, 1.0, None, None, None, None)
    for ctx in (a, b):
        ctx.newton_clamp_stats(reset=True)
    for step in (lambda c: c.mu_step(0.0, 0.0, 7), newton, lambda c: c.mu_step(0.01, 0.02, 7)):
        b.set_weighted_csr(0, Wx.indptr, Wx.indices, X[r, Wx.indices], Wx.data)
        b.als_step(0.1, 0, 7)
        b.als_step(0.1, 7, 7)
        b.clear_weight(0)
        reset(a)
        reset(b)
        step(a)
        step(b)
        assert factors(a) == factors(b)
    assert a.newton_clamp_stats(full=True) == b.newton_clamp_stats(full=True)
    assert a.newton_clamp_routes() == b.newton_clamp_routes()
    b.als_step(0.1, 0, 7)                                    # no weights bound: the shared route
    reset(a)
    reset(b)
    a.hals_step(0.01, 0.02, 7)
    b.hals_step(0.01, 0.02, 7)
    assert factors(a) == factors(b)
    a.close()
    b.close()


def test_refusals_leave_the_context_usable(lib):
    m, d, p, k = 40, 50, 30, 6
    rng = np.random.RandomState(2)
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    ctx = lib.Context(0)
    ctx.set_problem(40, 50, 30, 300)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.als_step(0.1, 0, 7)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.als_layout()
    ctx.set_problem(m, d, p, k)
    for w in range(3):
        ctx.set_factor(w, F[w])
    with pytest.raises(ValueError, match="neither data nor CSR weights"):
        ctx.als_step(0.1, 0, 7)
    ctx.set_data(0, X)
    ctx.set_data(1, Y)
    with pytest.raises(ValueError, match="l2 must be positive"):
        ctx.als_step(0.0, 0, 7)
    for mask in (0, 8):
        with pytest.raises(ValueError, match="update_mask"):
            ctx.als_step(0.1, 0, mask)
    W = (rng.rand(m, d) < 0.5).astype(float)
    ctx.set_weight(0, W)
    with pytest.raises(NotImplementedError, match="DENSE weights"):
        ctx.als_step(0.1, 0, 7)
    ctx.als_step(0.1, 0, A.Z_BIT)                            # the Z sweep does not read X
    assert np.abs(ctx.get_factor(Z_) - A.step(X, Y, None, None, *F, 0.1, mask=A.Z_BIT)[2]).max() <= 1e-4
    ctx.clear_weight(0)
    Ws = sp.csr_matrix(W)
    r = np.repeat(np.arange(m), np.diff(Ws.indptr))
    ctx.set_weighted_csr(0, Ws.indptr, Ws.indices, X[r, Ws.indices], Ws.data)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.als_step(0.1, 0, 7)
    y64, y32 = A.step(X, Y, Ws, None, *F, 0.1), A.step(X, Y, Ws, None, *F, 0.1, dtype=np.float32)
    for w in range(3):
        assert np.abs(ctx.get_factor(w) - y64[w]).max() <= A.tolerance(y32[w], y64[w], k)
    with pytest.raises(ValueError, match="rows out of range"):
        ctx.als_normal(U_, m - 1, 2, 0.1)
    ctx.close()


def test_dense_entry_weights_fit_like_their_pattern(lib):
    """CMF(solver='als') takes a dense W through the CSR of its non-zeros: the fit equals the one under the sparse W bit for bit."""
    from pycmf_amd import CMF
    X, Y, Wx, Wy, U, V, Z = fit_inputs(2)
    kw = dict(n_components=5, solver="als", l2_reg=0.05, max_iter=3, tol=0, x_init="custom", y_init="custom", V_non_negative=False)
    fits = []
    for W in (Wx * 1.5, sp.csr_matrix(Wx * 1.5)):
        model = CMF(**kw)
        fits.append([G.tobytes() for G in model.fit_transform(X, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights=W)])
        assert np.isfinite(model.reconstruction_err_)
    assert fits[0] == fits[1]
