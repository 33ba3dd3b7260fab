"""Multiplicative updates with per-entry weights on the device (cmf_mu_weighted_step, cmf_weighted_residual_sq,
CMF.fit(x_entry_weights=...)) against the float64 yardstick of wmu_yardstick.py on float32-rounded inputs.  The tolerances are
derived there; EVERY element of every updated factor is compared: exactly 0 where the yardstick is exactly 0, within tau relative
elsewhere."""
import numpy as np
import pytest
import scipy.sparse as sp

import wmu_yardstick as WM

pytestmark = pytest.mark.gpu

U_, V_, Z_ = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _problem(m, d, p, k, seed):
    """Non-zero values in [1e-3, 1e3]; zeros in the data, an empty row and an empty column; a zero factor row (test_gpu_kl's)."""
    rng = np.random.RandomState(seed)
    X, Y = (np.clip(np.abs(rng.randn(*s)) * (rng.rand(*s) < 0.8), 0, 1e3) for s in ((m, d), (d, p)))
    X[(X > 0) & (X < 1e-3)] = 1e-3
    Y[(Y > 0) & (Y < 1e-3)] = 1e-3
    X[m // 3] = 0
    X[:, d // 2] = 0
    Y[d // 5] = 0
    Y[:, p // 2] = 0
    F = [np.clip(np.abs(rng.randn(r, k)), 1e-3, 1e3) for r in (m, d, p)]
    F[0][1] = 0
    return _f32(X), _f32(Y), [_f32(f) for f in F]


def _weights(shape, seed, sparse):
    """rand in [0.25, 4) times a Bernoulli(0.6) mask, one all-zero row and one all-zero column.  sparse: the same as CSR, with some
    stored weights equal to 0 (the data has zeros of its own under the pattern)."""
    rng = np.random.RandomState(seed)
    W = _f32((0.25 + 3.75 * rng.rand(*shape)) * (rng.rand(*shape) < 0.6))
    W[shape[0] // 4] = 0
    W[:, shape[1] // 3] = 0
    if not sparse:
        return W
    W = sp.csr_matrix(W)
    W.data[rng.rand(W.nnz) < 0.05] = 0.0
    assert (W.data == 0).any() and W.nnz == len(W.data)
    return W


CONFIGS = {"dense/dense": (False, False), "csr/csr": (True, True), "csr/none": (True, None), "none/dense": (None, False)}


def _config(X, Y, config, seed):
    sx, sy = CONFIGS[config]
    return (None if sx is None else _weights(X.shape, seed, sx)), (None if sy is None else _weights(Y.shape, seed + 1, sy))


def _bind(ctx, which, T, W):
    """Data and weights of one relation.  CSR weights carry the data on their pattern: the data slot is left unset."""
    if sp.issparse(W):
        W = W.tocsr()
        r = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
        ctx.set_weighted_csr(which, W.indptr, W.indices, np.asarray(T)[r, W.indices], W.data)
        return
    ctx.set_data(which, T)
    if W is not None:
        ctx.set_weight(which, W)


def _context(lib, X, Y, F, Wx, Wy, split=0):
    ctx = lib.Context(0)
    if split:
        ctx.set_option("wmu_split", split)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], F[0].shape[1])
    _bind(ctx, 0, X, Wx)
    _bind(ctx, 1, Y, Wy)
    for w in range(3):
        ctx.set_factor(w, F[w])
    return ctx


def _check(gpu, ref, tol, label):
    """Every element: exact zero where the yardstick is exactly zero, |gpu - ref| <= tol * ref elsewhere.  Returns worst |err| / tol."""
    assert gpu.shape == ref.shape and np.isfinite(gpu).all(), label
    zero = ref == 0
    assert (gpu[zero] == 0).all(), "%s: %d elements are not exactly 0 where the yardstick is" % (label, int((gpu[zero] != 0).sum()))
    ratio = np.abs(gpu[~zero] - ref[~zero]) / (tol * ref[~zero])
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, "%s: worst |err| / tau = %.3f" % (label, worst)
    return worst


SHAPES = [(257, 1031, 77, 7), (300, 5000, 130, 256), (128, 3000, 150, 128), (70, 333, 129, 40), (100, 20000, 60, 16)]


# ------------------------------------------------------------------ 1. single sweeps and the full step
@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("m, d, p, k", SHAPES)
def test_single_sweeps_and_the_full_step(lib, m, d, p, k, config, l1, l2):
    X, Y, F = _problem(m, d, p, k, seed=k + m)
    Wx, Wy = _config(X, Y, config, seed=m)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    lay = ctx.mu_weighted_layout()
    if (m, d) == (100, 20000) and config == "dense/dense":
        assert lay[0] > 1 and lay[2] > 1, lay           # few output rows, long stream: the stream is cut into shares
    if config == "csr/csr":
        assert lay[:3] == (1, 1, 1) and ctx.data_layout(0) == (False, False) and ctx.data_layout(1) == (False, False)
    tU = tZ = WM.tau(k, d)
    tV = WM.tau(k, m + p)
    for mask, name in ((WM.V_BIT, "V"), (WM.U_BIT, "U"), (WM.Z_BIT, "Z"), (7, "full")):
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.mu_weighted_step(l1, l2, mask)
        got = [ctx.get_factor(w) for w in range(3)]
        ref = WM.step(X, Y, Wx, Wy, F[0], F[1], F[2], l1, l2, mask)
        full = mask == 7
        tols = (tU + 3 * tV if full else tU, tV, tZ + 3 * tV if full else tZ)
        worst = []
        for w, bit in ((U_, WM.U_BIT), (V_, WM.V_BIT), (Z_, WM.Z_BIT)):
            if mask & bit:
                worst.append(_check(got[w], ref[w], tols[w], "%s sweep, factor %d" % (name, w)))
            else:
                assert got[w].tobytes() == F[w].tobytes()
        print("(%d, %d, %d, k=%d) %s l1=%g l2=%g %s: shares %s, worst |err| / tau = %s"
              % (m, d, p, k, config, l1, l2, name, lay[:3], ["%.4f" % x for x in worst]))
    ctx.close()


# ------------------------------------------------------------------ 2. weighted residual
@pytest.mark.parametrize("config", ["dense/dense", "csr/csr", "csr/none", "none/dense"])
@pytest.mark.parametrize("m, d, p, k", SHAPES)
def test_weighted_residual(lib, m, d, p, k, config):
    X, Y, F = _problem(m, d, p, k, seed=3 * k + 1)
    Wx, Wy = _config(X, Y, config, seed=m + 7)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    ex, ey = ctx.weighted_residual_sq()
    for name, got, (T, W, A, B) in (("x", ex, (X, Wx, F[0], F[1])), ("y", ey, (Y, Wy, F[1], F[2]))):
        ref, wes = WM.residual_terms(T, W, A, B)
        tol = WM.resid_tol(k, wes, ref)
        print("(%d, %d, %d, k=%d) %s E_%s: |err| / tol = %.4f" % (m, d, p, k, config, name, abs(got - ref) / tol))
        assert abs(got - ref) <= tol
    assert ctx.weighted_residual_sq(True, False) == (ex, 0.0) and ctx.weighted_residual_sq(False, True) == (0.0, ey)
    ctx.close()


# ------------------------------------------------------------------ 3. exact arithmetic
@pytest.mark.parametrize("k", [7, 100, 200])
@pytest.mark.parametrize("dense_owner", ["V", "UZ"])
def test_exact_arithmetic_pins_the_orientation_and_the_k_pairing(lib, k, dense_owner):
    """test_gpu_kl's construction -- every product A_r . B_c is a power of two (one factor of each pair has one-hot rows, all entries
    are powers of two), T is that product times a power of two -- with weights 2^randint(-2, 3) Bernoulli(0.7): every term of every
    numerator and denominator is a multiple of 2^-4 and every sum stays below 2^20 (asserted), so every sum is exact in float32
    whatever the order and the result is determined bit for bit.  The factors are asymmetric, so a slip in the k pairing of the two
    products, in the transposed access of W or P, or in the output column map changes it."""
    m, d, p = 70, 333, 40
    rng = np.random.RandomState(k)

    def dense(r):
        return 2.0 ** rng.randint(0, 4, size=(r, k))

    def onehot(r):
        F = np.zeros((r, k))
        F[np.arange(r), rng.randint(0, k, size=r)] = 2.0 ** rng.randint(0, 3, size=r)
        return F
    F = [onehot(m), dense(d), onehot(p)] if dense_owner == "V" else [dense(m), onehot(d), dense(p)]
    X = (F[0] @ F[1].T) * 2.0 ** rng.randint(-2, 3, size=(m, d)) * (rng.rand(m, d) < 0.7)
    Y = (F[1] @ F[2].T) * 2.0 ** rng.randint(-2, 3, size=(d, p)) * (rng.rand(d, p) < 0.7)
    Wx = 2.0 ** rng.randint(-2, 3, size=(m, d)) * (rng.rand(m, d) < 0.7)
    Wy = 2.0 ** rng.randint(-2, 3, size=(d, p)) * (rng.rand(d, p) < 0.7)
    f32 = np.float32

    def expect(Fw, num, den):
        for S in (num, den):                              # the premise, from the float64 side alone
            assert S.max() < 2.0 ** 20 and (S * 16 == np.round(S * 16)).all()
        den = den.astype(f32).copy()
        den[den == 0] = f32(WM.EPS)
        return (Fw.astype(f32) * (num.astype(f32) / den)).astype(np.float64)
    for sparse in (False, True):
        wx, wy = (sp.csr_matrix(Wx), sp.csr_matrix(Wy)) if sparse else (Wx, Wy)
        ctx = _context(lib, X, Y, F, wx, wy)
        ctx.mu_weighted_step(0.0, 0.0, WM.V_BIT)           # V from the old U, Z
        nx, dx = WM.products(X, Wx, F[0], F[1], trans=True)
        ny, dy = WM.products(Y, Wy, F[1], F[2])
        assert (ctx.get_factor(V_) == expect(F[1], nx + ny, dx + dy)).all()
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.mu_weighted_step(0.0, 0.0, WM.U_BIT | WM.Z_BIT)
        assert (ctx.get_factor(U_) == expect(F[0], *WM.products(X, Wx, F[0], F[1]))).all()
        assert (ctx.get_factor(Z_) == expect(F[2], *WM.products(Y, Wy, F[1], F[2], trans=True))).all()
        ctx.close()


# ------------------------------------------------------------------ 4. repeated steps
@pytest.mark.parametrize("sparse, split", [(False, 1), (False, 0), (False, 3), (True, 0)])
def test_a_repeated_step_is_bit_identical(lib, sparse, split):
    m, d, p, k = 300, 2100, 130, 40
    X, Y, F = _problem(m, d, p, k, seed=9)
    Wx, Wy = _weights(X.shape, 1, sparse), _weights(Y.shape, 2, sparse)
    ctx = _context(lib, X, Y, F, Wx, Wy, split=split)
    lay = ctx.mu_weighted_layout()
    if not sparse:
        assert (lay[0] == 1) == (split == 1) and (split != 3 or lay[0] == 3), lay
    runs = []
    for _ in range(2):
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.mu_weighted_step(0.01, 0.02, 7)
        ctx.mu_weighted_step(0.01, 0.02, 7)
        runs.append([ctx.get_factor(w).tobytes() for w in range(3)] + [np.array(ctx.weighted_residual_sq()).tobytes()])
    assert runs[0] == runs[1]
    # every share count stays within the tolerance of the yardstick (two steps: the second starts from factors the first left)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.mu_weighted_step(0.01, 0.02, 7)
    ref = WM.step(X, Y, Wx, Wy, *F, 0.01, 0.02)
    tU, tV = WM.tau(k, d), WM.tau(k, m + p)
    for w, t in ((U_, tU + 3 * tV), (V_, tV), (Z_, tU + 3 * tV)):
        _check(ctx.get_factor(w), ref[w], t, "split %d, factor %d" % (split, w))
    ctx.close()


# ------------------------------------------------------------------ 5. W == 1 reduces to the ordinary step
@pytest.mark.parametrize("ones", ["array", "flag"])
@pytest.mark.parametrize("m, d, p, k", [(257, 1031, 77, 7), (128, 3000, 150, 128)])
def test_unit_weights_reduce_to_the_ordinary_step(lib, m, d, p, k, ones):
    """A dense array of ones, and no weights at all (the kernels' W == 1 flag): both within tau of the yardstick at W = 1, which is
    the reference's MU step (test_wmu_host.py) -- and so is cmf_mu_step on the same inputs.  Not bitwise: the association differs."""
    X, Y, F = _problem(m, d, p, k, seed=m + 1)
    Wx, Wy = (np.ones(X.shape), np.ones(Y.shape)) if ones == "array" else (None, None)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    ref = WM.step(X, Y, None, None, *F, 0.05, 0.1)
    tU, tV = WM.tau(k, d), WM.tau(k, m + p)
    tols = (tU + 3 * tV, tV, tU + 3 * tV)
    ctx.mu_weighted_step(0.05, 0.1, 7)
    worst_w = [_check(ctx.get_factor(w), ref[w], tols[w], "weighted step, factor %d" % w) for w in range(3)]
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.mu_step(0.05, 0.1, 7)
    worst_o = [_check(ctx.get_factor(w), ref[w], tols[w], "ordinary step, factor %d" % w) for w in range(3)]
    print("(%d, %d, %d, k=%d) ones as %s: worst |err| / tau weighted %s, ordinary %s"
          % (m, d, p, k, ones, ["%.4f" % x for x in worst_w], ["%.4f" % x for x in worst_o]))
    ctx.close()


# ------------------------------------------------------------------ 6. existing paths untouched
def test_existing_paths_are_untouched_by_weights_and_weighted_steps(lib):
    """test_frobenius_path_is_untouched_by_a_kl_step's scheme: context b has weights bound and runs weighted steps in between (their
    results thrown away), context a knows nothing of weights; mu_step from a captured graph, mu_kl_step, kl_divergence and
    residual_sq agree byte for byte."""
    m, d, p, k = 200, 300, 90, 12
    X, Y, F = _problem(m, d, p, k, seed=41)
    a, b = _context(lib, X, Y, F, None, None), _context(lib, X, Y, F, _weights(X.shape, 5, False), _weights(Y.shape, 6, False))

    def reset(ctx, G=F):
        for w in range(3):
            ctx.set_factor(w, G[w])

    def factors(ctx):
        return [ctx.get_factor(w).tobytes() for w in range(3)]
    for ctx in (a, b):
        ctx.set_option("graph", 1)
    for _ in range(3):
        a.mu_step(0.0, 0.0, 7)
    ra = a.residual_sq()
    for _ in range(3):                   # b: the same Frobenius steps first (its step graph is captured), then weighted work in between
        b.mu_step(0.0, 0.0, 7)
    assert factors(b) == factors(a)
    reset(a)
    reset(b)
    for _ in range(3):
        a.mu_step(0.0, 0.0, 7)
        keep = [b.get_factor(w) for w in range(3)]
        b.mu_weighted_step(0.01, 0.02, 7)
        b.weighted_residual_sq()
        reset(b, keep)
        b.mu_step(0.0, 0.0, 7)
    assert factors(b) == factors(a)
    assert b.residual_sq() == a.residual_sq() == ra
    reset(a)
    reset(b)
    b.mu_weighted_step(0.0, 0.0, 7)
    reset(b)
    a.mu_kl_step(0.0, 0.0, 7)
    b.mu_kl_step(0.0, 0.0, 7)
    assert factors(b) == factors(a) and b.kl_divergence() == a.kl_divergence()
    a.close()
    b.close()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_context_usable(lib):
    ctx = lib.Context(0)
    ctx.set_problem(40, 50, 30, 300)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.mu_weighted_step(0.0, 0.0, 7)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.weighted_residual_sq()
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.mu_weighted_layout()
    X, Y, F = _problem(40, 50, 30, 6, seed=2)
    Wx = _weights(X.shape, 3, False)
    ctx.set_problem(40, 50, 30, 6)
    for w in range(3):
        ctx.set_factor(w, F[w])
    with pytest.raises(ValueError, match="X has not been set"):
        ctx.mu_weighted_step(0.0, 0.0, 7)
    with pytest.raises(ValueError, match="X has not been set"):
        ctx.weighted_residual_sq()
    with pytest.raises(ValueError, match="set the data first"):       # dense weights before the data
        ctx.set_weight(0, Wx)
    with pytest.raises(ValueError, match="no dense weight image"):
        ctx.get_weight_block(0, 0, 1, 0, 1)
    ctx.set_data(0, X)
    ctx.set_weight(0, Wx)
    assert (ctx.get_weight_block(0, 3, 5, 7, 11) == Wx[3:8, 7:18]).all()
    with pytest.raises(ValueError, match="Y has not been set"):
        ctx.mu_weighted_step(0.0, 0.0, WM.Z_BIT)
    ctx.mu_weighted_step(0.0, 0.0, WM.U_BIT)               # the X side alone serves a U sweep
    _check(ctx.get_factor(U_), WM.step(X, Y, Wx, None, *F, mask=WM.U_BIT)[0], WM.tau(6, 50), "U sweep without Y")
    # an unweighted side held only as native CSR
    ctx.set_option("sparse_mode", 2)
    ctx.set_data(1, sp.csr_matrix(Y))
    assert ctx.data_layout(1) == (False, True)
    with pytest.raises(NotImplementedError, match="native CSR"):
        ctx.mu_weighted_step(0.0, 0.0, 7)
    ctx.set_option("sparse_mode", 0)
    ctx.set_data(1, Y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.mu_weighted_step(0.0, 0.0, 7)
    _check(ctx.get_factor(V_), WM.step(X, Y, Wx, None, *F)[1], WM.tau(6, 70), "V after the refusals")
    ctx.clear_weight(0)                                    # back to unweighted: W == 1 on both sides
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.mu_weighted_step(0.0, 0.0, 7)
    _check(ctx.get_factor(V_), WM.step(X, Y, None, None, *F)[1], WM.tau(6, 70), "V after clear_weight")
    ctx.close()


# ------------------------------------------------------------------ 8 - 10. fits
def fit_inputs(seed, m=60, d=90, p=20, k=5, obs=.3):
    r = np.random.RandomState(seed)
    Ut, Vt, Zt = (np.abs(r.randn(n, 3)) for n in (m, d, p))
    X = _f32(Ut @ Vt.T + .1 * np.abs(r.randn(m, d))); Y = _f32(Vt @ Zt.T + .1 * np.abs(r.randn(d, p)))
    Wx = (r.rand(m, d) < obs).astype(float); Wy = _f32(r.rand(d, p) + .5)
    U, V, Z = (_f32(np.abs(r.randn(n, k)) + .1) for n in (m, d, p))
    return X, Y, Wx, Wy, U, V, Z


@pytest.mark.parametrize("how", ["dense", "observed"])
def test_fit_matches_the_float64_yardstick(lib, how):
    from pycmf_amd import CMF
    X, Y, Wx, Wy, U, V, Z = fit_inputs(7, m=200, d=310, p=45, k=12)
    if how == "observed":                       # X as the sparse matrix of its observed entries, Y unweighted
        Xi, kw = sp.csr_matrix(X * Wx), dict(x_entry_weights="observed")
        Wx_ref, Wy = sp.csr_matrix(Wx), None
        assert Xi.nnz == Wx_ref.nnz
    else:
        Xi, kw, Wx_ref = X, dict(x_entry_weights=Wx, y_entry_weights=Wy), Wx
    model = CMF(n_components=12, solver="mu", max_iter=20, tol=0, x_init="custom", y_init="custom")
    Ug, Vg, Zg = model.fit_transform(Xi, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), **kw)
    Ur, Vr, Zr, n_iter, _ = WM.fit(X, Y, Wx_ref, Wy, U, V, Z, 20, 0)
    assert model.n_iter_ == n_iter == 20
    ref = sum(WM.errors(X, Y, Wx_ref, Wy, Ur, Vr, Zr))
    print("fit %s: reconstruction_err_ %.9g, yardstick %.9g, relative %.2e" % (how, model.reconstruction_err_, ref, abs(model.reconstruction_err_ - ref) / ref))
    assert abs(model.reconstruction_err_ - ref) <= 1e-4 * ref
    for G, R in ((Ug, Ur), (Vg, Vr), (Zg, Zr)):
        assert np.isfinite(G).all() and (G >= 0).all() and np.abs(G - R).max() <= 1e-3 * np.abs(R).max()
    # the weighted objective (l1 = l2 = 0: (E_x + E_y) / 2) step by step through the C ABI: non-increasing up to twice the residual tolerance
    ctx = _context(lib, X, Y, [U, V, Z], Wx_ref, Wy)
    prev = sum(ctx.weighted_residual_sq())
    for it in range(20):
        ctx.mu_weighted_step(0.0, 0.0, 7)
        F = [ctx.get_factor(w) for w in range(3)]
        tol = sum(WM.resid_tol(12, *WM.residual_terms(T, W, A, B)[::-1]) for T, W, A, B in ((X, Wx_ref, F[0], F[1]), (Y, Wy, F[1], F[2])))
        cur = sum(ctx.weighted_residual_sq())
        assert cur <= prev + 2 * tol, (it, prev, cur, tol)
        prev = cur
    ctx.close()
    # transform: V fixed, U re-fitted on the observed entries of new rows
    X_new = Xi[:50]
    w_new = "observed" if how == "observed" else Wx[:50]
    U2, V2, Z2 = model.transform(X_new, None, x_entry_weights=w_new)
    assert V2.tobytes() == model.components.tobytes() and Z2.tobytes() == model.y_weights.tobytes()
    assert U2.shape == (50, 12) and np.isfinite(U2).all() and (U2 >= 0).all()
    # held-out evaluation on the fitted model: the unobserved cells with a large true value as the test split
    X_train = sp.csr_matrix(X * Wx)
    X_test = sp.csr_matrix(X * (1 - Wx) * (X > np.percentile(X, 95)))
    res = model.evaluate(X_test, exclude=X_train)
    assert np.isfinite(res["auc"]) and 0.0 <= res["auc"] <= 1.0


@pytest.mark.parametrize("tol, seed, n_listed", [(3e-3, 5, 70), (3e-3, 6, 80), (1e-3, 1, 90)])
def test_fit_stops_at_the_yardsticks_iteration(lib, tol, seed, n_listed):
    from pycmf_amd import CMF
    X, Y, Wx, Wy, U, V, Z = fit_inputs(seed)
    _, _, _, n_ref, ratios = WM.fit(X, Y, Wx, Wy, U, V, Z, 200, tol, alpha=0.5)
    # the yardstick alone must be far from the crossing at every check, or rounding would decide the test
    margin = min(abs(r - tol) for r in ratios) / tol
    assert margin >= 0.2 and n_ref == n_listed, (n_ref, margin)
    model = CMF(n_components=5, solver="mu", max_iter=200, tol=tol, x_init="custom", y_init="custom")
    model.fit(X, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights=Wx, y_entry_weights=Wy)
    print("tol %g seed %d: stops at %d (yardstick %d), smallest distance to tol %.3f tol" % (tol, seed, model.n_iter_, n_ref, margin))
    assert model.n_iter_ == n_ref


def test_more_than_256_components_is_not_implemented(lib):
    from pycmf_amd import CMF
    X, Y, Wx, _, _, _, _ = fit_inputs(1)
    model = CMF(n_components=300, solver="mu", max_iter=2, x_init="random", y_init="random", random_state=0)
    with pytest.raises(NotImplementedError, match="k_pad"):
        model.fit(X, Y, x_entry_weights=Wx)


def test_a_weighted_fit_predicts_the_unobserved_cells(lib):
    """The point of it all: 30 % of a planted rank-3 X observed.  The fit on the observed cells recovers the others; the fit that
    takes the missing cells as zeros does not (float64 yardstick: RMSE 0.084 against 1.82, rms of X there 2.45)."""
    from pycmf_amd import CMF
    X, Y, Wx, _, U, V, Z = fit_inputs(3, m=120, d=150, p=20, k=3, obs=.3)
    unobserved = Wx == 0

    def rmse(Xfit, **kw):
        model = CMF(n_components=3, solver="mu", max_iter=300, tol=0, x_init="custom", y_init="custom")
        Ug, Vg, _ = model.fit_transform(Xfit, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), **kw)
        return float(np.sqrt((((X - Ug @ Vg.T) ** 2)[unobserved]).mean()))
    weighted, zeros = rmse(X, x_entry_weights=Wx), rmse(X * Wx)
    print("RMSE on the unobserved cells: weighted fit %.4f, missing-as-zeros fit %.4f" % (weighted, zeros))
    assert weighted < 0.5 * zeros


# ------------------------------------------------------------------ 11. memory
def test_a_sparse_observed_relation_never_takes_a_dense_image(lib):
    m, d, p, k = 20000, 30000, 64, 32
    rng = np.random.RandomState(0)
    X = sp.csr_matrix((rng.rand(200000) + 0.1, (rng.randint(0, m, 200000), rng.randint(0, d, 200000))), shape=(m, d))
    X.sum_duplicates()                                      # (a handful of cells drawn twice)
    X.data = _f32(X.data)
    X.data[:7] = 0.0                                        # observed zeros
    Y = _f32(rng.rand(d, p))
    F = [_f32(rng.rand(r, k) + 0.1) for r in (m, d, p)]
    from pycmf_amd.solver_shell import resolve_entry_weights
    ew = resolve_entry_weights(X, "observed", "x")
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    ctx.set_weighted_csr(0, ew.indptr, ew.indices, ew.t, ew.w)
    ctx.set_data(1, Y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.mu_weighted_step(0.0, 0.0, 7)
    lay = ctx.mu_weighted_layout()
    mp, dp, _, _ = ctx.geometry()
    assert lay[3] < 0.01 * 4.0 * mp * dp, lay
    assert ctx.data_layout(0) == (False, False)             # neither a dense image nor a data-slot CSR pair: the weights' own buffers
    Wx = sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape)
    ref = WM.step(X, Y, Wx, None, *F)
    tU, tV = WM.tau(k, d), WM.tau(k, m + p)
    worst = [_check(ctx.get_factor(w), ref[w], t, "factor %d" % w) for w, t in ((U_, tU + 3 * tV), (V_, tV), (Z_, tU + 3 * tV))]
    print("observed 2e5 of %d x %d: scratch %.2f MB (1 %% of the dense product: %.1f MB), worst |err| / tau %s"
          % (m, d, lay[3] / 2 ** 20, 0.04 * mp * dp / 2 ** 20, ["%.4f" % x for x in worst]))
    ctx.close()


# ------------------------------------------------------------------ 12. full size
def test_full_size_c4_step(lib):
    """C4's shape: one full step on synthetic |N(0,1)| data and factors under a Bernoulli(0.1) mask on X, Y unweighted; 16 rows of
    each factor recomputed in float64 from what the device holds (data and weight blocks, the factors before the step; U and Z from
    the V the step produced)."""
    m = d = 65536
    p, k = 256, 256
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    ctx.fill_data_synthetic(0, 11)
    ctx.fill_data_synthetic(1, 12)
    ctx.fill_weight_synthetic(0, 13, 0.1)
    for w in range(3):
        ctx.fill_factor_synthetic(w, 20 + w)
    lay = ctx.mu_weighted_layout()
    mp, dp, _, _ = ctx.geometry()
    assert lay[3] < 0.01 * 4.0 * mp * dp, lay
    assert lay[2] > 1, lay                                   # Z: two row blocks for 256 CUs
    U0, V0, Z0 = (ctx.get_factor(w) for w in range(3))
    ctx.mu_weighted_step(0.0, 0.0, 7)
    U1, V1, Z1 = (ctx.get_factor(w) for w in range(3))
    rng = np.random.RandomState(0)
    E = WM.EPS
    worst = [0.0, 0.0, 0.0]
    density = []
    for c in rng.choice(d, 16, replace=False):
        x = ctx.get_data_block(0, 0, m, int(c), 1)[:, 0].astype(np.float64)
        wx = ctx.get_weight_block(0, 0, m, int(c), 1)[:, 0].astype(np.float64)
        y = ctx.get_data_block(1, int(c), 1, 0, p)[0].astype(np.float64)
        assert set(np.unique(wx)) <= {0.0, 1.0}
        density.append(wx.mean())
        num = (wx * x) @ U0 + y @ Z0
        den = (wx * (U0 @ V0[c])) @ U0 + (Z0 @ V0[c]) @ Z0
        ref = V0[c] * (num / np.where(den == 0, E, den))
        worst[1] = max(worst[1], _check(V1[c], ref, WM.tau(k, m + p), "V row %d" % c))
    assert 0.09 < np.mean(density) < 0.11, np.mean(density)
    for r in rng.choice(m, 16, replace=False):
        x = ctx.get_data_block(0, int(r), 1, 0, d)[0].astype(np.float64)
        wx = ctx.get_weight_block(0, int(r), 1, 0, d)[0].astype(np.float64)
        den = (wx * (V1 @ U0[r])) @ V1
        ref = U0[r] * (((wx * x) @ V1) / np.where(den == 0, E, den))
        worst[0] = max(worst[0], _check(U1[r], ref, WM.tau(k, d), "U row %d" % r))
    for r in rng.choice(p, 16, replace=False):
        y = ctx.get_data_block(1, 0, d, int(r), 1)[:, 0].astype(np.float64)
        den = (V1 @ Z0[r]) @ V1
        ref = Z0[r] * ((y @ V1) / np.where(den == 0, E, den))
        worst[2] = max(worst[2], _check(Z1[r], ref, WM.tau(k, d), "Z row %d" % r))
    print("C4 full step, 10 %% of X observed: shares %s, scratch %.1f MB, worst |err| / tau U %.4f V %.4f Z %.4f" % (lay[:3], lay[3] / 2 ** 20, *worst))
    ctx.close()
