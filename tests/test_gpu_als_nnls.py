"""The non-negative row solve of the ALS solver on the device (cmf_als_nnls_rows, cmf_als_nnls_step, CMF(als_nn_sweeps=n)) against
the float64 yardstick of als_yardstick.py on float32-rounded inputs.  Tolerance per factor (als_yardstick.tolerance, the HALS
rule): tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|) with y32 the float32 run of the same formulas.

Measured on an MI355X (worst |err| / tol of each group): see DESIGN section 16."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
from test_gpu_als import SHAPES, _case, _context, _f32
from test_gpu_wmu import fit_inputs

pytestmark = pytest.mark.gpu

NAMES = "UVZ"
L2 = 0.1


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _rows_context(lib, k):
    """A context that only carries k / k_pad: cmf_als_nnls_rows reads nothing else of the problem."""
    ctx = lib.Context(0)
    ctx.set_problem(8, 8, 8, k)
    return ctx, ctx.geometry()[3]


def _padded(H, g, F, kp):
    """The systems in cmf_als_normal's layout: k_pad x k_pad with 1 on the padding diagonal, zero padding of g and f."""
    n, k = g.shape
    Hp = np.zeros((n, kp, kp), dtype=np.float32)
    Hp[:, :k, :k] = H
    idx = np.arange(k, kp)
    Hp[:, idx, idx] = 1
    gp, fp = np.zeros((n, kp), dtype=np.float32), np.zeros((n, kp), dtype=np.float32)
    gp[:, :k], fp[:, :k] = g, F
    return Hp, gp, fp


# ------------------------------------------------------------------ 1. exact arithmetic
def _exact_systems(n, k, rng):
    """Diagonals 1, 2 or 4, six off-diagonal entries per row drawn from {4, 8} (multiples of every diagonal, so delta H[j, c] keeps
    the resolution of r), integer g in [-16, 64], a start in multiples of 1/4 in [0, 4].  Then f_j = max(0, g_j / H_jj - sum_c
    (H_jc / H_jj) f_c) stays in [0, 64] at a resolution of 1/16 and r at 1/4 below 2^13: every value of the recurrence, in any
    order of its sums, is a float32."""
    H = np.zeros((n, k, k))
    for i in range(n):
        for _ in range(3 * k):
            a, b = rng.randint(0, k, size=2)
            if a != b:
                H[i, a, b] = H[i, b, a] = rng.choice([4.0, 8.0])
        H[i, np.arange(k), np.arange(k)] = rng.choice([1.0, 2.0, 4.0], size=k)
    g = rng.randint(-16, 65, size=(n, k)).astype(np.float64)
    F = rng.randint(0, 17, size=(n, k)) / 4.0
    F[:, ::3] = 0
    return H, g, F


@pytest.mark.parametrize("k", [7, 40, 128, 256])
def test_exact_systems_are_swept_exactly(lib, k):
    rng = np.random.RandomState(100 + k)
    H, g, F = _exact_systems(5, k, rng)
    ctx, kp = _rows_context(lib, k)
    Hp, gp, fp = _padded(H, g, F, kp)
    for sweeps in (1, 3):
        ref = A.cd_rows(H, g, F, sweeps)
        assert np.abs(ref * 16 - np.round(ref * 16)).max() == 0 and (ref == 0).any() and (ref > 0).any() and (ref != F).any()
        got = ctx.als_nnls_rows(Hp, gp, fp, sweeps)
        assert (got[:, :k] == ref).all(), "k %d, %d sweeps: %d of %d coordinates differ" % (k, sweeps, int((got[:, :k] != ref).sum()), ref.size)
        assert (got[:, k:] == 0).all()
    ctx.close()


# ------------------------------------------------------------------ 2. random systems
def _random_systems(k):
    """70 systems of a U sweep: rows of X with k / 4 .. 2 k observed entries (fewer and more than k), non-unit weights, rounded to
    float32 (element by element: H stays symmetric)."""
    rng = np.random.RandomState(7 + k)
    m, d, p = 70, 3 * k + 50, 5
    dens = rng.uniform(0.25 * k / d, 2.0 * k / d, size=(m, 1))
    Wx = sp.csr_matrix(_f32(0.25 + 3.75 * rng.rand(m, d)) * (rng.rand(m, d) < dens))
    X, Y = _f32(rng.rand(m, d)), np.zeros((d, p))
    U, V, Z = (_f32(np.abs(rng.randn(n, k))) for n in (m, d, p))
    H, g = A.systems(A.Relation(X, Wx), A.Relation(Y, None), U, V, Z, "U", L2)
    lens = np.diff(Wx.indptr)
    assert lens.min() < k < lens.max()
    return _f32(H), _f32(g), U


@pytest.mark.parametrize("k", [7, 40, 128, 256])
def test_random_systems_against_the_yardstick(lib, k):
    H, g, F = _random_systems(k)
    ctx, kp = _rows_context(lib, k)
    Hp, gp, fp = _padded(H, g, F, kp)
    worst = 0.0
    for sweeps in (1, 4, 16):
        y64, y32 = A.cd_rows(H, g, F, sweeps), A.cd_rows(H, g, F, sweeps, dtype=np.float32)
        full = None
        for n in (70, 5, 1):
            got = ctx.als_nnls_rows(Hp[:n], gp[:n], fp[:n], sweeps)
            tol = A.tolerance(y32[:n], y64[:n], k)
            err = float(np.abs(got[:, :k] - y64[:n]).max())
            worst = max(worst, err / tol)
            print("k %d, %d sweeps, %d rows: |err| / tol %.3f (tol %.3e), %d of %d coordinates clipped"
                  % (k, sweeps, n, err / tol, tol, int((y64[:n] == 0).sum()), y64[:n].size))
            assert np.isfinite(got).all() and err <= tol
            assert (got >= 0).all() and (got[:, k:] == 0).all()
            assert ctx.als_nnls_rows(Hp[:n], gp[:n], fp[:n], sweeps).tobytes() == got.tobytes()      # a repeated call
            if n == 70:
                full = got
            else:
                assert got.tobytes() == full[:n].tobytes()                                          # the batch does not matter
        for i in (37, 69):                                                                           # a row solved alone
            assert ctx.als_nnls_rows(Hp[i:i + 1], gp[i:i + 1], fp[i:i + 1], sweeps).tobytes() == full[i:i + 1].tobytes()
    print("k %d: worst |err| / tol %.3f" % (k, worst))
    ctx.close()


# ------------------------------------------------------------------ 3. full steps
_refs = {}


def _start(shape, yform, nn):
    """test_gpu_als's signed case, with |F| for the factors in nn: a non-negative factor starts as one."""
    X, Y, Wx, Wy, F, _ = _case(shape, yform)
    return X, Y, Wx, Wy, [np.abs(F[w]) if nn & (1 << w) else F[w] for w in range(3)]


def _reference(shape, yform, mask, nn, sweeps):
    key = (shape, yform, mask, nn, sweeps)
    if key not in _refs:
        X, Y, Wx, Wy, F = _start(shape, yform, nn)
        Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
        _refs[key] = tuple(A.step(Rx, Ry, None, None, *F, L2, mask=mask, nn_mask=nn, nn_sweeps=sweeps, dtype=dt) for dt in (np.float64, np.float32)) + (
            [A.no_information(Rx, Ry, *F, w) for w in NAMES],)
    return _refs[key]


def _step_case(lib, shape, yform, mask, nn, sweeps):
    k = shape[3]
    X, Y, Wx, Wy, F = _start(shape, yform, nn)
    y64, y32, empty = _reference(shape, yform, mask, nn, sweeps)
    ctx = _context(lib, X, Y, F, Wx, Wy, native_y=(yform == "csr"))
    ctx.newton_clamp_stats(reset=True)
    before = [ctx.get_factor(w).tobytes() for w in range(3)]
    ctx.als_nnls_step(L2, nn, mask, sweeps)
    got = [ctx.get_factor(w) for w in range(3)]
    report = []
    for w in range(3):
        if not mask & (1 << w):
            assert got[w].tobytes() == before[w], "factor %s was not swept and changed" % NAMES[w]
            continue
        tol = A.tolerance(y32[w], y64[w], k)
        err = float(np.abs(got[w] - y64[w]).max())
        report.append("%s %.3f" % (NAMES[w], err / tol))
        assert np.isfinite(got[w]).all() and err <= tol, "%s: |err| / tol = %.3f (tol %.3e)" % (NAMES[w], err / tol, tol)
        assert (got[w][empty[w]] == 0).all() and (y64[w][empty[w]] == 0).all(), "%s: rows without information must be exact zeros" % NAMES[w]
        if nn & (1 << w):
            assert (got[w] >= 0).all()
    if mask & 1:
        assert empty[0][shape[0] // 3]                               # the unobserved row of X is such a row of U
    assert ctx.newton_clamp_stats()[0] == 0
    print("%s Y %s mask %d nn %d sweeps %d: |err| / tol %s" % (shape, yform, mask, nn, sweeps, " ".join(report)))
    ctx.close()


@pytest.mark.parametrize("yform", ["dense", "csr", "observed"])
@pytest.mark.parametrize("shape", SHAPES)
def test_full_step_all_non_negative(lib, shape, yform):
    _step_case(lib, shape, yform, 7, 7, 4)


@pytest.mark.parametrize("shape, yform", list(zip(SHAPES, ["observed", "dense", "csr", "observed"])))
def test_full_step_with_a_signed_v(lib, shape, yform):
    """nn_mask = 5: V goes through the Cholesky solves, U and Z through coordinate descent, in one step."""
    _step_case(lib, shape, yform, 7, 5, 1)


@pytest.mark.parametrize("sweeps", [1, 4])
@pytest.mark.parametrize("mask, nn", [(7, 7), (1, 7), (2, 7), (4, 7), (1, 5), (2, 5), (4, 5)])
@pytest.mark.parametrize("shape, yform", [((257, 1031, 77, 7), "observed"), ((70, 333, 129, 40), "dense")])
def test_masks_and_sweep_counts(lib, shape, yform, mask, nn, sweeps):
    _step_case(lib, shape, yform, mask, nn, sweeps)


# ------------------------------------------------------------------ 4. unchanged paths
def test_without_non_negative_factors_the_step_is_the_als_step(lib):
    shape = (70, 333, 129, 40)
    X, Y, Wx, Wy, F, _ = _case(shape, "observed")
    runs = []
    for nnls in (False, True):
        ctx = _context(lib, X, Y, F, Wx, Wy)
        for mask in (7, 2):
            if nnls:
                ctx.als_nnls_step(L2, 0, mask, 4)
            else:
                ctx.als_step(L2, 0, mask)
        runs.append([ctx.get_factor(w).tobytes() for w in range(3)])
        ctx.close()
    assert runs[0] == runs[1]


def test_other_solvers_are_untouched_by_nnls_steps(lib):
    """Context b runs nnls steps in between (per-row route with CSR weights bound, then the shared route without), its factors
    reset afterwards; context a never hears of them.  cmf_mu_step, cmf_newton_step (per-row Hessians: a logit link) and
    cmf_hals_step agree byte for byte, and so do the clamp statistics of the Newton steps."""
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
        b.als_nnls_step(0.1, 7, 7, 4)
        b.als_nnls_step(0.1, 5, 7, 1)
        b.clear_weight(0)
        reset(a)
        reset(b)
        step(a)
        step(b)
        assert factors(a) == factors(b)
    assert a.newton_clamp_stats(full=True) == b.newton_clamp_stats(full=True)
    assert a.newton_clamp_routes() == b.newton_clamp_routes()
    b.als_nnls_step(0.1, 7, 7, 2)                            # no weights bound: the shared route (HALS sweeps)
    assert all((b.get_factor(w) >= 0).all() for w in range(3))
    reset(a)
    reset(b)
    a.hals_step(0.01, 0.02, 7)
    b.hals_step(0.01, 0.02, 7)
    assert factors(a) == factors(b)
    a.close()
    b.close()


def test_unweighted_non_negative_step_is_repeated_hals_sweeps(lib):
    """No observed side: the factors in nn_mask take `sweeps` HALS sweeps on the one Gram -- the yardstick's step within its tolerance."""
    m, d, p, k = 257, 1031, 77, 7
    rng = np.random.RandomState(2)
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    F = [_f32(np.abs(rng.randn(n, k))) for n in (m, d, p)]
    ctx = _context(lib, X, Y, F, None, None)
    ctx.als_nnls_step(L2, 7, 7, 3)
    y64, y32 = (A.step(X, Y, None, None, *F, L2, nn_mask=7, nn_sweeps=3, dtype=dt) for dt in (np.float64, np.float32))
    for w in range(3):
        got = ctx.get_factor(w)
        assert (got >= 0).all() and np.abs(got - y64[w]).max() <= A.tolerance(y32[w], y64[w], k)
    ctx.close()


# ------------------------------------------------------------------ 5. refusals
def test_refusals(lib):
    m, d, p, k = 40, 50, 30, 6
    rng = np.random.RandomState(2)
    ctx = lib.Context(0)
    with pytest.raises(ValueError):                              # no problem bound
        lib.check(ctx._lib.cmf_als_nnls_rows(ctx._h, 0, None, None, None, 1))
    ctx.set_problem(40, 50, 30, 300)
    kp = ctx.geometry()[3]
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.als_nnls_step(0.1, 7, 7, 4)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.als_nnls_rows(np.eye(kp)[None], np.zeros((1, kp)), np.zeros((1, kp)), 1)
    ctx.set_problem(m, d, p, k)
    kp = ctx.geometry()[3]
    F = [_f32(np.abs(rng.randn(n, k))) for n in (m, d, p)]
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.set_data(0, _f32(rng.randn(m, d)))
    ctx.set_data(1, _f32(rng.randn(d, p)))
    for sweeps in (0, -1, 1025):
        with pytest.raises(ValueError, match="sweeps must be 1 .. 1024"):
            ctx.als_nnls_step(0.1, 7, 7, sweeps)
        with pytest.raises(ValueError, match="sweeps must be 1 .. 1024"):
            ctx.als_nnls_rows(np.eye(kp)[None], np.zeros((1, kp)), np.zeros((1, kp)), sweeps)
    with pytest.raises(ValueError, match="l2 must be positive"):
        ctx.als_nnls_step(0.0, 7, 7, 4)
    for mask in (0, 8):
        with pytest.raises(ValueError, match="update_mask"):
            ctx.als_nnls_step(0.1, 7, mask, 4)
    with pytest.raises(ValueError, match="null pointer"):
        lib.check(ctx._lib.cmf_als_nnls_rows(ctx._h, 1, None, None, None, 1))
    ctx.als_nnls_step(0.1, 7, 7, 1024)                           # the largest count: rows stop when a sweep moves nothing
    assert all(np.isfinite(ctx.get_factor(w)).all() and (ctx.get_factor(w) >= 0).all() for w in range(3))
    ctx.close()


# ------------------------------------------------------------------ 6. fit through CMF
def test_fit_matches_the_float64_yardstick_and_beats_mu(lib):
    from pycmf_amd import CMF
    X, Y, Wx, _, U, V, Z = fit_inputs(3, m=120, d=150, p=20, k=3, obs=.3)
    l2, iters = 0.05, 10
    Xi, Wref = sp.csr_matrix(X * Wx), sp.csr_matrix(Wx)
    assert Xi.nnz == Wref.nnz
    kw = dict(n_components=3, l2_reg=l2, tol=0, x_init="custom", y_init="custom")
    model = CMF(solver="als", als_nn_sweeps=4, max_iter=iters, **kw)
    Ug, Vg, Zg = model.fit_transform(Xi, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights="observed")
    Ur, Vr, Zr = A.fit(X, Y, Wref, None, U, V, Z, iters, l2, nn_mask=7, nn_sweeps=4)[:3]
    ref = sum(A.errors(X, Y, Wref, None, Ur, Vr, Zr))
    print("fit: reconstruction_err_ %.9g, yardstick %.9g, relative %.2e" % (model.reconstruction_err_, ref, abs(model.reconstruction_err_ - ref) / ref))
    assert model.n_iter_ == iters and abs(model.reconstruction_err_ - ref) <= 1e-4 * ref
    assert min(Ug.min(), Vg.min(), Zg.min()) >= 0
    unobserved = Wx == 0
    mu = CMF(solver="mu", max_iter=300, **kw)
    Um, Vm, _ = mu.fit_transform(Xi, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights="observed")
    rmse = [float(np.sqrt((((X - P @ Q.T) ** 2)[unobserved]).mean())) for P, Q in ((Ug, Vg), (Um, Vm))]
    print("RMSE on the unobserved cells: ALS, 4 sweeps, after %d iterations %.4f, weighted MU after 300 %.4f" % (iters, rmse[0], rmse[1]))
    assert rmse[0] < rmse[1]
    # transform carries the keyword: V and Z fixed, U re-fitted non-negative on the observed entries of new rows
    U2, V2, Z2 = model.transform(Xi[:50], None, x_entry_weights="observed")
    assert V2.tobytes() == model.components.tobytes() and Z2.tobytes() == model.y_weights.tobytes()
    assert U2.shape == (50, 3) and np.isfinite(U2).all() and U2.min() >= 0
