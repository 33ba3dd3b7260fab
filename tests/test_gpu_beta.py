"""Beta-divergence multiplicative updates on the device (cmf_mu_beta_products, cmf_mu_beta_step, cmf_beta_divergence,
CMF(loss='beta-divergence')) against the float64 yardstick of beta_yardstick.py on float32-rounded inputs.  The tolerances are
derived there; EVERY element of every product and every updated factor is compared: exactly 0 where the yardstick is exactly 0,
within the bound relative elsewhere.

Worst |err| / bound observed on an MI355X over this file: products 0.042, sweeps and full steps 0.029, divergence 0.0055, fits
0.0003."""
import numpy as np
import pytest
import scipy.sparse as sp

import beta_yardstick as BY
from test_gpu_kl import _problem, _check, _context

pytestmark = pytest.mark.gpu

U_, V_, Z_ = 0, 1, 2
BETAS = [0.0, 0.5, 1.5]
SHAPES = [(257, 1031, 77, 7), (70, 333, 129, 40), (128, 3000, 150, 128), (300, 5000, 130, 256), (100, 20000, 60, 16)]


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


_cache = {}


def _beta_problem(m, d, p, k, beta):
    """test_gpu_kl's dense problem (values in [1e-3, 1e3], zeros in the data, an empty row and column, a zero factor row); for
    beta = 0 the same with every zero of the data replaced by a positive value.  Built once per (shape, beta = 0 or not)."""
    key = (m, d, p, k, beta == 0)
    if key not in _cache:
        X, Y, F = _problem(m, d, p, k, False, seed=k + m)
        if beta == 0:
            X, Y = X.copy(), Y.copy()
            X[X == 0] = 0.5
            Y[Y == 0] = 0.25
        for A in (X, Y) + tuple(F):
            A.setflags(write=False)
        _cache[key] = (X, Y, F)
    return _cache[key]


def _sweep_bounds(X, Y, F, beta, sweep, l1, l2, k, t_v=0.0):
    """(bound of the sweep's products, bound of its updated elements) from the yardstick's own S and quotients."""
    m, d, p = F[0].shape[0], F[1].shape[0], F[2].shape[0]
    if sweep == 0:
        L, lmax = d, BY.lmax_of(F[0], F[1])
    elif sweep == 2:
        L, lmax = d, BY.lmax_of(F[2], F[1])
    else:
        L, lmax = m + p, max(BY.lmax_of(F[1], F[0]), BY.lmax_of(F[1], F[2]))
    tn = BY.tau_products(k, L, beta, lmax)
    num, den = BY.sweep_products(X, Y, F[0], F[1], F[2], beta, sweep)
    q = BY.quotient(num, den, F[sweep], l1, l2)
    lq = float(np.abs(np.log2(q[q > 0])).max()) if (q > 0).any() else 0.0
    return tn, BY.tau_step(tn, beta, lq, t_v)


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("m, d, p, k", SHAPES)
def test_each_product_alone(lib, m, d, p, k, beta):
    X, Y, F = _beta_problem(m, d, p, k, beta)
    ctx = _context(lib, X, Y, F)
    lay = ctx.mu_beta_layout()
    if (m, d) == (100, 20000):
        assert lay[0] > 1 and lay[2] > 1, lay           # few output rows, long stream: the stream is cut into shares
    kp = ctx.geometry()[3]
    for sweep, name in ((1, "V"), (0, "U"), (2, "Z")):
        num, den = ctx.mu_beta_products(beta, sweep)
        assert num.shape == den.shape == (F[sweep].shape[0], kp)
        assert not num[:, k:].any() and not den[:, k:].any()          # the padded columns: exact zeros
        rn, rd = BY.sweep_products(X, Y, F[0], F[1], F[2], beta, sweep)
        tn, _ = _sweep_bounds(X, Y, F, beta, sweep, 0.0, 0.0, k)
        wn = _check(num[:, :k].astype(np.float64), rn, tn, "num of the %s sweep" % name)
        wd = _check(den[:, :k].astype(np.float64), rd, tn, "den of the %s sweep" % name)
        print("(%d, %d, %d, k=%d) beta=%g %s products: shares %s, worst |err| / tau = num %.4f den %.4f" % (m, d, p, k, beta, name, lay[:3], wn, wd))
    assert [ctx.get_factor(w).tobytes() for w in range(3)] == [np.asarray(F[w]).tobytes() for w in range(3)]    # nothing was updated
    ctx.close()


@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("m, d, p, k", SHAPES)
def test_single_sweeps_and_the_full_step(lib, m, d, p, k, beta, l1, l2):
    X, Y, F = _beta_problem(m, d, p, k, beta)
    ctx = _context(lib, X, Y, F)
    for mask, name in ((BY.V_BIT, "V"), (BY.U_BIT, "U"), (BY.Z_BIT, "Z"), (7, "full")):
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.mu_beta_step(beta, l1, l2, mask)
        got = [ctx.get_factor(w) for w in range(3)]
        ref = BY.step(X, Y, F[0], F[1], F[2], beta, l1, l2, mask)
        tV = _sweep_bounds(X, Y, F, beta, 1, l1, l2, k)[1]
        after_v = [F[0], ref[1], F[2]] if mask == 7 else F          # U and Z of a full step read the new V
        carry = tV if mask == 7 else 0.0
        tols = (_sweep_bounds(X, Y, after_v, beta, 0, l1, l2, k, carry)[1], tV, _sweep_bounds(X, Y, after_v, beta, 2, l1, l2, k, carry)[1])
        worst = []
        for w, bit in ((U_, BY.U_BIT), (V_, BY.V_BIT), (Z_, BY.Z_BIT)):
            if mask & bit:
                worst.append(_check(got[w], ref[w], tols[w], "%s sweep, factor %d" % (name, w)))
            else:
                assert got[w].tobytes() == np.asarray(F[w]).tobytes()
        print("(%d, %d, %d, k=%d) beta=%g l1=%g l2=%g %s: worst |err| / tau = %s" % (m, d, p, k, beta, l1, l2, name, ["%.4f" % x for x in worst]))
    ctx.close()


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("m, d, p, k", SHAPES)
def test_divergence(lib, m, d, p, k, beta):
    X, Y, F = _beta_problem(m, d, p, k, beta)
    ctx = _context(lib, X, Y, F)
    dx, dy = ctx.beta_divergence(beta)
    for name, got, (T, A, B) in (("x", dx, (X, F[0], F[1])), ("y", dy, (Y, F[1], F[2]))):
        ref, sum_abs = BY.divergence_terms(T, A, B, beta)
        lmax = max(BY.lmax_of(A, B), float(np.abs(np.log2(T[T > 0])).max()))
        tol = BY.div_tol(k, beta, lmax, sum_abs)
        print("(%d, %d, %d, k=%d) beta=%g D_%s: |err| / tol = %.4f" % (m, d, p, k, beta, name, abs(got - ref) / tol))
        assert abs(got - ref) <= tol
    assert ctx.beta_divergence(beta, True, False)[0] == dx and ctx.beta_divergence(beta, False, True) == (0.0, dy)
    ctx.close()


@pytest.mark.parametrize("k", [7, 100, 200])
@pytest.mark.parametrize("dense_owner", ["V", "UZ"])
def test_exact_arithmetic_at_beta_zero_pins_both_column_maps(lib, k, dense_owner):
    """The construction of test_gpu_kl's exact test with strictly positive data: every product A_r . B_c is a power of two and T is
    that product times a power of two, so r, p = r r, n = t p, d = s p and every sum are exact in float32 whatever the order: num
    and den are determined bit for bit.  The factors are asymmetric, so a slip in the second accumulator's column map, in the
    transposed access or in the k pairing changes them.  (The step is not held to the bit: the square root is not exact.)"""
    m, d, p = 70, 333, 40
    rng = np.random.RandomState(k)

    def dense(r):
        return 2.0 ** rng.randint(0, 4, size=(r, k))

    def onehot(r):
        F = np.zeros((r, k))
        F[np.arange(r), rng.randint(0, k, size=r)] = 2.0 ** rng.randint(0, 3, size=r)
        return F
    F = [onehot(m), dense(d), onehot(p)] if dense_owner == "V" else [dense(m), onehot(d), dense(p)]
    X = (F[0] @ F[1].T) * 2.0 ** rng.randint(-2, 3, size=(m, d))
    Y = (F[1] @ F[2].T) * 2.0 ** rng.randint(-2, 3, size=(d, p))
    assert (X > 0).all() and (Y > 0).all()
    ctx = _context(lib, X, Y, F)
    for sweep in (0, 1, 2):
        num, den = ctx.mu_beta_products(0.0, sweep)
        rn, rd = BY.sweep_products(X, Y, F[0], F[1], F[2], 0.0, sweep)
        assert (rn == rn.astype(np.float32)).all() and (rd == rd.astype(np.float32)).all()     # the yardstick's values are float32 numbers
        assert (num[:, :k] == rn).all(), "num of sweep %d" % sweep
        assert (den[:, :k] == rd).all(), "den of sweep %d" % sweep
    ctx.close()


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("split", [1, 0, 3])
def test_a_repeated_step_is_bit_identical(lib, beta, split):
    m, d, p, k = 300, 2100, 130, 40
    X, Y, F = _beta_problem(m, d, p, k, beta)
    ctx = _context(lib, X, Y, F, split=split)
    lay = ctx.mu_beta_layout()
    assert (lay[0] == 1) == (split == 1) and (split != 3 or lay[0] == 3), lay
    mp, dp, pp, kp = ctx.geometry()
    kl_small = (2 * ((max(mp + pp, dp) + 511) // 512) + 4) * kp * 8 + 64          # the KL step's column sums, which this step has none of
    assert lay[:3] == ctx.mu_kl_layout()[:3] and lay[3] - 64 == 2 * (ctx.mu_kl_layout()[3] - kl_small), lay   # twice the KL step's slabs
    runs = []
    for _ in range(2):
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.mu_beta_step(beta, 0.01, 0.02, 7)
        ctx.mu_beta_step(beta, 0.01, 0.02, 7)
        runs.append([ctx.get_factor(w).tobytes() for w in range(3)] + [np.array(ctx.beta_divergence(beta)).tobytes()]
                    + [a.tobytes() for a in ctx.mu_beta_products(beta, 1)])
    assert runs[0] == runs[1]
    ctx.close()


def _fit_bound(X, Y, U, V, Z, beta, k, n_iter):
    F = [U, V, Z]
    tV = _sweep_bounds(X, Y, F, beta, 1, 0.0, 0.0, k)[1]
    t_full = max(_sweep_bounds(X, Y, F, beta, s, 0.0, 0.0, k, tV)[1] for s in (0, 2))
    return BY.fit_rtol(n_iter, t_full)


@pytest.mark.parametrize("beta_loss", ["itakura-saito", 0.5, 1.5])
def test_fit_matches_the_float64_yardstick(lib, beta_loss):
    from pycmf_amd import CMF
    beta = 0.0 if beta_loss == "itakura-saito" else beta_loss
    X, Y, U, V, Z = BY.fit_problem(BY.FIT_SEEDS[beta])
    Ur, Vr, Zr, n_ref, ratios = BY.fit(X, Y, U, V, Z, beta, 200, BY.FIT_TOL)
    model = CMF(n_components=6, solver="mu", loss="beta-divergence", beta_loss=beta_loss, max_iter=200, tol=BY.FIT_TOL, x_init="custom", y_init="custom")
    Ug, Vg, Zg = model.fit_transform(X, Y, U=U.copy(), V=V.copy(), Z=Z.copy())
    assert model.n_iter_ == n_ref          # (test_beta_host.py: every check of the yardstick lies >= 10 % away from tol)
    rtol = _fit_bound(X, Y, U, V, Z, beta, 6, n_ref)
    worst = max(np.abs(G - R).max() / (rtol * np.abs(R).max()) for G, R in ((Ug, Ur), (Vg, Vr), (Zg, Zr)))
    ref = sum(BY.errors(X, Y, Ur, Vr, Zr, beta))
    print("fit beta=%g: %d iterations, accumulated bound %.2e, worst |err| / bound %.4f, reconstruction_err_ %.9g (yardstick %.9g)"
          % (beta, n_ref, rtol, worst, model.reconstruction_err_, ref))
    for G in (Ug, Vg, Zg):
        assert np.isfinite(G).all() and (G >= 0).all()
    assert worst <= 1.0
    assert abs(model.reconstruction_err_ - ref) <= rtol * ref


@pytest.mark.parametrize("beta_loss, loss", [(1, "kullback-leibler"), ("kullback-leibler", "kullback-leibler"), (2, "frobenius"), ("frobenius", "frobenius")])
def test_beta_one_and_two_give_the_kl_and_frobenius_factors_bit_for_bit(lib, beta_loss, loss):
    from pycmf_amd import CMF
    X, Y, U, V, Z = BY.fit_problem(3)
    got = []
    for kw in (dict(loss="beta-divergence", beta_loss=beta_loss), dict(loss=loss)):
        model = CMF(n_components=6, solver="mu", max_iter=20, tol=1e-9, x_init="custom", y_init="custom", **kw)
        got.append([np.asarray(A).tobytes() for A in model.fit_transform(X, Y, U=U.copy(), V=V.copy(), Z=Z.copy())] + [model.n_iter_, model.reconstruction_err_])
    assert got[0] == got[1]


def test_other_steps_are_untouched_by_a_beta_step(lib):
    m, d, p, k = 200, 300, 90, 12
    X, Y, F = _problem(m, d, p, k, False, seed=41)
    a, b = _context(lib, X, Y, F), _context(lib, X, Y, F)
    for ctx in (a, b):
        ctx.set_option("graph", 1)
    for ctx in (a, b):                   # the Frobenius step graph is captured, the KL scratch allocated
        for _ in range(3):
            ctx.mu_step(0.0, 0.0, 7)
        ctx.mu_kl_step(0.0, 0.0, 7)
        for w in range(3):
            ctx.set_factor(w, F[w])
    b.mu_beta_step(0.5, 0.0, 0.0, 7)     # b: beta work in between
    b.mu_beta_step(0.0, 0.01, 0.0, 7)
    b.beta_divergence(1.5)
    b.mu_beta_products(0.5, 1)
    for w in range(3):
        b.set_factor(w, F[w])
    for ctx in (a, b):
        for _ in range(3):
            ctx.mu_step(0.0, 0.0, 7)
        ctx.mu_kl_step(0.01, 0.02, 7)
    assert [b.get_factor(w).tobytes() for w in range(3)] == [a.get_factor(w).tobytes() for w in range(3)]
    assert b.residual_sq() == a.residual_sq() and b.kl_divergence() == a.kl_divergence()
    a.close()
    b.close()


def test_refusals_leave_the_context_usable(lib):
    ctx = lib.Context(0)
    ctx.set_problem(40, 50, 30, 300)
    for call in (lambda: ctx.mu_beta_step(0.5, 0.0, 0.0, 7), lambda: ctx.beta_divergence(0.5), lambda: ctx.mu_beta_products(0.5, 0), ctx.mu_beta_layout):
        with pytest.raises(NotImplementedError, match="k_pad"):
            call()
    X, Y, F = _problem(40, 50, 30, 6, False, seed=2)
    ctx.set_problem(40, 50, 30, 6)
    for w in range(3):
        ctx.set_factor(w, F[w])
    for beta in (-0.5, 2.5, float("nan")):
        with pytest.raises(ValueError, match=r"beta must lie in \[0, 2\]"):
            ctx.mu_beta_step(beta, 0.0, 0.0, 7)
        with pytest.raises(ValueError, match=r"beta must lie in \[0, 2\]"):
            ctx.beta_divergence(beta)
    with pytest.raises(ValueError, match="X has not been set"):
        ctx.mu_beta_step(0.5, 0.0, 0.0, 7)
    with pytest.raises(ValueError, match="X has not been set"):
        ctx.beta_divergence(0.5)
    ctx.set_data(0, X)
    with pytest.raises(ValueError, match="Y has not been set"):
        ctx.mu_beta_step(0.5, 0.0, 0.0, BY.Z_BIT)
    with pytest.raises(ValueError, match="Y has not been set"):
        ctx.mu_beta_products(0.5, 1)
    with pytest.raises(ValueError, match="sweep must be"):
        ctx.mu_beta_products(0.5, 3)
    ctx.mu_beta_step(0.5, 0.0, 0.0, BY.U_BIT)                    # the X side alone serves a U sweep
    tol = _sweep_bounds(X, Y, F, 0.5, 0, 0.0, 0.0, 6)[1]
    _check(ctx.get_factor(U_), BY.step(X, Y, *F, 0.5, mask=BY.U_BIT)[0], tol, "U sweep without Y")
    ctx.set_data(1, Y)
    # weights, a background weight and biases on a relation the call reads
    P = sp.csr_matrix((X > 0).astype(float))
    P.sort_indices()
    ctx.set_weight(0, np.ones_like(X))
    with pytest.raises(NotImplementedError, match="X has entry weights bound"):
        ctx.mu_beta_step(0.5, 0.0, 0.0, 7)
    ctx.mu_beta_step(0.5, 0.0, 0.0, BY.Z_BIT)                    # a sweep that does not read X goes through
    ctx.set_weighted_csr(0, P.indptr, P.indices, np.asarray(X[P.nonzero()]).ravel(), 2.0 * np.ones(P.nnz))
    ctx.set_background_weight(0, 1.0)
    with pytest.raises(NotImplementedError, match="X has a background weight bound"):
        ctx.mu_beta_step(0.5, 0.0, 0.0, 7)
    ctx.set_background_weight(0, 0.0)
    ctx.set_biases(0, True, 0.5, 0.1)
    with pytest.raises(NotImplementedError, match="X has biases bound"):
        ctx.beta_divergence(0.5)
    ctx.clear_weight(0)
    # a relation held only as native CSR
    ctx.set_option("sparse_mode", 2)
    ctx.set_data(1, sp.csr_matrix(Y))
    assert ctx.data_layout(1) == (False, True)
    with pytest.raises(NotImplementedError, match="sparse_mode 1"):
        ctx.mu_beta_step(0.5, 0.0, 0.0, 7)
    with pytest.raises(NotImplementedError, match="sparse_mode 1"):
        ctx.mu_beta_products(0.5, 2)
    ctx.set_option("sparse_mode", 0)
    ctx.set_data(1, Y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.mu_beta_step(0.5, 0.0, 0.0, 7)
    tol = _sweep_bounds(X, Y, F, 0.5, 1, 0.0, 0.0, 6)[1]
    _check(ctx.get_factor(V_), BY.step(X, Y, *F, 0.5)[1], tol, "V after the refusals")
    ctx.close()
