"""Host side of the beta-divergence loss (no GPU): the float64 yardstick of the GPU tests against sklearn's own multiplicative
update and divergence at beta = 0, 0.5 and 1.5, its monotone decrease, the seeds of the GPU fit test, and the argument validation
of ``loss='beta-divergence'`` / ``beta_loss`` -- which must raise before any device is touched."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import beta_yardstick as BY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = [0.0, 0.5, 1.5]


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


# ------------------------------------------------------------------ yardstick against sklearn
@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.3, 0.0), (0.0, 0.2), (0.1, 0.4)])
@pytest.mark.parametrize("beta", BETAS)
def test_yardstick_is_sklearns_update_and_divergence(beta, l1, l2):
    try:
        from sklearn.decomposition._nmf import _multiplicative_update_w, _multiplicative_update_h, _beta_divergence
    except ImportError:                                     # private names: only their absence may skip
        pytest.skip("this sklearn has no _multiplicative_update_w / _h")
    rng = np.random.RandomState(5)
    n, f, k = 23, 17, 4
    W, H = np.abs(rng.randn(n, k)) + 0.1, np.abs(rng.randn(k, f)) + 0.1       # positive factors: S >= EPS everywhere
    X = np.abs(rng.randn(n, f)) + 0.05
    if beta > 0:
        X[3] = 0
        X[:, 5] = 0
    g = BY.gamma_of(beta)
    # single matrix X ~ W H as the U side of the collective model: X = U V^T with U = W, V = H^T, nothing on the Y side
    Y0, Z0 = np.zeros((f, 1)), np.zeros((1, k))
    # (sklearn >= 1.4 returns the updated factor, which it changed in place; earlier versions return the ratio)
    Wc = W.copy()
    ret = _multiplicative_update_w(X, Wc, H.copy(), beta_loss=beta, l1_reg_W=l1, l2_reg_W=l2, gamma=g)[0]
    U1, _, _ = BY.step(X, Y0, W, H.T, Z0, beta, l1, l2, mask=BY.U_BIT)
    assert _rel(U1, ret if ret is Wc else W * ret) <= 1e-12
    Hc = H.copy()
    ret = _multiplicative_update_h(X, W.copy(), Hc, beta_loss=beta, l1_reg_H=l1, l2_reg_H=l2, gamma=g)
    _, V1, _ = BY.step(X, Y0, W, H.T, Z0, beta, l1, l2, mask=BY.V_BIT)   # Z = 0: the y part of V's products vanishes
    assert _rel(V1, (ret if ret is Hc else H * ret).T) <= 1e-12
    ref = _beta_divergence(X, W, H, beta, square_root=False)
    assert abs(BY.divergence(X, W, H.T, beta) - ref) <= 1e-12 * abs(ref)
    ref = _beta_divergence(X, W, H, beta, square_root=True)
    assert abs(BY.errors(X, Y0, W, H.T, Z0, beta)[0] - ref) <= 1e-12 * abs(ref)


def test_beta_one_and_two_are_the_kl_and_frobenius_formulas():
    import kl_yardstick as KL
    rng = np.random.RandomState(2)
    X, Y = rng.poisson(1.0, (20, 30)).astype(float), rng.poisson(1.0, (30, 9)).astype(float)
    U, V, Z = (np.abs(rng.randn(n, 4)) + 0.1 for n in (20, 30, 9))
    for Fa, Fb in zip(BY.step(X, Y, U, V, Z, 1.0, 0.1, 0.2), KL.step(X, Y, U, V, Z, 0.1, 0.2)):
        assert _rel(Fa, Fb) <= 1e-12
    assert abs(BY.divergence(X, U, V, 1.0) - KL.divergence(X, U, V)) <= 1e-12 * KL.divergence(X, U, V)
    assert abs(BY.divergence(X, U, V, 2.0) - 0.5 * ((X - U @ V.T) ** 2).sum()) <= 1e-12 * BY.divergence(X, U, V, 2.0)
    num, den = BY.pair(X, U, V, 2.0)
    assert _rel(num, X @ V) <= 1e-13 and _rel(den, U @ (V.T @ V)) <= 1e-12


def _problem(seed, m=40, d=60, p=30, k=5, zeros=False):
    rng = np.random.RandomState(seed)
    X, Y = np.abs(rng.randn(m, d)) + 0.01, np.abs(rng.randn(d, p)) + 0.01
    if zeros:
        X[2] = 0
        X[:, 7] = 0
        Y[rng.rand(d, p) < 0.2] = 0
    U, V, Z = (np.abs(rng.randn(n, k)) + 0.1 for n in (m, d, p))
    return X, Y, U, V, Z


@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("beta", BETAS)
def test_collective_objective_never_rises_over_60_iterations(beta, l1, l2):
    X, Y, U, V, Z = _problem(11, zeros=beta > 0)
    prev = BY.objective(X, Y, U, V, Z, beta, l1, l2)
    for _ in range(60):
        U, V, Z = BY.step(X, Y, U, V, Z, beta, l1, l2)
        cur = BY.objective(X, Y, U, V, Z, beta, l1, l2)
        assert np.isfinite(cur) and cur <= prev * (1 + 1e-13)
        prev = cur
    assert all(np.isfinite(F).all() and (F >= 0).all() for F in (U, V, Z))
    if beta > 0:
        assert (U[2] == 0).all()          # the all-zero row of X: its factor row goes to exactly 0 in the first sweep


def test_corner_cases_by_hand():
    E = BY.EPS
    # a zero owned row: s = 0, p = EPS^(beta - 2) finite, den = 0 * p = 0 exactly, num = t * p
    num, den = BY.pair(np.array([[3.0]]), np.zeros((1, 1)), np.ones((1, 1)), 0.0)
    assert den[0, 0] == 0.0 and num[0, 0] == 3.0 * E ** -2.0
    # t = 0: an exact zero in the numerator
    assert BY.pair(np.array([[0.0]]), np.ones((1, 1)), np.ones((1, 1)), 0.5)[0][0, 0] == 0.0
    # Itakura-Saito by hand: t = 2, s = 1 -> 2 - log 2 - 1
    assert BY.divergence(np.array([[2.0]]), np.ones((1, 1)), np.ones((1, 1)), 0.0) == 2.0 - np.log(2.0) - 1.0
    assert BY.divergence(np.array([[0.0]]), np.ones((1, 1)), np.ones((1, 1)), 0.0) == np.inf
    # t = 0 at beta = 0.5: s^beta / beta
    assert BY.divergence(np.array([[0.0]]), np.array([[4.0]]), np.ones((1, 1)), 0.5) == 2.0 / 0.5
    assert BY.gamma_of(0.0) == 0.5 and BY.gamma_of(0.5) == 1 / 1.5 and BY.gamma_of(1.0) == BY.gamma_of(1.5) == BY.gamma_of(2.0) == 1.0
    assert (BY.reg(np.zeros((3, 2)), np.zeros((3, 2)), 0.0, 0.0) == E).all()


def test_tolerance_functions():
    u = 2.0 ** -24
    assert BY.pow_err(-1.5, 20.0) == (3 * 1.5 * 20 + 2) * u
    assert BY.tau_products(7, 100, 0.0, 30.0) == (7 * 3 + 100 + 9) * u + 5 * u
    assert BY.tau_products(7, 100, 0.5, 30.0) == (7 * 2.5 + 100 + 9) * u + BY.pow_err(-1.5, 30.0)
    assert BY.tau_step(1e-5, 1.5, 9.0) == 2e-5 + 3 * u + u
    assert BY.tau_step(1e-5, 0.0, 9.0) == 0.5 * (2e-5 + 3 * u) + 2 * u + u


@pytest.mark.parametrize("beta", BETAS)
def test_the_seeds_of_the_gpu_fit_keep_every_check_away_from_tol(beta):
    """The GPU test asserts n_iter_ == the yardstick's: every ratio of the float64 stopping test must lie at least 10 % away from
    tol, so that the equality rests on the reference and not on rounding."""
    X, Y, U, V, Z = BY.fit_problem(BY.FIT_SEEDS[beta])
    _, _, _, n_iter, ratios = BY.fit(X, Y, U, V, Z, beta, 200, BY.FIT_TOL)
    margin = min(abs(r - BY.FIT_TOL) for r in ratios) / BY.FIT_TOL
    print("beta %g: stops at %d, ratios %s, smallest distance to tol %.3f tol" % (beta, n_iter, ["%.2e" % r for r in ratios], margin))
    assert ratios and margin >= 0.1 and 10 <= n_iter < 200


# ------------------------------------------------------------------ the loss and beta_loss keywords
def _data(m=8, d=6, p=4):
    rng = np.random.RandomState(0)
    return rng.rand(m, d) + 0.1, rng.rand(d, p) + 0.1


def test_loss_survives_clone_and_get_params():
    from sklearn.base import clone
    from pycmf_amd import CMF
    model = CMF(n_components=3, solver="mu", loss="beta-divergence", beta_loss=0.5)
    assert model.get_params()["loss"] == "beta-divergence" and model.get_params()["beta_loss"] == 0.5
    twin = clone(model)
    assert twin.loss == "beta-divergence" and twin.beta_loss == 0.5 and twin.get_params() == model.get_params()
    assert model._kwargs()["loss"] == "beta-divergence" and model._kwargs()["beta_loss"] == 0.5


@pytest.mark.parametrize("kwargs, match", [
    (dict(beta_loss=-0.1), r"beta_loss in \[0, 2\]"),
    (dict(beta_loss=2.5), r"beta_loss in \[0, 2\]"),
    (dict(beta_loss=float("nan")), r"beta_loss in \[0, 2\]"),
    (dict(beta_loss=float("inf")), r"beta_loss in \[0, 2\]"),
    (dict(beta_loss=True), "Invalid beta_loss"),
    (dict(beta_loss="poisson"), "Invalid beta_loss"),
    (dict(beta_loss=0.5, solver="newton"), "solver='mu'"),
    (dict(beta_loss=0.5, solver="als"), "solver='mu'"),
    (dict(beta_loss=0.5, n_gpus=2), "n_gpus must be 1"),
])
def test_fit_rejects_bad_arguments_before_any_device(no_device, kwargs, match):
    from pycmf_amd import CMF, collective_matrix_factorization
    X, Y = _data()
    kwargs.setdefault("solver", "mu")
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, loss="beta-divergence", **kwargs).fit(X, Y)
    with pytest.raises(ValueError, match=match):
        collective_matrix_factorization(X, Y, n_components=3, loss="beta-divergence", **kwargs)


@pytest.mark.parametrize("extra, match", [
    (dict(x_entry_weights=np.ones((8, 6))), "x_entry_weights"),
    (dict(y_entry_weights=np.ones((6, 4))), "y_entry_weights"),
    (dict(x_background_weight=0.5), "x_background_weight"),
    (dict(y_biases=True), "y_biases"),
])
def test_weights_background_and_biases_are_refused_with_this_loss(no_device, extra, match):
    from pycmf_amd import CMF
    X, Y = _data()
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, solver="mu", loss="beta-divergence", beta_loss=0.5).fit(X, Y, **extra)


@pytest.mark.parametrize("which", ["X", "Y"])
@pytest.mark.parametrize("sparse", [False, True])
def test_negative_data_is_refused_before_any_device(no_device, which, sparse):
    from pycmf_amd import CMF
    X, Y = _data()
    (X if which == "X" else Y)[1, 2] = -0.5
    if sparse:
        X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    with pytest.raises(ValueError, match="%s has negative entries" % which):
        CMF(n_components=3, solver="mu", loss="beta-divergence", beta_loss=1.5).fit(X, Y)


@pytest.mark.parametrize("beta_loss", [0, 0.0, "itakura-saito"])
def test_itakura_saito_refuses_zeros_and_sparse_relations(no_device, beta_loss):
    from pycmf_amd import CMF
    X, Y = _data()
    Xz = X.copy()
    Xz[2, 3] = 0.0
    with pytest.raises(ValueError, match="X has zeros"):
        CMF(n_components=3, solver="mu", loss="beta-divergence", beta_loss=beta_loss).fit(Xz, Y)
    Ys = sp.csr_matrix(Y * (Y > 0.5))
    with pytest.raises(ValueError, match="Y is sparse, its implicit zeros"):
        CMF(n_components=3, solver="mu", loss="beta-divergence", beta_loss=beta_loss).fit(X, Ys)


def test_solver_object_parses_beta_and_selects_the_path(no_device):
    from pycmf_amd.solver_shell import HipMUSolver, LOSSES
    assert LOSSES == ("frobenius", "kullback-leibler", "beta-divergence")
    s = HipMUSolver(loss="beta-divergence", beta_loss="itakura-saito")
    assert s.loss == "beta-divergence" and s.beta == 0.0 and s.beta_loss == 2.0 and s._path == "beta-divergence"
    assert s._run_params() is None and s._device_step_error(0, 0, 0.5) is None
    assert HipMUSolver(loss="beta-divergence", beta_loss=0.5).beta == 0.5
    assert HipMUSolver(200, 1e-4, 1.5, loss="beta-divergence").beta == 1.5          # positional, as the reference passes it
    assert HipMUSolver(loss="kullback-leibler", beta_loss=0.5).beta is None and HipMUSolver().beta is None
    with pytest.raises(ValueError, match=r"beta_loss in \[0, 2\]"):
        HipMUSolver(loss="beta-divergence", beta_loss=3)
    with pytest.raises(ValueError, match="x_entry_weights"):
        HipMUSolver(loss="beta-divergence", beta_loss=0.5, x_entry_weights=np.ones((8, 6)))
    X, Y = _data()
    X[0, 0] = 0.0
    with pytest.raises(ValueError, match="X has zeros"):
        s.update_step(X, Y, np.ones((8, 3)), np.ones((6, 3)), np.ones((4, 3)), 0, 0, 0.5)


class _Recorder:
    """Stands in for _lib.Context: records which step and error calls a solver makes."""

    def __init__(self, *a, **k):
        self.calls = []
        self.shape = None

    def set_problem(self, m, d, p, k):
        self.shape = (m, d, p, k)

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append(name)
            if name in ("kl_divergence", "beta_divergence", "residual_sq"):
                return 1.0, 1.0
            if name == "mu_step_error":
                return 1.0, 1.0
            if name == "get_factor":
                return 0.0
            return None
        return call


@pytest.mark.parametrize("beta_loss, step, err", [
    (2, "mu_step", "residual_sq"), ("frobenius", "mu_step", "residual_sq"),
    (1, "mu_kl_step", "kl_divergence"), ("kullback-leibler", "mu_kl_step", "kl_divergence"),
    (0.5, "mu_beta_step", "beta_divergence"), ("itakura-saito", "mu_beta_step", "beta_divergence"),
])
def test_beta_one_and_two_take_the_kl_and_frobenius_code_paths(monkeypatch, beta_loss, step, err):
    from pycmf_amd import _lib
    from pycmf_amd.solver_shell import HipMUSolver
    monkeypatch.setattr(_lib, "Context", _Recorder)
    s = HipMUSolver(loss="beta-divergence", beta_loss=beta_loss)
    X, Y = _data()
    U, V, Z = np.ones((8, 3)), np.ones((6, 3)), np.ones((4, 3))
    s.update_step(X, Y, U, V, Z, 0.0, 0.0, 0.5)
    s.compute_error(X, Y, U, V, Z)
    steps = [c for c in s._ctx.calls if c.endswith("_step")]
    errs = [c for c in s._ctx.calls if c in ("residual_sq", "kl_divergence", "beta_divergence")]
    assert steps == [step] and errs == [err]
    assert (s._run_params() is not None) == (step == "mu_step")


def test_a_sparse_relation_is_uploaded_dense_for_this_loss(monkeypatch):
    from pycmf_amd import _lib
    from pycmf_amd.solver_shell import HipMUSolver
    seen = []

    class Rec(_Recorder):
        def set_data(self, which, M):
            seen.append(sp.issparse(M))
    monkeypatch.setattr(_lib, "Context", Rec)
    X, Y = _data()
    Xs = sp.csr_matrix(X * (X > 0.5))
    U, V, Z = np.ones((8, 3)), np.ones((6, 3)), np.ones((4, 3))
    HipMUSolver(loss="beta-divergence", beta_loss=0.5).update_step(Xs, Y, U, V, Z, 0.0, 0.0, 0.5)
    assert seen == [False, False]
    del seen[:]
    HipMUSolver(loss="beta-divergence", beta_loss=1).update_step(Xs, Y, U, V, Z, 0.0, 0.0, 0.5)     # the KL path keeps the layout
    assert seen == [True, False]


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared_in_all_three_places():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11
    for name, nargs in (("cmf_mu_beta_step", 5), ("cmf_beta_divergence", 4), ("cmf_mu_beta_products", 5), ("cmf_mu_beta_layout", 2)):
        m = re.search(r"\bint %s\s*\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name])
    for name in ("mu_beta_step", "beta_divergence", "mu_beta_products", "mu_beta_layout"):
        assert callable(getattr(_lib.Context, name))
