"""Host side of the Kullback-Leibler loss (no GPU): the float64 yardstick of the GPU tests against sklearn's own multiplicative
update and divergence, its monotone decrease, its corner cases by hand, and the argument validation of ``loss=`` -- which must
raise before any device is touched."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import kl_yardstick as KL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
@pytest.mark.parametrize("sparse", [False, True])
def test_yardstick_is_sklearns_update_and_divergence(l1, l2, sparse):
    try:
        from sklearn.decomposition._nmf import _multiplicative_update_w, _multiplicative_update_h, _beta_divergence
    except ImportError:                                     # private names: only their absence may skip
        pytest.skip("this sklearn has no _multiplicative_update_w / _h")
    rng = np.random.RandomState(5)
    n, f, k = 23, 17, 4
    X = rng.poisson(1.0, (n, f)).astype(float)
    X[3] = 0
    X[:, 5] = 0
    W, H = np.abs(rng.randn(n, k)) + 0.1, np.abs(rng.randn(k, f)) + 0.1
    Xs = sp.csr_matrix(X) if sparse else X
    # single matrix X ~ W H as the U side of the collective model: X = U V^T with U = W, V = H^T, nothing on the Y side
    Y0, Z0 = np.zeros((f, 1)), np.zeros((1, k))
    # (sklearn >= 1.4 returns the updated factor, which it changed in place; earlier versions return the ratio)
    Wc = W.copy()
    ret = _multiplicative_update_w(Xs, Wc, H.copy(), beta_loss=1, l1_reg_W=l1, l2_reg_W=l2, gamma=1.0)[0]
    U1, _, _ = KL.step(Xs, Y0, W, H.T, Z0, l1, l2, mask=KL.U_BIT)
    assert _rel(U1, ret if ret is Wc else W * ret) <= 1e-12
    Hc = H.copy()
    ret = _multiplicative_update_h(Xs, W.copy(), Hc, beta_loss=1, l1_reg_H=l1, l2_reg_H=l2, gamma=1.0)
    _, V1, _ = KL.step(Xs, Y0, W, H.T, Z0, l1, l2, mask=KL.V_BIT)   # Z = 0: the y part of V's numerator and colsum Z vanish
    assert _rel(V1, (ret if ret is Hc else H * ret).T) <= 1e-12
    ref = _beta_divergence(Xs, W, H, 1, square_root=False)
    assert abs(KL.divergence(Xs, W, H.T) - ref) <= 1e-12 * abs(ref)
    ref = _beta_divergence(Xs, W, H, 1, square_root=True)
    assert abs(KL.errors(Xs, Y0, W, H.T, Z0)[0] - ref) <= 1e-12 * abs(ref)


def _problem(kind, seed, m=40, d=55, p=13, k=5):
    rng = np.random.RandomState(seed)
    if kind == "dense":
        X, Y = np.abs(rng.randn(m, d)), np.abs(rng.randn(d, p))
    else:
        X, Y = rng.poisson(1.0, (m, d)).astype(float), rng.poisson(1.0, (d, p)).astype(float)
        X[2] = 0
        X[:, 7] = 0
    U, V, Z = (np.abs(rng.randn(n, k)) + 0.1 for n in (m, d, p))
    return X, Y, U, V, Z


@pytest.mark.parametrize("kind", ["dense", "counts"])
def test_collective_objective_decreases_monotonically(kind):
    X, Y, U, V, Z = _problem(kind, 11)
    prev = KL.objective(X, Y, U, V, Z)
    for _ in range(30):
        U, V, Z = KL.step(X, Y, U, V, Z)
        cur = KL.objective(X, Y, U, V, Z)
        assert np.isfinite(cur) and cur <= prev * (1 + 1e-13)
        prev = cur
    assert all(np.isfinite(F).all() and (F >= 0).all() for F in (U, V, Z))
    if kind == "counts":
        assert (U[2] == 0).all()          # the all-zero row of X: its factor row goes to exactly 0 in the first sweep


def test_sparse_and_dense_yardstick_agree():
    X, Y, U, V, Z = _problem("counts", 4)
    a = KL.step(X, Y, U, V, Z, 0.1, 0.2)
    b = KL.step(sp.csr_matrix(X), sp.csr_matrix(Y), U, V, Z, 0.1, 0.2)
    for Fa, Fb in zip(a, b):
        assert _rel(Fa + 1.0, Fb + 1.0) <= 1e-13
    assert abs(KL.divergence(X, U, V) - KL.divergence(sp.csr_matrix(X), U, V)) <= 1e-12 * KL.divergence(X, U, V)


def test_corner_cases_by_hand():
    E = KL.EPS
    # one component, X 2 x 2: S = u v^T
    X = np.array([[2.0, 0.0], [0.0, 0.0]])         # a zero row and a zero column
    U, V = np.array([[1.0], [3.0]]), np.array([[2.0], [5.0]])
    Y, Z = np.zeros((2, 1)), np.zeros((1, 1))
    # U numerator: row 0 = 2 / (1 * 2) * 2 = 2, row 1 = 0; denominator colsum V = 7
    U1, _, _ = KL.step(X, Y, U, V, Z, mask=KL.U_BIT)
    assert U1[0, 0] == 1.0 * (2.0 / 7.0) and U1[1, 0] == 0.0
    # V numerator (x part): row 0 = 2 / 2 * 1 = 1, row 1 = 0; denominator colsum U + colsum Z = 4
    _, V1, _ = KL.step(X, Y, U, V, Z, mask=KL.V_BIT)
    assert V1[0, 0] == 2.0 * (1.0 / 4.0) and V1[1, 0] == 0.0
    # S < EPS: the quotient divides by EPS, not by S
    Us, Vs = np.array([[1e-5]]), np.array([[1e-5]])
    assert KL.numerator(np.array([[3.0]]), Us, Vs)[0, 0] == 3.0 / E * 1e-5
    # S = 0 under a zero of T: exact zero, no 0 / 0
    assert KL.numerator(np.array([[0.0]]), np.zeros((1, 1)), Vs)[0, 0] == 0.0
    # zero denominator: colsum = 0, l1 = l2 = 0 -> EPS; with the factor at 0 the update stays 0 and finite
    U2, _, _ = KL.step(np.array([[1.0]]), np.zeros((1, 1)), np.array([[2.0]]), np.zeros((1, 1)), np.zeros((1, 1)), mask=KL.U_BIT)
    assert U2[0, 0] == 2.0 * ((1.0 / E * 0.0) / E) == 0.0
    assert (KL.reg(np.zeros(2), np.zeros((3, 2)), 0.0, 0.0) == E).all()
    assert (KL.reg(np.zeros(2), np.ones((3, 2)), 0.5, 2.0) == 2.5).all()
    # divergence: t = 0 contributes s; t > 0 with s = 0 counts s as EPS in the log
    assert KL.divergence(np.array([[0.0]]), np.array([[2.0]]), np.array([[3.0]])) == 6.0
    assert KL.divergence(np.array([[2.0]]), np.array([[1.0]]), np.array([[2.0]])) == 0.0
    assert KL.divergence(np.array([[1.0]]), np.zeros((1, 1)), np.ones((1, 1))) == np.log(1.0 / E) - 1.0


def test_tolerance_functions():
    assert KL.tau(7, 1031) == (7 + 2062 + 16) * 2.0 ** -24
    assert KL.div_tol(5, 1.0, 2.0, 3.0) == 21 * 2.0 ** -24 * 6.0


# ------------------------------------------------------------------ the loss keyword
def _data(m=8, d=6, p=4):
    rng = np.random.RandomState(0)
    return rng.rand(m, d), rng.rand(d, p)


def test_loss_is_a_constructor_parameter_and_survives_clone():
    from sklearn.base import clone
    from pycmf_amd import CMF
    assert CMF().loss == "frobenius" and CMF().get_params()["loss"] == "frobenius"
    model = CMF(n_components=3, solver="mu", loss="kullback-leibler")
    assert model.get_params()["loss"] == "kullback-leibler"
    twin = clone(model)
    assert twin.loss == "kullback-leibler" and twin.get_params() == model.get_params()
    assert model._kwargs()["loss"] == "kullback-leibler"


@pytest.mark.parametrize("kwargs, match", [
    (dict(loss="itakura-saito"), "Invalid loss"),
    (dict(loss="kl"), "Invalid loss"),
    (dict(loss=1), "Invalid loss"),
    (dict(loss="kullback-leibler", solver="newton"), "solver='mu'"),
    (dict(loss="kullback-leibler", solver="mu", n_gpus=2), "n_gpus must be 1"),
])
def test_fit_rejects_bad_loss_arguments_before_any_device(no_device, kwargs, match):
    from pycmf_amd import CMF
    X, Y = _data()
    kwargs.setdefault("solver", "mu")
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, **kwargs).fit(X, Y)


@pytest.mark.parametrize("which", ["X", "Y"])
@pytest.mark.parametrize("sparse", [False, True])
def test_kl_rejects_negative_data_before_any_device(no_device, which, sparse):
    from pycmf_amd import CMF, collective_matrix_factorization
    X, Y = _data()
    (X if which == "X" else Y)[1, 2] = -0.5
    if sparse:
        X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    with pytest.raises(ValueError, match="%s has negative entries" % which):
        CMF(n_components=3, solver="mu", loss="kullback-leibler").fit(X, Y)
    with pytest.raises(ValueError, match="%s has negative entries" % which):
        collective_matrix_factorization(X, Y, n_components=3, solver="mu", loss="kullback-leibler")


def test_solver_object_validates_loss_and_data_without_a_device(no_device):
    from pycmf_amd.solver_shell import HipMUSolver
    with pytest.raises(ValueError, match="Invalid loss"):
        HipMUSolver(loss="poisson")
    s = HipMUSolver(loss="kullback-leibler", beta_loss="kullback-leibler")
    assert s.loss == "kullback-leibler" and s.beta_loss == 2.0     # beta_loss keeps its meaning: none
    assert s._run_params() is None and s._device_step_error(0, 0, 0.5) is None
    assert HipMUSolver()._run_params() is not None
    X, Y = _data()
    X[0, 0] = -1.0
    k = 3
    with pytest.raises(ValueError, match="X has negative entries"):
        s.update_step(X, Y, np.ones((8, k)), np.ones((6, k)), np.ones((4, k)), 0, 0, 0.5)


def test_frobenius_fit_with_the_keyword_takes_the_old_path(no_device):
    """loss='frobenius' changes nothing: the fit reaches the device exactly as before (here: the fixture's refusal)."""
    from pycmf_amd import CMF
    X, Y = _data()
    with pytest.raises(AssertionError, match="device context was opened"):
        CMF(n_components=3, solver="mu", loss="frobenius", x_init="random", y_init="random", random_state=0).fit(X, Y)


# ------------------------------------------------------------------ ABI surface
def test_kernel_class_and_entry_points_are_declared_in_all_three_places():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_KLMU"] == 10 == _lib.KERNEL_CLASSES["klmu"]
    assert enum["CMF_K_COUNT"] == 11 == len(_lib.KERNEL_CLASSES) == 1 + max(_lib.KERNEL_CLASSES.values())
    for name in ("cmf_mu_kl_step", "cmf_kl_divergence", "cmf_mu_kl_layout"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES
    for name in ("mu_kl_step", "kl_divergence", "mu_kl_layout"):
        assert callable(getattr(_lib.Context, name))
