"""Host side of the per-entry weights (no GPU): the float64 yardstick of the GPU tests against the oracle's MU step at W = 1, its
sparse and dense forms against each other, corner cases by hand, the monotone decrease of the weighted objective, and the argument
validation of ``x_entry_weights`` / ``y_entry_weights`` -- which must raise before any device is touched."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import wmu_yardstick as WM

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


def _problem(seed=3, m=23, d=17, p=11, k=6):
    rng = np.random.RandomState(seed)
    X, Y = np.abs(rng.randn(m, d)) * (rng.rand(m, d) < 0.8), np.abs(rng.randn(d, p)) * (rng.rand(d, p) < 0.8)
    U, V, Z = (np.abs(rng.randn(n, k)) + 0.1 for n in (m, d, p))
    return X, Y, U, V, Z


# ------------------------------------------------------------------ yardstick against the oracle at W = 1
@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("form", ["none", "dense", "csr"])
def test_yardstick_at_unit_weights_is_the_oracles_mu_step(form, mask, l1, l2):
    from oracle.cmf_oracle import mu_update_step
    X, Y, U, V, Z = _problem()
    ones = {"none": lambda s: None, "dense": np.ones, "csr": lambda s: sp.csr_matrix(np.ones(s))}[form]
    got = WM.step(X, Y, ones(X.shape), ones(Y.shape), U, V, Z, l1, l2, mask)
    Ur, Vr, Zr = U.copy(), V.copy(), Z.copy()
    mu_update_step(X, Y, Ur, Vr, Zr, l1, l2, update_U=bool(mask & 1), update_V=bool(mask & 2), update_Z=bool(mask & 4))
    for g, r in zip(got, (Ur, Vr, Zr)):
        assert _rel(g, r) <= 1e-12


@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("sparse_data", [False, True])
def test_sparse_and_dense_forms_of_the_same_weights_agree(l1, l2, sparse_data):
    X, Y, U, V, Z = _problem(seed=8)
    rng = np.random.RandomState(1)
    Wx = (rng.rand(*X.shape) + 0.25) * (rng.rand(*X.shape) < 0.6)
    Wy = (rng.rand(*Y.shape) + 0.25) * (rng.rand(*Y.shape) < 0.6)
    Wx[4] = 0
    Wy[:, 2] = 0
    Xi, Yi = (sp.csr_matrix(X), sp.csr_matrix(Y)) if sparse_data else (X, Y)
    dense = WM.step(Xi, Yi, Wx, Wy, U, V, Z, l1, l2)
    sparse = WM.step(Xi, Yi, sp.csr_matrix(Wx), sp.csr_matrix(Wy), U, V, Z, l1, l2)
    for a, b in zip(dense, sparse):
        assert _rel(a, b) <= 1e-12
    for T, W, A, B in ((Xi, Wx, U, V), (Yi, Wy, V, Z)):
        assert np.allclose(WM.residual_terms(T, W, A, B), WM.residual_terms(T, sp.csr_matrix(W), A, B), rtol=1e-12, atol=0)
    assert abs(WM.objective(Xi, Yi, Wx, Wy, U, V, Z, l1, l2) - WM.objective(X, Y, sp.csr_matrix(Wx), sp.csr_matrix(Wy), U, V, Z, l1, l2)) <= 1e-12 * WM.objective(X, Y, Wx, Wy, U, V, Z, l1, l2)


# ------------------------------------------------------------------ by hand
def test_two_by_two_with_one_observed_cell():
    X = np.array([[3.0, 5.0], [7.0, 11.0]])
    W = np.array([[0.0, 2.0], [0.0, 0.0]])                     # only (0, 1) is observed, with weight 2
    U, V = np.array([[1.0], [4.0]]), np.array([[2.0], [0.5]])
    Y, Z = np.zeros((2, 1)), np.zeros((1, 1))
    U1, _, _ = WM.step(X, Y, W, None, U, V, Z, mask=WM.U_BIT)
    # row 0: num = 2 * 5 * 0.5 = 5, den = 2 * (1 * 0.5) * 0.5 = 0.5 -> 1 * 5 / 0.5 = 10 = X[0, 1] / V[1]; row 1: nothing observed -> 0
    assert U1[0, 0] == 10.0 and U1[1, 0] == 0.0
    _, V1, _ = WM.step(X, Y, W, None, U, V, Z, mask=WM.V_BIT)
    # V row 1: num = 2 * 5 * 1 = 10, den = 2 * 0.5 * 1 = 1 -> 0.5 * 10 = 5; V row 0: no observed cell on the X side, Y = 0, Z = 0 -> 0
    assert V1[1, 0] == 5.0 and V1[0, 0] == 0.0
    assert WM.residual_terms(X, W, U, V) == (2 * (5 - 0.5) ** 2, 2 * 4.5 * 0.5)
    assert WM.residual_terms(X, sp.csr_matrix(W), U, V) == (2 * (5 - 0.5) ** 2, 2 * 4.5 * 0.5)


def test_a_row_without_observed_cells_goes_to_exact_zero():
    X, Y, U, V, Z = _problem(seed=2)
    W = np.ones(X.shape)
    W[5] = 0
    for Wf in (W, sp.csr_matrix(W)):
        U1, _, _ = WM.step(X, Y, Wf, None, U, V, Z, mask=WM.U_BIT)           # den 0 -> EPS, num 0: U * (0 / EPS)
        assert (U1[5] == 0).all() and (np.delete(U1, 5, axis=0) > 0).all()
        U2, _, _ = WM.step(X, Y, Wf, None, U, V, Z, 0.05, 0.1, mask=WM.U_BIT)  # den = l1 + l2 U > 0, num 0
        assert (U2[5] == 0).all()


def test_reg_and_the_tolerance_functions():
    F = np.array([[1.0, 2.0]])
    assert (WM.reg(np.array([[0.0, 3.0]]), F, 0.0, 0.0) == [[WM.EPS, 3.0]]).all()
    assert (WM.reg(np.array([[0.0, 3.0]]), F, 0.5, 0.0) == [[0.5, 3.5]]).all()
    assert (WM.reg(np.array([[0.0, 3.0]]), F, 0.5, 0.25) == [[0.75, 4.0]]).all()
    assert (WM.reg(np.array([[0.0, 3.0]]), F, 0.0, 0.25) == [[0.25, 3.5]]).all()
    assert WM.EPS == 2.0 ** -23
    assert WM.tau(7, 100) == (7 + 200 + 16) * 2.0 ** -24
    assert WM.tau(256, 65536 + 256) == (256 + 2 * 65792 + 16) * 2.0 ** -24
    assert WM.resid_tol(6, 10.0, 3.0) == 2.0 ** -24 * (2 * 8 * 10.0 + 8 * 3.0)


# ------------------------------------------------------------------ monotone
@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("weights", ["mask", "real", "csr-mask", "x-only"])
def test_the_weighted_objective_never_rises(weights, l1, l2):
    X, Y, U, V, Z = _problem(seed=11, m=40, d=30, p=12, k=4)
    rng = np.random.RandomState(4)
    if weights in ("mask", "csr-mask"):
        Wx, Wy = (rng.rand(*X.shape) < 0.4).astype(float), (rng.rand(*Y.shape) < 0.4).astype(float)
        if weights == "csr-mask":
            Wx, Wy = sp.csr_matrix(Wx), sp.csr_matrix(Wy)
    elif weights == "real":
        Wx, Wy = rng.rand(*X.shape) * 3, rng.rand(*Y.shape) * 3
    else:
        Wx, Wy = (rng.rand(*X.shape) < 0.4).astype(float), None
    prev = WM.objective(X, Y, Wx, Wy, U, V, Z, l1, l2)
    for _ in range(50):
        U, V, Z = WM.step(X, Y, Wx, Wy, U, V, Z, l1, l2)
        cur = WM.objective(X, Y, Wx, Wy, U, V, Z, l1, l2)
        assert cur <= prev * (1 + 1e-12)
        prev = cur


def test_fit_returns_the_ratios_of_every_check():
    X, Y, U, V, Z = _problem(seed=11, m=40, d=30, p=12, k=4)
    W = (np.random.RandomState(0).rand(*X.shape) < 0.5).astype(float)
    *_, n_iter, ratios = WM.fit(X, Y, W, None, U, V, Z, 200, 1e-3)
    assert n_iter % 10 == 0 and len(ratios) == n_iter // 10 and ratios[-1] < 1e-3 and all(r >= 1e-3 for r in ratios[:-1])
    *_, n_iter, ratios = WM.fit(X, Y, W, None, U, V, Z, 7, 0)
    assert n_iter == 7 and ratios == []


# ------------------------------------------------------------------ validation, before any device
def _data():
    rng = np.random.RandomState(0)
    return np.abs(rng.randn(8, 6)), np.abs(rng.randn(6, 4))


def _bad(kind, shape):
    W = np.ones(shape)
    if kind == "shape":
        return np.ones((shape[0] + 1, shape[1]))
    W[1, 2] = {"negative": -0.5, "nan": np.nan, "inf": np.inf}[kind]
    return W


@pytest.mark.parametrize("kind, match", [("negative", "non-negative"), ("nan", "finite"), ("inf", "finite"), ("shape", "has shape")])
@pytest.mark.parametrize("side", ["x", "y"])
@pytest.mark.parametrize("sparse_w", [False, True])
def test_bad_weights_are_refused_before_any_device(no_device, kind, match, side, sparse_w):
    from pycmf_amd import CMF, collective_matrix_factorization
    X, Y = _data()
    W = _bad(kind, X.shape if side == "x" else Y.shape)
    if sparse_w:
        W = sp.csr_matrix(W)
    kw = {side + "_entry_weights": W}
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, solver="mu").fit(X, Y, **kw)
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, solver="mu").fit_transform(X, Y, **kw)
    with pytest.raises(ValueError, match=match):
        collective_matrix_factorization(X, Y, n_components=3, solver="mu", **kw)


@pytest.mark.parametrize("ctor, match", [
    (dict(solver="newton"), "solver='mu'"),
    (dict(solver="mu", loss="kullback-leibler"), "loss='frobenius'"),
    (dict(solver="mu", n_gpus=2), "n_gpus must be 1"),
])
def test_weights_need_mu_frobenius_and_one_gpu(no_device, ctor, match):
    from pycmf_amd import CMF
    X, Y = _data()
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, **ctor).fit(X, Y, x_entry_weights=np.ones(X.shape))
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, **ctor).fit(X, Y, y_entry_weights=sp.csr_matrix(np.ones(Y.shape)))


def test_observed_needs_a_sparse_relation_and_other_strings_are_refused(no_device):
    from pycmf_amd import CMF
    X, Y = _data()
    with pytest.raises(ValueError, match="'observed' needs a SciPy sparse X"):
        CMF(n_components=3, solver="mu").fit(X, Y, x_entry_weights="observed")
    with pytest.raises(ValueError, match="'observed' needs a SciPy sparse Y"):
        CMF(n_components=3, solver="mu").fit(sp.csr_matrix(X), Y, x_entry_weights="observed", y_entry_weights="observed")
    with pytest.raises(ValueError, match="instead of an array"):
        CMF(n_components=3, solver="mu").fit(sp.csr_matrix(X), Y, x_entry_weights="seen")


def test_transform_validates_its_weights_before_any_device(no_device):
    from pycmf_amd import CMF
    X, Y = _data()
    model = CMF(n_components=3, solver="mu")
    model.x_weights, model.components, model.y_weights = np.ones((8, 3)), np.ones((6, 3)), np.ones((4, 3))
    with pytest.raises(ValueError, match="non-negative"):
        model.transform(X, None, x_entry_weights=-np.ones(X.shape))
    with pytest.raises(ValueError, match="relation that is not"):
        model.transform(X, None, y_entry_weights=np.ones(Y.shape))


def test_solver_object_takes_the_keywords_and_keeps_the_loop_on_the_host(no_device):
    from pycmf_amd.solver_shell import HipMUSolver
    X, Y = _data()
    s = HipMUSolver(x_entry_weights=np.ones(X.shape))
    assert s._run_params() is None and s._device_step_error(0, 0, 0.5) is None
    assert HipMUSolver()._run_params() is not None and HipMUSolver()._weights_key() == ()
    with pytest.raises(ValueError, match="loss='frobenius'"):
        HipMUSolver(loss="kullback-leibler", y_entry_weights=np.ones(Y.shape))
    bad = HipMUSolver(x_entry_weights=-np.ones(X.shape))
    with pytest.raises(ValueError, match="non-negative"):
        bad.update_step(X, Y, np.ones((8, 3)), np.ones((6, 3)), np.ones((4, 3)), 0, 0, 0.5)


def test_what_the_host_hands_to_the_library():
    """'observed': every stored entry, explicit zeros included, with weight 1.  A sparse W: its stored pattern (stored zero weights
    included) with the relation gathered on it, from a dense or a sparse relation alike.  A dense W on a sparse relation: both dense."""
    from pycmf_amd.solver_shell import resolve_entry_weights
    X = sp.csr_matrix((np.array([2.0, 0.0, 5.0, 7.0]), np.array([1, 3, 0, 3]), np.array([0, 2, 2, 4])), shape=(3, 4))
    assert X.nnz == 4                                            # (0, 3) is a stored zero
    ew = resolve_entry_weights(X, "observed", "x")
    assert ew.kind == "csr" and ew.indptr.tolist() == [0, 2, 2, 4] and ew.indices.tolist() == [1, 3, 0, 3]
    assert ew.t.tolist() == [2.0, 0.0, 5.0, 7.0] and ew.w.tolist() == [1.0, 1.0, 1.0, 1.0]
    assert ew.indptr.dtype == np.int64 and ew.indices.dtype == np.int32
    # CSC input, unsorted indices: the canonical CSR pattern, the caller's matrix untouched
    Xc = X.tocsc()
    ew = resolve_entry_weights(Xc, "observed", "x")
    assert ew.indices.tolist() == [1, 3, 0, 3] and ew.t.tolist() == [2.0, 0.0, 5.0, 7.0]
    W = sp.csr_matrix((np.array([0.5, 0.0, 3.0]), np.array([1, 2, 3]), np.array([0, 2, 2, 3])), shape=(3, 4))
    for M in (X, X.toarray()):
        ew = resolve_entry_weights(M, W, "x")
        assert ew.kind == "csr" and ew.indptr.tolist() == [0, 2, 2, 3] and ew.indices.tolist() == [1, 2, 3]
        assert ew.w.tolist() == [0.5, 0.0, 3.0] and ew.t.tolist() == [2.0, 0.0, 7.0]
    ew = resolve_entry_weights(X, np.full((3, 4), 2.0), "x")
    assert ew.kind == "dense" and isinstance(ew.data, np.ndarray) and (ew.data == X.toarray()).all() and (ew.W == 2.0).all()
    assert resolve_entry_weights(X, None, "x") is None


def test_get_params_and_clone_do_not_know_the_keywords():
    from sklearn.base import clone
    from pycmf_amd import CMF
    model = CMF(n_components=3, solver="mu")
    assert not any("entry_weights" in name for name in model.get_params())
    assert clone(model).get_params() == model.get_params()


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared_in_all_three_places():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    for name in ("cmf_set_weight_f64", "cmf_set_weight_f32", "cmf_set_weighted_csr", "cmf_clear_weight", "cmf_mu_weighted_step",
                 "cmf_weighted_residual_sq", "cmf_mu_weighted_layout", "cmf_fill_weight_synthetic", "cmf_get_weight_block_f32"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES
    for name in ("set_weight", "set_weighted_csr", "clear_weight", "mu_weighted_step", "weighted_residual_sq", "mu_weighted_layout",
                 "fill_weight_synthetic", "get_weight_block"):
        assert callable(getattr(_lib.Context, name))
