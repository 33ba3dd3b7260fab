"""Host side of the HALS solver (no GPU): the float64 yardstick of the GPU tests against sklearn's compiled coordinate-descent
kernel, its corner cases, the monotone decrease of the objective, and the argument validation of ``solver='hals'`` -- which must
raise before any device is touched."""
import os
import re
import warnings

import numpy as np
import pytest

import hals_yardstick as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _problem(seed=3, m=23, d=17, p=11, k=6):
    rng = np.random.RandomState(seed)
    X, Y = np.abs(rng.randn(m, d)) * (rng.rand(m, d) < 0.8), np.abs(rng.randn(d, p)) * (rng.rand(d, p) < 0.8)
    U, V, Z = (np.abs(rng.randn(n, k)) * (rng.rand(n, k) < 0.9) for n in (m, d, p))
    return X, Y, U, V, Z


def _sklearn_sweep(F, N, G, l1, l2):
    """sklearn's _update_coordinate_descent without shuffling: HHt + l2 on the diagonal, XHt - l1, the compiled sweep."""
    from sklearn.decomposition._cdnmf_fast import _update_cdnmf_fast
    W = np.array(F, dtype=np.float64, order="C")
    HHt = np.array(G, dtype=np.float64, order="C")
    HHt.flat[::HHt.shape[0] + 1] += l2
    XHt = np.ascontiguousarray(N - l1 if l1 != 0 else N, dtype=np.float64)
    _update_cdnmf_fast(W, HHt, XHt, np.arange(F.shape[1], dtype=np.intp))
    return W


# ------------------------------------------------------------------ the yardstick against sklearn's compiled sweep
@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.3, 0.2)])
@pytest.mark.parametrize("which", ["U", "V", "Z"])
def test_sweep_equals_sklearns_coordinate_descent(which, l1, l2):
    X, Y, U, V, Z = _problem()
    F = {"U": U, "V": V, "Z": Z}[which]
    N, G = H.products(X, Y, U, V, Z, which)
    got, ref = H.hals_sweep(F, N, G, l1, l2), _sklearn_sweep(F, N, G, l1, l2)
    assert np.max(np.abs(got - ref)) <= 1e-12
    assert ((got == 0) == (ref == 0)).all() and (got == 0).any() and (got >= 0).all()
    assert (F == 0).sum() > 0 and (got[F == 0] > 0).any()          # exact zeros revive


def test_a_column_with_zero_curvature_is_left_unchanged():
    X, Y, U, V, Z = _problem()
    V[:, 2] = 0                                                     # then G[2, :] = V^T V[2, :] = 0 for the U and Z sweeps
    N, G = H.products(X, Y, U, V, Z, "U")
    assert G[2, 2] == 0 and (G[2] == 0).all()
    got = H.hals_sweep(U, N, G, 0.0, 0.0)
    assert (got[:, 2] == U[:, 2]).all() and (U[:, 2] != 0).any()
    assert not (got[:, 3] == U[:, 3]).all()
    assert not (H.hals_sweep(U, N, G, 0.0, 0.1)[:, 2] == U[:, 2]).all()   # l2 alone gives it curvature: shrinks towards 0


def test_jacobi_order_is_a_different_method():
    X, Y, U, V, Z = _problem()
    N, G = H.products(X, Y, U, V, Z, "V")
    a, b = H.hals_sweep(V, N, G), H.hals_sweep(V, N, G, jacobi=True)
    assert (a[:, 0] == b[:, 0]).all() and np.max(np.abs(a - b)) > 1e-3


@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6, 7])
def test_objective_never_increases_over_50_steps(mask, l1, l2):
    X, Y, U, V, Z = _problem(seed=5)
    prev = H.objective(X, Y, U, V, Z, l1, l2)
    first = prev
    for _ in range(50):
        Un, Vn, Zn = H.hals_step(X, Y, U, V, Z, l1, l2, mask)
        for bit, old, new in ((1, U, Un), (2, V, Vn), (4, Z, Zn)):
            assert (mask & bit) or (old == new).all()
        U, V, Z = Un, Vn, Zn
        cur = H.objective(X, Y, U, V, Z, l1, l2)
        assert cur <= prev * (1 + 1e-13)
        prev = cur
    assert prev < 0.9 * first


def test_float32_yardstick_follows_the_float64_one():
    X, Y, U, V, Z = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in _problem())
    a, b = H.hals_step(X, Y, U, V, Z, 0.05, 0.1), H.hals_step(X, Y, U, V, Z, 0.05, 0.1, dtype=np.float32)
    for x, y in zip(a, b):
        assert y.dtype == np.float32 and np.max(np.abs(x - y)) <= 1e-4 * np.max(np.abs(x))
        assert H.tolerance(y, x, 6) >= 22 * 2.0 ** -24 * np.max(np.abs(x))


def test_fit_loop_stops_like_the_reference_loop():
    X, Y, U, V, Z = _problem(seed=7)
    trace = []
    *_, n = H.hals_fit(X, Y, U, V, Z, max_iter=200, tol=1e-3, trace=trace)
    assert n == trace[-1][0] and n % 10 == 0 and trace[-1][2] < 1e-3 and all(t[2] >= 1e-3 for t in trace[:-1])
    assert H.hals_fit(X, Y, U, V, Z, max_iter=7, tol=0)[3] == 7


# ------------------------------------------------------------------ validation before any device is opened
def _fit_args():
    X, Y, U, V, Z = _problem()
    return X, Y


@pytest.mark.parametrize("flag", ["U_non_negative", "V_non_negative", "Z_non_negative"])
def test_signed_factors_are_refused(no_device, flag):
    from pycmf_amd import CMF, HipHALSSolver
    X, Y = _fit_args()
    with pytest.raises(ValueError, match="solver='newton'"):
        CMF(n_components=3, solver="hals", x_init="random", y_init="random", random_state=0, **{flag: False}).fit(X, Y)
    with pytest.raises(ValueError, match="solver='newton'"):
        HipHALSSolver(**{flag: False})


def test_more_than_one_gpu_is_refused(no_device):
    from pycmf_amd import CMF
    X, Y = _fit_args()
    with pytest.raises(ValueError, match="n_gpus must be 1"):
        CMF(n_components=3, solver="hals", x_init="random", y_init="random", random_state=0, n_gpus=2).fit(X, Y)


def test_kl_loss_and_entry_weights_are_refused_in_the_existing_words(no_device):
    from pycmf_amd import CMF
    X, Y = _fit_args()
    with pytest.raises(ValueError, match="solver='mu', got 'hals'"):
        CMF(n_components=3, solver="hals", loss="kullback-leibler", x_init="random", y_init="random", random_state=0).fit(X, Y)
    with pytest.raises(ValueError, match="x_entry_weights / y_entry_weights are implemented by the multiplicative-update solver only"):
        CMF(n_components=3, solver="hals", x_init="random", y_init="random", random_state=0).fit(X, Y, x_entry_weights=np.ones(X.shape))


def test_more_than_256_components_are_refused(no_device):
    from pycmf_amd import CMF
    rng = np.random.RandomState(0)
    X, Y = np.abs(rng.randn(300, 280)), np.abs(rng.randn(280, 270))
    with pytest.raises(NotImplementedError, match="n_components <= 256"):
        CMF(n_components=257, solver="hals", x_init="random", y_init="random", random_state=0).fit(X, Y)


def test_a_link_warns_and_the_fit_goes_on_to_the_device(no_device):
    from pycmf_amd import CMF
    X, Y = _fit_args()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(AssertionError, match="device context was opened"):
            CMF(n_components=3, solver="hals", x_link="logit", x_init="random", y_init="random", random_state=0).fit(X, Y)
    assert any("does not accept link functions other than linear" in str(x.message) and "hals" in str(x.message) for x in w)


@pytest.mark.parametrize("solver", ["mu", "newton", "hals"])
def test_known_solvers_dispatch_to_the_device(no_device, solver):
    from pycmf_amd import CMF
    X, Y = _fit_args()
    with pytest.raises(AssertionError, match="device context was opened"):
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0).fit(X, Y)


def test_solver_classes_dispatch_as_before(monkeypatch):
    """solver='mu' and 'newton' still build their own solver objects; 'hals' builds HipHALSSolver; 'cd' is not a name."""
    from pycmf_amd import estimator, solver_shell
    built = []

    class Stop(Exception):
        pass
    for name in ("HipMUSolver", "HipNewtonSolver", "HipHALSSolver"):
        def make(name=name):
            def ctor(*a, **k):
                built.append(name)
                raise Stop()
            return ctor
        monkeypatch.setattr(estimator, name, make())
    X, Y = _fit_args()
    for solver in ("mu", "newton", "hals"):
        with pytest.raises(Stop):
            estimator.collective_matrix_factorization(X, Y, n_components=3, solver=solver, x_init="random", y_init="random")
    assert built == ["HipMUSolver", "HipNewtonSolver", "HipHALSSolver"]
    with pytest.raises(ValueError, match="No such solver: cd"):
        estimator.collective_matrix_factorization(X, Y, n_components=3, solver="cd")
    s = solver_shell.HipHALSSolver(max_iter=5, tol=0.0, l1_reg=0.1, l2_reg=0.2)
    assert s._run_params() is None and s.alpha == 0.5 and s._update_mask() == 7


# ------------------------------------------------------------------ ABI surface
def test_entry_points_and_the_timing_class_are_declared_in_all_three_places():
    import pycmf_amd
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_HALS"] == enum["CMF_K_COUNT"] == _lib.LATER_KERNEL_CLASSES["hals"] and enum["CMF_K_END"] == enum["CMF_K_HALS"] + 1
    assert "hals" not in _lib.KERNEL_CLASSES
    for name, nargs in (("cmf_hals_step", 4), ("cmf_hals_sweep", 6)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert callable(_lib.Context.hals_step) and callable(_lib.Context.hals_sweep)
    assert "HipHALSSolver" in pycmf_amd.__all__ and callable(pycmf_amd.HipHALSSolver)


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    assert b"cmf_hals_step" in blob and b"cmf_hals_sweep" in blob and b"hals_sweep_kernel" in blob
