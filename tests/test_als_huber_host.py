"""The Huber loss of the ALS solver (x_huber_delta / y_huber_delta), host side: the majoriser, the NumPy yardstick
(huber_yardstick.py) -- descent on every route, robustness against planted outliers, the Frobenius fit under a delta no residual
reaches --, keyword validation before any device is opened, the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
import huber_yardstick as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


# ------------------------------------------------------------------ the majoriser
def test_half_quadratic_majoriser_bounds_the_loss_and_touches_it_at_the_current_residual():
    rng = np.random.RandomState(0)
    r, r0 = 20.0 * rng.randn(10000), 20.0 * rng.randn(10000)
    delta = np.exp(2.0 * rng.randn(10000))
    gap = H.bound(r, r0, delta) - H.rho(r, delta)
    print("smallest gap %.3e relative to rho" % float((gap / np.maximum(H.rho(r, delta), 1.0)).min()))
    assert (gap >= -1e-12 * np.maximum(H.rho(r, delta), 1.0)).all()
    for at in (r0, -r0):
        assert (H.bound(at, r0, delta) == H.rho(r0, delta)).all()
    assert (H.omega(np.array([0.0, 1.0, -1.0, 2.0, -4.0]), 1.0) == np.array([1.0, 1.0, 1.0, 0.5, 0.25])).all()
    assert (H.rho(np.array([0.0, 1.0, -2.0]), 1.0) == np.array([0.0, 0.5, 1.5])).all()


# ------------------------------------------------------------------ the yardstick
ROUTES = {"exact": (3, 0, dict()), "cg": (3, 0, dict(cg_steps=3)), "dual": (40, 0, dict(dual_max=128)),
          "nnls": (3, 7, dict(nn_sweeps=4)), "nncg": (3, 7, dict(nn_cg_steps=3, nn_sweeps=4))}
# (nncg: U and V, which read the observed X, run projected CG; Z reads the full Y alone, where nn_cg_steps selects nothing: it keeps the
# coordinate descent of nn_sweeps, as in test_als_nncg_host.py -- under nn_sweeps = 0 it would only be projected, without a guarantee)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("seed", [3, 5, 7])
def test_objective_never_rises_on_the_planted_problem(seed, route):
    """planted(seed), delta = 1 on X, Y full, l2 = 0.5, 10 iterations V, U, Z in float64: the Huber objective after every iteration
    is at most the one before it."""
    k, nn_mask, kw = ROUTES[route]
    P = H.planted(seed, k)
    trace = []
    H.fit(P.Rx, P.Ry, P.U, P.V, P.Z, P.max_iter, P.l2, deltas=(1.0, None), nn_mask=nn_mask, trace=trace, **kw)
    seq = [H.objective(P.Rx, P.Ry, P.U, P.V, P.Z, P.l2, deltas=(1.0, None))] + trace
    print("seed %d %s: %s" % (seed, route, " ".join("%.1f" % v for v in seq)))
    assert len(trace) == 10 and all(b <= a for a, b in zip(seq, seq[1:])), seq


@pytest.mark.parametrize("seed", [3, 5, 7])
def test_huber_fit_halves_the_error_on_the_clean_unobserved_cells(seed):
    P = H.planted(seed)
    Uf, Vf, Zf = A.fit(P.Rx, P.Ry, None, None, P.U, P.V, P.Z, P.max_iter, P.l2)[:3]
    Uh, Vh, Zh = H.fit(P.Rx, P.Ry, P.U, P.V, P.Z, P.max_iter, P.l2, deltas=(1.0, None))[:3]
    frob, huber = P.heldout_rmse(Uf, Vf), P.heldout_rmse(Uh, Vh)
    print("seed %d: RMSE on the clean unobserved cells, Frobenius %.3f, Huber %.3f" % (seed, frob, huber))
    assert huber < 0.5 * frob


def test_a_delta_no_residual_reaches_is_the_frobenius_fit():
    P = H.planted(3)
    ref = A.fit(P.Rx, P.Ry, None, None, P.U, P.V, P.Z, 4, P.l2)[:3]
    got = H.fit(P.Rx, P.Ry, P.U, P.V, P.Z, 4, P.l2, deltas=(1e30, None))[:3]
    assert all((a == b).all() for a, b in zip(ref, got))
    assert H.errors(P.Rx, P.Ry, *got, deltas=(1e30, None))[0] == pytest.approx(A.errors(P.Rx, P.Ry, None, None, *got)[0], rel=1e-14)


def test_planted_is_the_problem_of_the_issue():
    P = H.planted(3)
    assert P.X.shape == (120, 150) and P.Y.shape == (150, 20) and P.U.shape == (120, 3)
    assert 0.27 < P.M.mean() < 0.33 and 0.03 < P.outliers.sum() / P.M.sum() < 0.07
    assert np.allclose(np.abs(P.X - P.noisy)[P.outliers], 10.0) and (P.X == P.noisy)[~P.outliers].all()


# ------------------------------------------------------------------ validation before any device is opened
def _fit(kw, fit_kw=None, X=None, absolute=False):
    from pycmf_amd import CMF
    P = H.planted(3)
    if absolute:   # (the initialisers of non-negative factors refuse negative data)
        P.X, P.Y = np.abs(P.X), np.abs(P.Y)
    kw = dict(dict(solver="als", l2_reg=0.5, U_non_negative=False, V_non_negative=False, Z_non_negative=False), **kw)
    fit_kw = dict(x_entry_weights=P.W) if fit_kw is None else fit_kw
    return CMF(n_components=3, x_init="random", y_init="random", random_state=0, **kw).fit(P.X if X is None else X, P.Y, **fit_kw)


@pytest.mark.parametrize("kw, fit_kw, match", [
    (dict(x_huber_delta=0.0), None, "x_huber_delta must be None or a finite number > 0"),
    (dict(y_huber_delta=-1.0), None, "y_huber_delta must be None or a finite number > 0"),
    (dict(x_huber_delta=float("inf")), None, "x_huber_delta must be None or a finite number > 0"),
    (dict(x_huber_delta=float("nan")), None, "x_huber_delta must be None or a finite number > 0"),
    (dict(x_huber_delta=True), None, "x_huber_delta must be None or a finite number > 0"),
    (dict(x_huber_delta="1"), None, "x_huber_delta must be None or a finite number > 0"),
    (dict(x_huber_delta=1.0, solver="mu", l2_reg=0.0), dict(), "must be None with solver='mu'"),
    (dict(x_huber_delta=1.0, solver="hals", l2_reg=0.0), dict(), "must be None with solver='hals'"),
    (dict(x_huber_delta=1.0, n_gpus=2), dict(), "x_huber_delta runs on one GPU: n_gpus must be 1"),
    (dict(x_huber_delta=1.0), dict(), "x_huber_delta=1.0 needs x_entry_weights that name the observed entries.*got None"),
    (dict(x_huber_delta=1.0), "dense", "x_huber_delta=1.0 needs x_entry_weights that name the observed entries.*got a dense array"),
    (dict(y_huber_delta=2.0), None, "y_huber_delta=2.0 needs y_entry_weights"),
    (dict(x_huber_delta=1.0, x_link="logit"), None, "x_huber_delta=1.0 on a relation with x_link='logit' is not built"),
    (dict(x_huber_delta=1.0), "background", "x_huber_delta=1.0 together with x_background_weight=0.5 is not built"),
])
def test_bad_values_are_refused_before_a_device_is_touched(no_device, kw, fit_kw, match):
    P = H.planted(3)
    if fit_kw == "dense":
        fit_kw = dict(x_entry_weights=P.M.astype(float))
    elif fit_kw == "background":
        fit_kw = dict(x_entry_weights=P.W, x_background_weight=0.5)
    with pytest.raises(ValueError, match=match):
        _fit(kw, fit_kw)


def test_solver_object_validates_too_and_good_values_reach_the_device(no_device):
    from pycmf_amd import HipALSSolver
    from pycmf_amd.solver_shell import check_huber_delta
    with pytest.raises(ValueError, match="x_huber_delta must be None or a finite number > 0"):
        HipALSSolver(l2_reg=0.1, x_huber_delta=np.bool_(True))
    with pytest.raises(ValueError, match="y_huber_delta must be None or a finite number > 0"):
        HipALSSolver(l2_reg=0.1, y_huber_delta=-2)
    s = HipALSSolver(l2_reg=0.1, x_huber_delta=np.float32(0.5), loss="frobenius")
    assert (s.x_huber_delta, s.y_huber_delta, s.huber_loss, s.als_loss) == (0.5, None, None, "frobenius")
    assert HipALSSolver(l2_reg=0.1).x_huber_delta is None
    assert check_huber_delta(None, "x", "mu", 4) is None and check_huber_delta(2, "y") == 2.0
    for extra in (dict(), dict(als_nn_sweeps=4, U_non_negative=True), dict(als_cg_steps=3), dict(als_nn_cg_steps=3, V_non_negative=True),
                  dict(als_dual_max=64), dict(als_l2_scale=0.5), dict(y_huber_delta=None)):
        with pytest.raises(AssertionError, match="device context was opened"):
            _fit(dict(x_huber_delta=1.0, **extra), absolute=True)
    with pytest.raises(AssertionError, match="device context was opened"):
        _fit(dict(x_huber_delta=1.0), dict(x_entry_weights="observed"), X=sp.csr_matrix(np.where(H.planted(3).M, H.planted(3).X, 0.0)))


def test_the_options_survive_clone_set_params_and_repr(no_device):
    from sklearn.base import clone
    from pycmf_amd import CMF
    assert CMF().x_huber_delta is None and CMF().y_huber_delta is None
    assert "x_huber_delta" not in CMF(x_huber_delta=1.0).get_params()
    assert CMF(solver="als").get_params() == CMF(solver="als", x_huber_delta=1.0).get_params()
    assert vars(CMF(solver="als")) == vars(CMF(solver="als", x_huber_delta=None, y_huber_delta=None))
    with pytest.raises(TypeError, match="unexpected keyword argument 'x_huber_deltas'"):
        CMF(x_huber_deltas=1.0)
    first = CMF(n_components=3, solver="als", l2_reg=0.5, x_huber_delta=1.0)
    model = clone(first)
    assert model is not first and model.x_huber_delta == 1.0 and model._kwargs()["x_huber_delta"] == 1.0 and model._kwargs()["y_huber_delta"] is None
    assert model.get_params() == first.get_params() and clone(clone(model)).x_huber_delta == 1.0
    assert model.set_params(y_huber_delta=2.0, max_iter=7) is model and (model.x_huber_delta, model.y_huber_delta, model.max_iter) == (1.0, 2.0, 7)
    assert repr(model).endswith(", x_huber_delta=1.0, y_huber_delta=2.0)") and repr(CMF(y_huber_delta=0.5)) == "CMF(y_huber_delta=0.5)"
    assert "huber" not in repr(CMF(n_components=3))
    with pytest.raises(ValueError, match="x_huber_delta must be None or a finite number > 0"):
        clone(model).set_params(x_huber_delta=-3).fit(np.ones((4, 4)), np.ones((4, 4)))


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    for name, nargs in (("cmf_set_huber_delta", 3), ("cmf_get_huber_delta", 3), ("cmf_als_huber_loss", 3), ("cmf_als_huber_weights", 6)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("set_huber_delta", "get_huber_delta", "als_huber_loss", "als_huber_weights"))
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(CMF_K_\w+)\s*=\s*(\d+)", header)}
    assert enum["CMF_K_COUNT"] == 11                                              # (no new kernel class: CMF_K_KLMU)
    text = header[header.index("ALS with a Huber loss"):header.index("int cmf_set_huber_delta")]
    assert "CMF_EUNSUPPORTED" in text and "background weight" in text and "logistic loss" in text and "MU, HALS and Newton" in text


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    for name in (b"cmf_set_huber_delta", b"cmf_get_huber_delta", b"cmf_als_huber_loss", b"cmf_als_huber_weights", b"als_huber_pass_kernel"):
        assert name in blob, name
