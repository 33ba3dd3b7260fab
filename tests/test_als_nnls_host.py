"""Non-negative row solve of the ALS solver, host side: the NumPy yardstick (als_yardstick.py) against scipy's NNLS and the
KKT conditions, the planted problem of the documentation against the projection and the weighted MU yardstick, one pass against
the HALS yardstick, keyword validation before any device is opened, the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.linalg
import scipy.optimize
import scipy.sparse as sp

import als_yardstick as A
import hals_yardstick as HY
import wmu_yardstick as WM
from test_gpu_wmu import fit_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _planted():
    X, Y, Wx, _, U, V, Z = fit_inputs(3, m=120, d=150, p=20, k=3, obs=.3)
    return X, Y, Wx, U, V, Z


# ------------------------------------------------------------------ the yardstick
def test_many_sweeps_reach_the_nnls_solution_and_its_kkt_conditions():
    """The U systems of the planted problem: 2000 passes equal scipy.optimize.nnls on the Cholesky-transformed system
    (|L^T f - L^-1 g|^2 = f^T H f - 2 g^T f + const) within 1e-10 relative (measured 1.3e-15), and satisfy f >= 0,
    (H f - g)_j >= -eps where f_j = 0, |(H f - g)_j| <= eps where f_j > 0."""
    X, Y, Wx, U, V, Z = _planted()
    H, g = A.systems(A.Relation(X, sp.csr_matrix(Wx)), A.Relation(Y, None), U, V, Z, "U", 0.05)
    F = A.cd_rows(H, g, U, 2000)
    ref = np.empty_like(F)
    for i in range(len(F)):
        L = np.linalg.cholesky(H[i])
        ref[i] = scipy.optimize.nnls(L.T, scipy.linalg.solve_triangular(L, g[i], lower=True))[0]
    rel = np.abs(F - ref).max() / np.abs(ref).max()
    grad = np.einsum("nij,nj->ni", H, F) - g
    eps = 1e-10 * (np.abs(g).max() + np.abs(np.einsum("nij,nj->ni", H, F)).max())
    print("cd_rows against scipy nnls: %.2e relative; clipped coordinates %d of %d" % (rel, int((F == 0).sum()), F.size))
    assert rel <= 1e-10
    assert (F >= 0).all() and (grad[F == 0] >= -eps).all() and (np.abs(grad[F > 0]) <= eps).all()
    assert (F == 0).any() and (F > 0).any()


def test_planted_problem_descends_and_beats_projection_and_300_mu_iterations():
    """Planted rank 3, 120 x 150, 30 % of X observed, Y unweighted, l2 = 0.05, all three factors non-negative, 4 passes, 10
    iterations (float64: objective 42.69 against 44.15 for the weighted MU after 300 iterations and 90.69 for the projection
    after 10; RMSE on the unobserved cells 0.0677 against 0.0842 and 0.1521)."""
    X, Y, Wx, U, V, Z = _planted()
    l2 = 0.05
    Ws = sp.csr_matrix(Wx)
    trace = []
    Un, Vn, Zn = A.fit(X, Y, Ws, None, U, V, Z, 10, l2, nn_mask=7, nn_sweeps=4, trace=trace)[:3]
    seq = [A.objective(X, Y, Wx, None, U, V, Z, l2)] + trace
    assert len(trace) == 10 and all(b <= a * (1 + 1e-12) for a, b in zip(seq, seq[1:])), seq
    assert min(Un.min(), Vn.min(), Zn.min()) >= 0
    Um, Vm, Zm, _, _ = WM.fit(X, Y, Wx, None, U, V, Z, 300, 0, l2=l2)
    Up, Vp, Zp, _, _ = A.fit(X, Y, Ws, None, U, V, Z, 10, l2, nn_mask=7)
    mu, proj = (A.objective(X, Y, Wx, None, P, Q, R, l2) for P, Q, R in ((Um, Vm, Zm), (Up, Vp, Zp)))
    unobserved = Wx == 0
    rmse = [float(np.sqrt((((X - P @ Q.T) ** 2)[unobserved]).mean())) for P, Q in ((Un, Vn), (Um, Vm), (Up, Vp))]
    print("objective: start %.1f, CD %s; MU after 300: %.2f; projection after 10: %.2f; RMSE on the unobserved cells: CD %.4f, MU %.4f, "
          "projection %.4f" % (seq[0], " ".join("%.2f" % t for t in trace), mu, proj, rmse[0], rmse[1], rmse[2]))
    assert trace[-1] < mu and trace[-1] < proj
    assert rmse[0] < rmse[1] and rmse[0] < rmse[2]


def test_one_sweep_on_an_unweighted_problem_is_a_hals_step():
    """No weights at all: every row of a sweep has the one Gram, and one pass is hals_yardstick's step with l1 = 0."""
    X, Y, _, U, V, Z = _planted()
    l2 = 0.05
    got = A.step(X, Y, None, None, U, V, Z, l2, nn_mask=7, nn_sweeps=1)
    ref = HY.hals_step(X, Y, U, V, Z, 0.0, l2)
    for a, b in zip(got, ref):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    # a signed V (nn_mask without its bit) takes the exact solve
    got = A.step(X, Y, None, None, U, V, Z, l2, nn_mask=5, nn_sweeps=1)
    assert (got[1] == A.step(X, Y, None, None, U, V, Z, l2, mask=A.V_BIT)[1]).all()


def test_rows_without_information_become_zeros():
    X, Y, Wx, U, V, Z = _planted()
    Wx = Wx.copy()
    Wx[7] = 0
    Un, _, _ = A.step(X, Y, sp.csr_matrix(Wx), None, U, V, Z, 0.05, mask=A.U_BIT, nn_mask=7, nn_sweeps=4)
    assert (Un[7] == 0).all() and (Un.sum(axis=1) > 0).sum() == len(Un) - 1


# ------------------------------------------------------------------ validation before any device is opened
@pytest.mark.parametrize("value", [-1, 1025, 2.0, "4", None, True])
def test_bad_sweep_counts_are_refused_before_a_device_is_touched(no_device, value):
    from pycmf_amd import CMF, HipALSSolver
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_nn_sweeps must be an integer 0 .. 1024"):
        CMF(n_components=3, solver="als", l2_reg=0.05, x_init="random", y_init="random", random_state=0, als_nn_sweeps=value).fit(X, Y)
    with pytest.raises(ValueError, match="als_nn_sweeps must be an integer 0 .. 1024"):
        HipALSSolver(l2_reg=0.05, nn_sweeps=value)


@pytest.mark.parametrize("solver", ["mu", "hals", "newton"])
def test_other_solvers_refuse_the_keyword(no_device, solver):
    from pycmf_amd import CMF
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_nn_sweeps is the non-negative row solve of solver='als'"):
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, als_nn_sweeps=4).fit(X, Y)
    with pytest.raises(AssertionError, match="device context was opened"):        # 0 is every solver's default: the fit goes on
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, als_nn_sweeps=0).fit(X, Y)


def test_good_keyword_reaches_the_solver_and_survives_clone(no_device):
    from sklearn.base import clone
    from pycmf_amd import CMF, HipALSSolver
    X, Y, _, U, V, Z = _planted()
    model = clone(CMF(n_components=3, solver="als", l2_reg=0.05, als_nn_sweeps=4))
    assert model.als_nn_sweeps == 4 and model.get_params()["als_nn_sweeps"] == 4 and model._kwargs()["als_nn_sweeps"] == 4
    assert CMF().als_nn_sweeps == 0
    with pytest.raises(AssertionError, match="device context was opened"):
        model.set_params(x_init="random", y_init="random", random_state=0).fit(X, Y)
    assert HipALSSolver(l2_reg=0.05, nn_sweeps=np.int64(4)).nn_sweeps == 4 and HipALSSolver(l2_reg=0.05).nn_sweeps == 0


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11
    for name, nargs in (("cmf_als_nnls_step", 5), ("cmf_als_nnls_rows", 6)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("als_nnls_step", "als_nnls_rows"))


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    assert b"cmf_als_nnls_step" in blob and b"cmf_als_nnls_rows" in blob and b"als_nnls_kernel" in blob
