"""Conjugate-gradient row solve of the ALS solver, host side: the NumPy yardstick (als_yardstick.py) against its own exact solves,
the planted problem of the documentation, keyword validation before any device is opened, the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
from test_gpu_wmu import fit_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCUMENTED_STEPS = 6
L2 = 0.05


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _planted():
    X, Y, Wx, _, U, V, Z = fit_inputs(3, m=120, d=150, p=20, k=12, obs=.5)
    return X, Y, Wx, U, V, Z


SIGNED = dict(U_non_negative=False, V_non_negative=False, Z_non_negative=False)


# ------------------------------------------------------------------ the yardstick
def test_k_steps_are_the_exact_solve():
    """k = 7: CG on a 7 x 7 positive definite system ends after 7 steps.  All three sweeps of a signed random problem, X observed
    (rows with fewer and with more than k entries, non-unit weights), Y observed for V (two sides) and full for V (S and N):
    within 1e-10 relative of np.linalg.solve on als_yardstick.systems."""
    rng = np.random.RandomState(5)
    m, d, p, k = 40, 60, 9, 7
    X, Y = rng.randn(m, d), rng.randn(d, p)
    Wx = sp.csr_matrix((0.25 + 3.75 * rng.rand(m, d)) * (rng.rand(m, d) < rng.uniform(0.05, 0.4, size=(m, 1))))
    Wy = sp.csr_matrix((0.25 + 3.75 * rng.rand(d, p)) * (rng.rand(d, p) < 0.5))
    U, V, Z = (rng.randn(n, k) for n in (m, d, p))
    worst = 0.0
    for wy in (Wy, None):
        Rx, Ry = A.Relation(X, Wx), A.Relation(Y, wy)
        for which in "UVZ":
            if not A.observed(Rx, Ry, which):
                continue
            H, g = A.systems(Rx, Ry, U, V, Z, which, 0.1)
            ref = np.linalg.solve(H, g[:, :, None])[:, :, 0]
            got = A.sweep(Rx, Ry, U, V, Z, which, 0.1, cg_steps=k)
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    print("7 CG steps against the exact solve: worst relative difference %.2e" % worst)
    assert worst <= 1e-10


def test_planted_problem_descends_for_every_step_count_and_the_documented_count_is_close_to_exact_als():
    """Planted problem, 120 x 150 with 50 % of X observed, Y unweighted, k = 12, l2 = 0.05, signed factors, 20 iterations
    (float64): the objective never rises for 1, 2, 3, 4 and 6 steps, and the documented 6 steps end within 2 % of exact ALS
    (measured: exact 50.46; 1 step 144.70, 2 steps 60.84, 3 steps 55.29, 4 steps 51.45 -- 1.96 % above, too close to the bound to
    document --, 6 steps 50.05)."""
    X, Y, Wx, U, V, Z = _planted()
    Ws = sp.csr_matrix(Wx)
    start = A.objective(X, Y, Wx, None, U, V, Z, L2)
    Ur, Vr, Zr, _, _ = A.fit(X, Y, Ws, None, U, V, Z, 20, L2)
    exact = A.objective(X, Y, Wx, None, Ur, Vr, Zr, L2)
    last = {}
    for steps in (1, 2, 3, 4, 6):
        trace = []
        A.fit(X, Y, Ws, None, U, V, Z, 20, L2, cg_steps=steps, trace=trace)
        seq = [start] + trace
        assert len(trace) == 20 and all(b <= a * (1 + 1e-12) for a, b in zip(seq, seq[1:])), (steps, seq)
        last[steps] = trace[-1]
    print("objective after 20 iterations: exact ALS %.2f; CG %s" % (exact, ", ".join("%d steps %.2f" % kv for kv in sorted(last.items()))))
    assert last[DOCUMENTED_STEPS] <= 1.02 * exact
    assert last[1] > last[2] > last[3] > last[4] > last[DOCUMENTED_STEPS]


def test_rows_without_information_become_zeros_and_other_routes_are_kept():
    X, Y, Wx, U, V, Z = _planted()
    Wx = Wx.copy()
    Wx[7] = 0
    Ws = sp.csr_matrix(Wx)
    Un, _, _ = A.step(X, Y, Ws, None, U, V, Z, L2, cg_steps=4, mask=A.U_BIT)
    assert (Un[7] == 0).all() and (np.abs(Un).sum(axis=1) > 0).sum() == len(Un) - 1
    # Z has no observed relation here: the exact solve; a factor in nn_mask: the projection, or coordinate descent
    assert (A.step(X, Y, Ws, None, U, V, Z, L2, cg_steps=4, mask=A.Z_BIT)[2] == A.step(X, Y, Ws, None, U, V, Z, L2, mask=A.Z_BIT)[2]).all()
    assert (A.step(X, Y, Ws, None, U, V, Z, L2, cg_steps=4, mask=A.U_BIT, nn_mask=A.U_BIT)[0]
            == A.step(X, Y, Ws, None, U, V, Z, L2, mask=A.U_BIT, nn_mask=A.U_BIT)[0]).all()
    assert (A.step(X, Y, Ws, None, U, V, Z, L2, cg_steps=4, mask=A.U_BIT, nn_mask=A.U_BIT, nn_sweeps=2)[0]
            == A.step(X, Y, Ws, None, U, V, Z, L2, nn_sweeps=2, mask=A.U_BIT, nn_mask=A.U_BIT)[0]).all()


# ------------------------------------------------------------------ validation before any device is opened
@pytest.mark.parametrize("value", [-1, 1025, 2.0, "4", None, True])
def test_bad_step_counts_are_refused_before_a_device_is_touched(no_device, value):
    from pycmf_amd import CMF, HipALSSolver
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_cg_steps must be an integer 0 .. 1024"):
        CMF(n_components=3, solver="als", l2_reg=0.05, x_init="random", y_init="random", random_state=0, als_cg_steps=value, **SIGNED).fit(X, Y)
    with pytest.raises(ValueError, match="als_cg_steps must be an integer 0 .. 1024"):
        HipALSSolver(l2_reg=0.05, cg_steps=value)


@pytest.mark.parametrize("solver", ["mu", "hals", "newton"])
def test_other_solvers_refuse_the_keyword(no_device, solver):
    from pycmf_amd import CMF
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_cg_steps is the conjugate-gradient row solve of solver='als'"):
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, als_cg_steps=4).fit(X, Y)
    with pytest.raises(AssertionError, match="device context was opened"):        # 0 is every solver's default: the fit goes on
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, als_cg_steps=0).fit(X, Y)


def test_all_non_negative_factors_refuse_the_keyword(no_device):
    """*_non_negative=True is the default: CG would have nothing to act on and the keyword would silently do nothing."""
    from pycmf_amd import CMF
    X, Y, _, U, V, Z = _planted()
    kw = dict(n_components=3, solver="als", l2_reg=0.05, x_init="random", y_init="random", random_state=0, als_cg_steps=4)
    with pytest.raises(ValueError, match="acts on signed factors only"):
        CMF(**kw).fit(X, Y)
    with pytest.raises(AssertionError, match="device context was opened"):        # one signed factor is enough
        CMF(V_non_negative=False, **kw).fit(X, Y)
    with pytest.raises(AssertionError, match="device context was opened"):        # and 0 asks for nothing
        CMF(**dict(kw, als_cg_steps=0)).fit(X, Y)


def test_good_keyword_reaches_the_solver_and_survives_clone(no_device):
    from sklearn.base import clone
    from pycmf_amd import CMF, HipALSSolver
    X, Y, _, U, V, Z = _planted()
    model = clone(CMF(n_components=3, solver="als", l2_reg=0.05, als_cg_steps=4, **SIGNED))
    assert model.als_cg_steps == 4 and model.get_params()["als_cg_steps"] == 4 and model._kwargs()["als_cg_steps"] == 4
    assert CMF().als_cg_steps == 0
    with pytest.raises(AssertionError, match="device context was opened"):
        model.set_params(x_init="random", y_init="random", random_state=0).fit(X, Y)
    solver = HipALSSolver(l2_reg=0.05, cg_steps=np.int64(4), nn_sweeps=2)
    assert solver.cg_steps == 4 and solver.nn_sweeps == 2 and HipALSSolver(l2_reg=0.05).cg_steps == 0


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11
    for name, nargs in (("cmf_als_cg_step", 6), ("cmf_als_cg_rows", 7)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("als_cg_step", "als_cg_rows"))


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    assert b"cmf_als_cg_step" in blob and b"cmf_als_cg_rows" in blob and b"als_cg_kernel" in blob
