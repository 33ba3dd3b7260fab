"""Per-row l2 of the ALS solver, host side: pycmf_amd.l2_multipliers on hand-counted patterns, the yardstick under multipliers
(als_l2rows_yardstick.py) against als_yardstick.py and its own descent, the validation of als_l2_scale before any device is opened,
the option on the estimator, and the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import als_l2rows_yardstick as LR
import als_yardstick as A
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


# ------------------------------------------------------------------ l2_multipliers on hand-counted patterns
def _hand_pattern():
    """X 4 x 5 observed: row 0 holds 3 entries, row 1 none, row 2 two entries of which one is a STORED ZERO weight, row 3 five.
    Column counts of the positive weights: 2, 2, 2, 2, 1."""
    rows = [0, 0, 0, 2, 2, 3, 3, 3, 3, 3]
    cols = [0, 1, 3, 2, 4, 0, 1, 2, 3, 4]
    w = [1.0, 2.0, 0.5, 1.5, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    Wx = sp.csr_matrix((w, (rows, cols)), shape=(4, 5))
    assert Wx.nnz == 10                                       # the zero weight is stored
    return Wx


@pytest.mark.parametrize("nu", [0.0, 0.5, 1.0])
def test_multipliers_of_hand_counted_patterns(nu):
    import pycmf_amd
    Wx = _hand_pattern()
    n_rows, n_cols = np.array([3.0, 0.0, 1.0, 5.0]), np.array([2.0, 2.0, 2.0, 2.0, 1.0])
    # X observed, Y (5 x 3) full: U counts X's rows, V X's columns plus the 3 cells of its row of Y, Z the 5 cells of its column
    mU, mV, mZ = pycmf_amd.l2_multipliers((4, 5), (5, 3), Wx, None, nu=nu)
    assert mU.dtype == mV.dtype == mZ.dtype == np.float64
    assert (mU == np.maximum(n_rows, 1.0) ** nu).all()        # the empty row: the floor at 1
    assert (mV == (n_cols + 3.0) ** nu).all()
    assert (mZ == np.full(3, 5.0) ** nu).all()
    if nu == 0.0:
        assert (mU == 1).all() and (mV == 1).all() and (mZ == 1).all()
    # a background weight 0.25 on X: n + c0 D, D the cells of the row (5) or of the column (4)
    bU, bV, bZ = pycmf_amd.l2_multipliers((4, 5), (5, 3), Wx, None, x_background_weight=0.25, nu=nu)
    assert (bU == np.maximum(n_rows + 0.25 * 5, 1.0) ** nu).all()
    assert (bV == (n_cols + 0.25 * 4 + 3.0) ** nu).all() and (bZ == mZ).all()
    # the same pattern as dense weights and as the solver's resolved weights
    from pycmf_amd.solver_shell import resolve_entry_weights
    for W in (Wx.toarray(), resolve_entry_weights(sp.csr_matrix(np.ones((4, 5))), Wx, "x")):
        dU, dV, _ = pycmf_amd.l2_multipliers((4, 5), (5, 3), W, None, nu=nu)
        assert (dU == mU).all() and (dV == mV).all()
    # Y observed too (its own counts), and a relation that is not there: None for a factor that reads nothing
    Wy = sp.csr_matrix(np.array([[1, 0, 0], [1, 1, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0.0]]))
    oU, oV, oZ = pycmf_amd.l2_multipliers((4, 5), (5, 3), Wx, Wy, nu=nu)
    assert (oU == mU).all() and (oV == np.maximum(n_cols + np.array([1.0, 2, 0, 1, 1]), 1.0) ** nu).all()
    assert (oZ == np.array([4.0, 1.0, 1.0]) ** nu).all()      # an empty column of Y: the floor
    xU, xV, xZ = pycmf_amd.l2_multipliers((4, 5), None, Wx, None, nu=nu)
    assert xZ is None and (xU == mU).all() and (xV == np.maximum(n_cols, 1.0) ** nu).all()
    yU, yV, yZ = pycmf_amd.l2_multipliers(None, (5, 3), None, Wy, nu=nu)
    assert yU is None and (yZ == oZ).all()
    assert "l2_multipliers" in pycmf_amd.__all__


def test_multipliers_refuse_shapes_that_do_not_fit():
    import pycmf_amd
    with pytest.raises(ValueError, match="shape_x"):
        pycmf_amd.l2_multipliers((4, 5), (6, 3), None, None)
    with pytest.raises(ValueError, match="relation of shape"):
        pycmf_amd.l2_multipliers((4, 6), None, _hand_pattern(), None)


# ------------------------------------------------------------------ the yardstick under multipliers
def test_all_ones_are_the_plain_yardstick_with_difference_zero():
    X, Y, Wx, U, V, Z = _planted()
    Wxs = sp.csr_matrix(Wx)
    ones = tuple(np.ones(F.shape[0]) for F in (U, V, Z))
    for kw in (dict(), dict(nn_mask=7, nn_sweeps=4), dict(cg_steps=3)):
        ref = A.step(X, Y, Wxs, None, np.abs(U), np.abs(V), np.abs(Z), 0.05, **kw)
        for mults in (ones, (None, None, None)):
            got = LR.step(X, Y, Wxs, None, np.abs(U), np.abs(V), np.abs(Z), 0.05, mults, **kw)
            assert all(float(np.abs(g - r).max()) == 0.0 for g, r in zip(got, ref)), kw
    assert LR.objective(X, Y, Wxs, None, U, V, Z, 0.05, ones) == pytest.approx(A.objective(X, Y, Wxs, None, U, V, Z, 0.05), rel=1e-14)


def test_a_row_under_a_multiplier_is_the_row_under_the_scaled_scalar():
    X, Y, Wx, U, V, Z = _planted()
    Rx, Ry = A.Relation(X, sp.csr_matrix(Wx)), A.Relation(Y, None)
    rng = np.random.RandomState(1)
    m = rng.choice([0.5, 1.0, 2.0, 4.0], size=U.shape[0])
    got = LR.sweep(Rx, Ry, U, V, Z, "U", 0.5, m)
    for v in (0.5, 1.0, 2.0, 4.0):
        assert (got[m == v] == A.sweep(Rx, Ry, U, V, Z, "U", 0.5 * v)[m == v]).all()
    # and the gradient of the scaled objective vanishes at every swept row
    G = A.gradient(X, Y, sp.csr_matrix(Wx), None, got, V, Z, 0.0, "U") + 0.5 * m[:, None] * got
    assert np.abs(G).max() <= 1e-9 * (np.abs(got).max() + 1)


@pytest.mark.parametrize("route", ["signed exact", "nn_sweeps = 4"])
def test_the_full_objective_descends(route):
    """The planted problem of test_als_host.py, the regulariser with the multipliers max(n, 1)^nu included: 10 iterations, monotone."""
    import pycmf_amd
    X, Y, Wx, U, V, Z = _planted()
    Wxs = sp.csr_matrix(Wx)
    kw = dict() if route == "signed exact" else dict(nn_mask=7, nn_sweeps=4)
    for nu in (0.5, 1.0):
        mults = pycmf_amd.l2_multipliers(X.shape, Y.shape, Wxs, None, nu=nu)
        assert len(np.unique(mults[0])) > 5 and len(np.unique(mults[2])) == 1     # the rows of U differ; Z reads a full relation
        F = (U, V, Z)
        seq = [LR.objective(X, Y, Wxs, None, *F, 0.05, mults)]
        for _ in range(10):
            F = LR.step(X, Y, Wxs, None, *F, 0.05, mults, **kw)
            seq.append(LR.objective(X, Y, Wxs, None, *F, 0.05, mults))
        print("%s, nu %.1f: %s" % (route, nu, " ".join("%.3f" % s for s in seq)))
        assert all(b <= a * (1 + 1e-12) for a, b in zip(seq, seq[1:])), seq
        assert seq[-1] < 0.5 * seq[0]
        if kw:
            assert min(f.min() for f in F) >= 0


# ------------------------------------------------------------------ validation before any device is opened
@pytest.mark.parametrize("kw, match", [(dict(als_l2_scale=1.5), r"als_l2_scale must be a number in \[0, 1\]"),
                                       (dict(als_l2_scale=-0.1), r"als_l2_scale must be a number in \[0, 1\]"),
                                       (dict(als_l2_scale=float("nan")), r"als_l2_scale must be a number in \[0, 1\]"),
                                       (dict(als_l2_scale=True), r"als_l2_scale must be a number in \[0, 1\]"),
                                       (dict(als_l2_scale="1"), r"als_l2_scale must be a number in \[0, 1\]"),
                                       (dict(als_l2_scale=0.5, solver="mu"), "must be 0 with solver='mu'"),
                                       (dict(als_l2_scale=0.5, solver="hals"), "must be 0 with solver='hals'"),
                                       (dict(als_l2_scale=0.5, n_gpus=2), "n_gpus must be 1")])
def test_bad_values_are_refused_before_a_device_is_touched(no_device, kw, match):
    from pycmf_amd import CMF
    X, Y, Wx, U, V, Z = _planted()
    kw = dict(dict(solver="als"), **kw)
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, l2_reg=0.05, x_init="random", y_init="random", random_state=0, **kw).fit(np.abs(X), np.abs(Y))


def test_solver_object_validates_too_and_good_values_reach_the_device(no_device):
    from pycmf_amd import CMF, HipALSSolver
    from pycmf_amd.solver_shell import check_als_l2_scale
    with pytest.raises(ValueError, match=r"number in \[0, 1\]"):
        HipALSSolver(l2_reg=0.1, l2_scale=2)
    with pytest.raises(ValueError, match=r"number in \[0, 1\]"):
        HipALSSolver(l2_reg=0.1, l2_scale=np.bool_(True))
    assert HipALSSolver(l2_reg=0.1).l2_scale == 0.0 and HipALSSolver(l2_reg=0.1, l2_scale=1).l2_scale == 1.0
    assert HipALSSolver(l2_reg=0.1, l2_scale=np.float32(0.5)).l2_multipliers is None
    assert check_als_l2_scale(0, "mu", 4) == 0.0 and check_als_l2_scale(0.0, "newton") == 0.0     # off: any solver
    X, Y, Wx, U, V, Z = _planted()
    # it composes with the other ALS keywords: nothing is refused, the fit goes on to the device
    for extra in (dict(), dict(als_nn_sweeps=4), dict(als_cg_steps=3, U_non_negative=False), dict(als_nn_cg_steps=3), dict(als_dual_max=64)):
        with pytest.raises(AssertionError, match="device context was opened"):
            CMF(n_components=3, solver="als", l2_reg=0.05, als_l2_scale=0.5, x_init="random", y_init="random", random_state=0,
                **extra).fit(np.abs(X), np.abs(Y), x_entry_weights=sp.csr_matrix(Wx))


def test_the_option_outside_get_params_survives_clone_set_params_and_repr(no_device):
    from sklearn.base import clone
    from pycmf_amd import CMF
    assert CMF().als_l2_scale == 0.0 and "als_l2_scale" not in CMF(als_l2_scale=0.5).get_params()
    assert CMF(solver="als", l2_reg=0.05).get_params() == CMF(solver="als", l2_reg=0.05, als_l2_scale=0.5).get_params()
    assert vars(CMF(solver="als")) == vars(CMF(solver="als", als_l2_scale=0.0))
    with pytest.raises(TypeError, match="unexpected keyword argument 'als_l2_scales'"):
        CMF(als_l2_scales=0.5)
    first = CMF(n_components=3, solver="als", l2_reg=0.05, als_l2_scale=0.5)
    model = clone(first)
    assert model is not first and model.als_l2_scale == 0.5 and model._kwargs()["als_l2_scale"] == 0.5
    assert model.get_params() == first.get_params() and clone(clone(model)).als_l2_scale == 0.5
    assert model.set_params(als_l2_scale=1.0, max_iter=7) is model and (model.als_l2_scale, model.max_iter) == (1.0, 7)
    assert clone(CMF(n_components=3)).als_l2_scale == 0.0 and "als_l2_scale" not in repr(CMF(n_components=3))
    assert repr(model).endswith(", als_l2_scale=1.0)") and repr(CMF(als_l2_scale=0.5)) == "CMF(als_l2_scale=0.5)"
    both = CMF(als_dual_max=5, als_l2_scale=0.25)
    assert repr(both) == "CMF(als_dual_max=5, als_l2_scale=0.25)" and (clone(both).als_dual_max, clone(both).als_l2_scale) == (5, 0.25)
    with pytest.raises(ValueError, match=r"number in \[0, 1\]"):
        clone(model).set_params(als_l2_scale=3).fit(np.ones((4, 4)), np.ones((4, 4)))


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    for name, nargs in (("cmf_set_l2_rows", 3), ("cmf_get_l2_rows", 4)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("set_l2_rows", "get_l2_rows"))
    text = header[header.index("a per-row l2"):header.index("int cmf_set_l2_rows")]
    assert "ONE" in text and "bias_l2 UNSCALED" in text and "MU, HALS and Newton" in text and "CMF_EUNSUPPORTED" in text


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    assert b"cmf_set_l2_rows" in blob and b"cmf_get_l2_rows" in blob
