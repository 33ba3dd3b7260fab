"""ALS solver, host side: the NumPy yardstick (als_yardstick.py) against closed forms and its own optimality conditions, the planted
problem of the documentation against the weighted MU yardstick, keyword validation before any device is opened, the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
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


def _problem(seed=3, m=23, d=17, p=11, k=6):
    rng = np.random.RandomState(seed)
    X, Y = rng.randn(m, d), rng.randn(d, p)
    U, V, Z = (rng.randn(n, k) for n in (m, d, p))
    return X, Y, U, V, Z


def _planted():
    X, Y, Wx, _, U, V, Z = fit_inputs(3, m=120, d=150, p=20, k=3, obs=.3)
    return X, Y, Wx, U, V, Z


# ------------------------------------------------------------------ the yardstick
def test_unweighted_sweeps_are_the_closed_form():
    """Fully observed, unweighted, signed: F = (T B)(B^T B + l2 I)^-1 per sweep, the new V used for U and Z."""
    X, Y, U, V, Z = _problem()
    l2, k = 0.3, U.shape[1]
    Un, Vn, Zn = A.step(X, Y, None, None, U, V, Z, l2)
    Vc = (X.T @ U + Y @ Z) @ np.linalg.inv(U.T @ U + Z.T @ Z + l2 * np.eye(k))
    Uc = (X @ Vc) @ np.linalg.inv(Vc.T @ Vc + l2 * np.eye(k))
    Zc = (Y.T @ Vc) @ np.linalg.inv(Vc.T @ Vc + l2 * np.eye(k))
    for got, ref in ((Un, Uc), (Vn, Vc), (Zn, Zc)):
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # the same data as sparse matrices and under weights of ones (dense and as a full pattern): the same sweeps
    for Xs, Ys, Wx, Wy in ((sp.csr_matrix(X), sp.csr_matrix(Y), None, None), (X, Y, np.ones(X.shape), sp.csr_matrix(np.ones(Y.shape)))):
        for got, ref in zip(A.step(Xs, Ys, Wx, Wy, U, V, Z, l2), (Uc, Vc, Zc)):
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("config", ["csr/none", "none/csr", "csr/csr", "dense/none"])
def test_every_swept_row_has_zero_gradient(config):
    """Observed sides with non-unit weights, an empty row and an empty column: after the sweep of a factor the gradient of the
    objective with respect to each of its rows vanishes (relative to the size of its two terms)."""
    X, Y, U, V, Z = _problem(seed=5, m=31, d=27, p=13, k=7)
    rng = np.random.RandomState(9)

    def weights(shape, kind):
        if kind == "none":
            return None
        W = (0.25 + 3.75 * rng.rand(*shape)) * (rng.rand(*shape) < 0.35)
        W[shape[0] // 4] = 0
        W[:, shape[1] // 3] = 0
        return sp.csr_matrix(W) if kind == "csr" else W
    kx, ky = config.split("/")
    Wx, Wy = weights(X.shape, kx), weights(Y.shape, ky)
    l2 = 0.05
    F = dict(U=U, V=V, Z=Z)
    for which, bit in (("V", A.V_BIT), ("U", A.U_BIT), ("Z", A.Z_BIT)):
        Un, Vn, Zn = A.step(X, Y, Wx, Wy, F["U"], F["V"], F["Z"], l2, mask=bit)
        F = dict(U=Un, V=Vn, Z=Zn)
        G = A.gradient(X, Y, Wx, Wy, Un, Vn, Zn, l2, which)
        H, g = A.systems(A.Relation(X, Wx), A.Relation(Y, Wy), Un, Vn, Zn, which, l2)
        scale = np.abs(np.einsum("nij,nj->ni", H, F[which])).max() + np.abs(g).max()
        assert np.abs(G).max() <= 1e-10 * scale, (config, which)
    if kx != "none":                                        # a row of U without observations solves to exact zeros
        assert (F["U"][X.shape[0] // 4] == 0).all()


def test_objective_descends_and_beats_300_mu_iterations_on_the_planted_problem():
    """Planted rank 3, 120 x 150, 30 % of X observed, Y unweighted, l2 = 0.05, signed factors: monotone descent over 10 iterations,
    and the objective after them below 0.95 x the weighted MU yardstick's after 300 (float64: 39.64 against 44.15)."""
    X, Y, Wx, U, V, Z = _planted()
    l2 = 0.05
    trace = []
    Ua, Va, Za, n, _ = A.fit(X, Y, sp.csr_matrix(Wx), None, U, V, Z, 10, l2, trace=trace)
    assert n == 10 and len(trace) == 10
    start = A.objective(X, Y, Wx, None, U, V, Z, l2)
    seq = [start] + trace
    assert all(b <= a * (1 + 1e-12) for a, b in zip(seq, seq[1:])), seq
    Um, Vm, Zm, _, _ = WM.fit(X, Y, Wx, None, U, V, Z, 300, 0, l2=l2)
    mu = WM.objective(X, Y, Wx, None, Um, Vm, Zm, l2=l2)
    assert abs(mu - A.objective(X, Y, Wx, None, Um, Vm, Zm, l2)) <= 1e-9 * mu      # the two yardsticks agree on the objective
    unobserved = Wx == 0
    rmse = [float(np.sqrt((((X - P @ Q.T) ** 2)[unobserved]).mean())) for P, Q in ((Ua, Va), (Um, Vm))]
    print("objective: start %.1f, ALS %s; MU after 300: %.2f; RMSE on the unobserved cells: ALS %.4f, MU %.4f"
          % (start, " ".join("%.2f" % t for t in trace), mu, rmse[0], rmse[1]))
    assert trace[-1] < 0.95 * mu
    assert rmse[0] < rmse[1]
    # the non-negative projection is honoured and is weaker (documented): every factor >= 0, a larger objective
    Up, Vp, Zp, _, _ = A.fit(X, Y, Wx, None, U, V, Z, 10, l2, nn_mask=7)
    assert min(Up.min(), Vp.min(), Zp.min()) >= 0 and A.objective(X, Y, Wx, None, Up, Vp, Zp, l2) > trace[-1]


def test_float32_yardstick_prices_the_tolerance():
    """The tolerance rule has teeth: one float32 step is within 1e-4 of the float64 one relative to the largest entry (issue's
    table: 3e-6 .. 4.3e-5 at these shapes), so the device bound is a few 1e-4 at most."""
    rng = np.random.RandomState(0)
    m, d, p, k = 70, 333, 129, 40
    X, Y = rng.randn(m, d), rng.randn(d, p)
    U, V, Z = (np.float32(rng.randn(n, k)).astype(np.float64) for n in (m, d, p))
    Wx = sp.csr_matrix((rng.rand(m, d) < 0.05).astype(float))
    y64 = A.step(X, Y, Wx, None, U, V, Z, 0.1)
    y32 = A.step(X, Y, Wx, None, U, V, Z, 0.1, dtype=np.float32)
    for a, b in zip(y32, y64):
        assert a.dtype == np.float32 and np.abs(a - b).max() <= 1e-4 * np.abs(b).max()
        assert A.tolerance(a, b, k) <= 4e-4 * np.abs(b).max()


def test_route_truth_table():
    """Every combination of the facts of a sweep and the options of a step: 2 observed x 2 non-negative x {0, > 0}^4 options x
    shared term x logistic x k_pad in {32, 64}.  The precedence is the device's (als_route): the non-negative CG rows before
    nn_sweeps on a non-negative observed factor; CG only on a signed observed factor; the dual rows only where the exact rows would
    run, with no shared term, no logistic relation and k_pad > 32; a sweep without an observed relation never leaves the shared
    routes; and with the new options at zero the answer is the one of the four old arguments.  This pins the Python mirror
    (als_yardstick.route), which the float64 references are routed by, not the device's als_route: the device's table is held to it
    by the GPU tests that compare each route with its reference and by test_gpu_als_dispatch.py."""
    import itertools
    seen = set()
    for obs, nn, s, c, n, dm, shared, logit, kp in itertools.product((False, True), (False, True), (0, 2), (0, 3), (0, 4), (0, 128),
                                                                        (False, True), (False, True), (32, 64)):
        got = A.route(obs, nn, s, c, n, dm, shared, logit, kp)
        seen.add(got)
        if not obs:
            want = A.SHARED_HALS if nn and s else A.SHARED_EXACT
        elif nn and n:
            want = A.ROWS_NNCG
        elif nn and s:
            want = A.ROWS_NNLS
        elif not nn and c:
            want = A.ROWS_CG
        elif dm and not shared and not logit and kp > 32:
            want = A.ROWS_DUAL
        else:
            want = A.ROWS_EXACT
        assert got == want, (obs, nn, s, c, n, dm, shared, logit, kp)
        assert (got == A.ROWS_NNCG) == (obs and nn and n > 0)
        assert (got == A.ROWS_CG) == (obs and not nn and c > 0)
        if got == A.ROWS_DUAL:                                # only where the exact rows would run otherwise
            assert A.route(obs, nn, s, c, n, 0, shared, logit, kp) == A.ROWS_EXACT and not shared and not logit and kp > 32
        if n == 0 and dm == 0:                                # the old callers, arguments unchanged
            assert got == A.route(obs, nn, s, c)
    assert seen == {A.SHARED_EXACT, A.SHARED_HALS, A.ROWS_EXACT, A.ROWS_NNLS, A.ROWS_CG, A.ROWS_NNCG, A.ROWS_DUAL}


# ------------------------------------------------------------------ validation before any device is opened
@pytest.mark.parametrize("kw, match", [(dict(l2_reg=0.0), "l2_reg > 0"), (dict(l2_reg=0.1, l1_reg=0.01), "l1_reg must be 0"),
                                       (dict(l2_reg=0.1, n_gpus=2), "n_gpus must be 1"),
                                       (dict(l2_reg=0.1, loss="kullback-leibler"), "kullback-leibler")])
def test_bad_keywords_are_refused_before_a_device_is_touched(no_device, kw, match):
    from pycmf_amd import CMF
    X, Y, U, V, Z = _problem()
    with pytest.raises(ValueError, match=match):
        CMF(n_components=3, solver="als", x_init="random", y_init="random", random_state=0, **kw).fit(np.abs(X), np.abs(Y))


def test_solver_object_validates_too(no_device):
    from pycmf_amd import HipALSSolver
    with pytest.raises(ValueError, match="l2_reg > 0"):
        HipALSSolver()
    with pytest.raises(ValueError, match="l1_reg must be 0"):
        HipALSSolver(l1_reg=0.1, l2_reg=0.1)
    s = HipALSSolver(l2_reg=0.1, U_non_negative=False, x_entry_weights="observed")
    assert s._run_params() is None and s._nn_mask() == 6 and s._update_mask() == 7


def test_more_than_256_components_are_refused(no_device):
    from pycmf_amd import CMF
    rng = np.random.RandomState(0)
    X, Y = rng.randn(300, 280), rng.randn(280, 270)
    with pytest.raises(NotImplementedError, match="n_components <= 256"):
        CMF(n_components=257, solver="als", l2_reg=0.1, x_init="random", y_init="random", random_state=0).fit(X, Y)


def test_entry_weights_are_admitted_and_validated_on_the_host(no_device):
    from pycmf_amd import CMF
    X, Y = (np.abs(M) for M in _problem()[:2])
    model = CMF(n_components=3, solver="als", l2_reg=0.1, x_init="random", y_init="random", random_state=0)
    with pytest.raises(ValueError, match="must be non-negative"):
        model.fit(X, Y, x_entry_weights=-np.ones(X.shape))
    with pytest.raises(AssertionError, match="device context was opened"):      # good weights: the fit goes on to the device
        model.fit(X, Y, x_entry_weights=(np.abs(X) > 0.5).astype(float))
    with pytest.raises(ValueError, match="No such solver: als2"):
        CMF(n_components=3, solver="als2").fit(X, Y)


def test_dense_weights_become_the_pattern_of_their_non_zeros():
    from pycmf_amd.solver_shell import HipALSSolver
    X, Y, U, V, Z = _problem()
    W = (np.abs(X) > 0.7) * 2.5
    s = HipALSSolver(l2_reg=0.1, x_entry_weights=W)
    ew, none = s._resolve_weights(X, Y)
    assert none is None and ew.kind == "csr" and ew.indptr[-1] == int((W != 0).sum())
    r = np.repeat(np.arange(X.shape[0]), np.diff(ew.indptr))
    assert (ew.w == 2.5).all() and (ew.t == X[r, ew.indices]).all() and (W[r, ew.indices] != 0).all()


def test_clone_keeps_the_solver():
    from sklearn.base import clone
    from pycmf_amd import CMF
    model = clone(CMF(n_components=4, solver="als", l2_reg=0.05, U_non_negative=False))
    assert model.solver == "als" and model.l2_reg == 0.05 and model.U_non_negative is False


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared_and_the_class_enums_stay():
    import pycmf_amd
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11 and enum["CMF_K_END"] == enum["CMF_K_HALS"] + 1 == 12
    for name, nargs in (("cmf_als_step", 4), ("cmf_als_normal", 7), ("cmf_als_layout", 2)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("als_step", "als_normal", "als_layout"))
    assert "HipALSSolver" in pycmf_amd.__all__ and callable(pycmf_amd.HipALSSolver)
    text = header[header.index("ALS solver"):header.index("int cmf_als_step")]
    assert "SIGNED FACTORS" in text and "cmf_hals_step" in text and "cmf_mu_step" in text


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    assert b"cmf_als_step" in blob and b"cmf_als_normal" in blob and b"cmf_als_layout" in blob and b"als_normal_kernel" in blob
