"""ALS with a background weight (implicit feedback), host side: the structured yardstick (als_yardstick.py with cx / cy) against the
dense weighted problem it is equal to, its optimality conditions, the planted click problem of the documentation, keyword
validation before any device is opened, the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
import click_problem as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _problem(seed=5, m=31, d=27, p=13, k=7):
    rng = np.random.RandomState(seed)
    X, Y = rng.randn(m, d), rng.randn(d, p)
    U, V, Z = (np.abs(rng.randn(n, k)) for n in (m, d, p))
    return X, Y, U, V, Z


def _weights(rng, shape, floor):
    """CSR weights >= floor on 35 % of the cells, with an empty row and an empty column."""
    W = (floor + 3.75 * rng.rand(*shape)) * (rng.rand(*shape) < 0.35)
    W[shape[0] // 4] = 0
    W[:, shape[1] // 3] = 0
    return sp.csr_matrix(W)


# (cx, cy, Y observed?): X with a background beside an observed Y without one, both with backgrounds, X with a background beside full Y
CONFIGS = {"x": (0.5, 0.0, True), "both": (0.5, 0.25, True), "x+fullY": (0.5, 0.0, False)}


def _config(name):
    cx, cy, y_obs = CONFIGS[name]
    X, Y, U, V, Z = _problem()
    rng = np.random.RandomState(9)
    Wx = _weights(rng, X.shape, cx)
    Wy = _weights(rng, Y.shape, max(cy, 0.25)) if y_obs else None
    Dx, Wdx = A.dense_equivalent(X, Wx, cx)
    Dy, Wdy = A.dense_equivalent(Y, Wy, cy) if cy else (Y, Wy)
    return (X, Y, Wx, Wy, cx, cy), (Dx, Dy, Wdx, Wdy), (U, V, Z)


# ------------------------------------------------------------------ the structured form is the dense weighted problem
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_structured_step_equals_the_dense_equivalent(config):
    """One step of each route -- exact, 4 coordinate-descent sweeps, 3 CG steps -- equals the same step without a background
    fed c0 everywhere / w on the pattern / data 0 off it, to 1e-10 of the largest entry.  An empty row and an empty column included."""
    (X, Y, Wx, Wy, cx, cy), (Dx, Dy, Wdx, Wdy), (U, V, Z) = _config(config)
    l2 = 0.05
    assert (np.diff(Wx.indptr) == 0).any() and (np.diff(Wx.tocsc().indptr) == 0).any()
    cases = (("exact", A.step(X, Y, Wx, Wy, U, V, Z, l2, cx=cx, cy=cy), A.step(Dx, Dy, Wdx, Wdy, U, V, Z, l2)),
             ("nnls", A.step(X, Y, Wx, Wy, U, V, Z, l2, cx=cx, cy=cy, nn_mask=7, nn_sweeps=4), A.step(Dx, Dy, Wdx, Wdy, U, V, Z, l2, nn_mask=7, nn_sweeps=4)),
             ("cg", A.step(X, Y, Wx, Wy, U, V, Z, l2, cx=cx, cy=cy, cg_steps=3), A.step(Dx, Dy, Wdx, Wdy, U, V, Z, l2, cg_steps=3)))
    for route, got, ref in cases:
        for name, a, b in zip("UVZ", got, ref):
            err = np.abs(a - b).max() / np.abs(b).max()
            print("%s %s %s: %.2e" % (config, route, name, err))
            assert err <= 1e-10, (config, route, name)
    # the error and the objective are the dense ones too
    Un, Vn, Zn = cases[0][1]
    for a, b in zip(A.errors(X, Y, Wx, Wy, Un, Vn, Zn, cx=cx, cy=cy), A.errors(Dx, Dy, Wdx, Wdy, Un, Vn, Zn)):
        assert abs(a - b) <= 1e-10 * b
    assert abs(A.objective(X, Y, Wx, Wy, Un, Vn, Zn, l2, cx=cx, cy=cy) - A.objective(Dx, Dy, Wdx, Wdy, Un, Vn, Zn, l2)) <= 1e-10 * A.objective(Dx, Dy, Wdx, Wdy, Un, Vn, Zn, l2)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_every_swept_row_has_zero_gradient_of_the_dense_objective(config):
    """After the exact sweep of a factor the gradient of the dense-equivalent objective with respect to each of its rows vanishes
    (relative to the size of its two terms, the scale of test_als_host.py)."""
    (X, Y, Wx, Wy, cx, cy), (Dx, Dy, Wdx, Wdy), (U, V, Z) = _config(config)
    l2 = 0.05
    F = dict(U=U, V=V, Z=Z)
    for which, bit in (("V", A.V_BIT), ("U", A.U_BIT), ("Z", A.Z_BIT)):
        Un, Vn, Zn = A.step(X, Y, Wx, Wy, F["U"], F["V"], F["Z"], l2, cx=cx, cy=cy, mask=bit)
        F = dict(U=Un, V=Vn, Z=Zn)
        G = A.gradient(Dx, Dy, Wdx, Wdy, Un, Vn, Zn, l2, which)
        H, g = A.systems(A.Relation(Dx, Wdx), A.Relation(Dy, Wdy), Un, Vn, Zn, which, l2)
        scale = np.abs(np.einsum("nij,nj->ni", H, F[which])).max() + np.abs(g).max()
        assert np.abs(G).max() <= 1e-10 * scale, (config, which)
    # a row of U without stored entries: an ordinary row -- exact zeros, because nothing enters its right-hand side
    assert (F["U"][X.shape[0] // 4] == 0).all()


def test_systems_of_a_row_without_entries():
    (X, Y, Wx, Wy, cx, cy), _, (U, V, Z) = _config("x")
    i = X.shape[0] // 4
    H, g = A.systems(A.Relation(X, Wx), A.Relation(Y, Wy), U, V, Z, "U", 0.05, cx=cx, cy=cy, rows=[i])
    assert (g == 0).all() and np.abs(H[0] - (cx * V.T @ V + 0.05 * np.eye(V.shape[1]))).max() <= 1e-13 * np.abs(H).max()


# ------------------------------------------------------------------ the planted click problem
def _click_fits(seed):
    counts, train, test, Y, U0, V0, Z0 = K.clicks(seed)
    P, W = K.click_relations(counts, train)
    ones = sp.csr_matrix(train.astype(np.float64))
    trace = []
    U, V, Z, _, _ = A.fit(P, Y, W, None, U0, V0, Z0, 15, 2.0, cx=1.0, trace=trace)
    start = A.objective(P, Y, W, None, U0, V0, Z0, 2.0, cx=1.0)
    rec = {"background": K.recall_at(U @ V.T, train, test)}
    U, V, Z, _, _ = A.fit(P, Y, ones, None, U0, V0, Z0, 15, 2.0, cx=1.0)
    rec["zeros as data"] = K.recall_at(U @ V.T, train, test)
    U, V, Z, _, _ = A.fit(P, Y, ones, None, U0, V0, Z0, 15, 2.0)
    rec["observed only"] = K.recall_at(U @ V.T, train, test)
    rec["popularity"] = K.recall_at(np.broadcast_to(train.sum(axis=0)[None].astype(np.float64), train.shape), train, test)
    return rec, [start] + trace


def test_planted_clicks_background_weight_beats_the_alternatives():
    """120 x 150, 8 % clicks, a quarter held out, k = 8, l2 = 2, c0 = 1, w = 1 + count, signed factors, 15 iterations, seeds 3 / 5 / 7:
    the objective never rises, and recall@10 on the held-out clicks exceeds 1.3 x the larger of the observed-only fit and
    popularity, and 1.3 x the fit with w = c0 = 1 (measured worst ratio 1.71: seed 7 against popularity)."""
    rows = ("background", "zeros as data", "observed only", "popularity")
    table = {}
    for seed in (3, 5, 7):
        rec, seq = _click_fits(seed)
        table[seed] = rec
        assert all(b <= a * (1 + 1e-12) for a, b in zip(seq, seq[1:])), (seed, seq)
    print("recall@10        " + "  ".join("seed %d" % s for s in table))
    for r in rows:
        print("%-16s " % r + "  ".join("%.3f " % table[s][r] for s in table))
    worst = min(table[s]["background"] / max(table[s][r] for r in rows[1:]) for s in table)
    print("worst ratio %.2f" % worst)
    for seed, rec in table.items():
        assert rec["background"] > 1.3 * max(rec["observed only"], rec["popularity"]), (seed, rec)
        assert rec["background"] > 1.3 * rec["zeros as data"], (seed, rec)


# ------------------------------------------------------------------ validation before any device is opened
def _fit_args():
    X, Y = (np.abs(M) for M in _problem()[:2])
    W = sp.csr_matrix((X > 0.5) * (1.0 + X))
    return X, Y, W


@pytest.mark.parametrize("solver", ["mu", "hals", "newton"])
def test_background_needs_the_als_solver(no_device, solver):
    from pycmf_amd import CMF
    X, Y, W = _fit_args()
    kw = dict(l2_reg=0.1) if solver != "hals" else {}
    with pytest.raises(ValueError, match="x_background_weight is the implicit-feedback model of solver='als'"):
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, **kw).fit(
            X, Y, x_entry_weights=(W if solver == "mu" else None), x_background_weight=1.0)


@pytest.mark.parametrize("value", [True, np.nan, np.inf, -0.5, "1", None])
def test_bad_background_values_are_refused(no_device, value):
    from pycmf_amd import CMF, HipALSSolver
    X, Y, W = _fit_args()
    model = CMF(n_components=3, solver="als", l2_reg=0.1, x_init="random", y_init="random", random_state=0)
    with pytest.raises(ValueError, match="x_background_weight must be a finite number >= 0"):
        model.fit(X, Y, x_entry_weights=W, x_background_weight=value)
    with pytest.raises(ValueError, match="y_background_weight must be a finite number >= 0"):
        model.fit_transform(X, Y, y_entry_weights=sp.csr_matrix(Y), y_background_weight=value)
    with pytest.raises(ValueError, match="y_background_weight must be a finite number >= 0"):
        HipALSSolver(l2_reg=0.1, y_entry_weights="observed", y_background_weight=value)


def test_background_needs_sparse_entry_weights(no_device):
    from pycmf_amd import CMF, HipALSSolver, collective_matrix_factorization
    X, Y, W = _fit_args()
    model = CMF(n_components=3, solver="als", l2_reg=0.1, x_init="random", y_init="random", random_state=0)
    with pytest.raises(ValueError, match="x_background_weight=1.0 needs x_entry_weights"):
        model.fit(X, Y, x_background_weight=1.0)
    with pytest.raises(ValueError, match="y_background_weight=0.5 needs y_entry_weights"):
        model.fit(X, Y, x_entry_weights=W, y_background_weight=0.5)
    with pytest.raises(ValueError, match="pass a SciPy sparse W or 'observed'"):
        model.fit(X, Y, x_entry_weights=W.toarray(), x_background_weight=1.0)
    with pytest.raises(ValueError, match="pass a SciPy sparse W or 'observed'"):
        HipALSSolver(l2_reg=0.1, x_entry_weights=W.toarray(), x_background_weight=1.0)
    with pytest.raises(ValueError, match="needs x_entry_weights"):
        collective_matrix_factorization(X, Y, n_components=3, solver="als", l2_reg=0.1, x_init="random", y_init="random",
                                        x_background_weight=1.0)


def test_a_stored_weight_below_the_background_is_refused(no_device):
    from pycmf_amd import CMF
    X, Y, W = _fit_args()
    model = CMF(n_components=3, solver="als", l2_reg=0.1, x_init="random", y_init="random", random_state=0)
    assert W.data.min() < 1.75
    with pytest.raises(ValueError, match="below x_background_weight=1.75"):
        model.fit(X, Y, x_entry_weights=W, x_background_weight=1.75)
    with pytest.raises(ValueError, match="below x_background_weight=1.5"):      # 'observed': every weight is 1
        model.fit(sp.csr_matrix(X * (X > 0.5)), Y, x_entry_weights="observed", x_background_weight=1.5)
    model.components, model.x_weights, model.y_weights = np.ones((X.shape[1], 3)), None, None
    with pytest.raises(ValueError, match="below x_background_weight=1.75"):      # the fold-in validates the same way
        model.transform(X, None, x_entry_weights=W, x_background_weight=1.75)
    with pytest.raises(AssertionError, match="device context was opened"):      # good values: the fit goes on to the device
        model.fit(X, Y, x_entry_weights=W, x_background_weight=1.0)


def test_implicit_confidence():
    import pycmf_amd
    rng = np.random.RandomState(0)
    R = sp.csr_matrix(rng.poisson(0.3, (9, 7)).astype(float))
    P, W = pycmf_amd.implicit_confidence(R, alpha=2.0, background=0.5)
    assert sp.issparse(P) and sp.issparse(W) and P.shape == W.shape == R.shape
    assert (P.indptr == R.indptr).all() and (P.indices == R.indices).all() and (W.indptr == R.indptr).all() and (W.indices == R.indices).all()
    assert (P.data == 1).all() and (W.data == 0.5 + 2.0 * R.data).all()
    P, W = pycmf_amd.implicit_confidence(R.tocoo())                     # defaults: confidence 1 + count, any sparse layout
    assert (W.toarray() == np.where(R.toarray() > 0, 1 + R.toarray(), 0)).all() and (P.toarray() == (R.toarray() > 0)).all()
    for bad in (-1.0, np.nan, np.inf):
        Rb = R.copy()
        Rb.data[0] = bad
        with pytest.raises(ValueError, match="counts must be"):
            pycmf_amd.implicit_confidence(Rb)
    with pytest.raises(ValueError, match="SciPy sparse"):
        pycmf_amd.implicit_confidence(R.toarray())
    with pytest.raises(ValueError, match="alpha must be"):
        pycmf_amd.implicit_confidence(R, alpha=-1)
    assert "implicit_confidence" in pycmf_amd.__all__


def test_clone_carries_nothing_new():
    """The keywords are fit parameters: the estimator has no attribute for them."""
    from sklearn.base import clone
    from pycmf_amd import CMF
    model = CMF(n_components=4, solver="als", l2_reg=2.0, U_non_negative=False)
    assert not any("background" in name for name in model.get_params())
    assert clone(model).get_params() == model.get_params()


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared_and_the_class_enums_stay():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11 and enum["CMF_K_END"] == 12
    for name, nargs in (("cmf_set_background_weight", 3), ("cmf_get_background_weight", 3), ("cmf_als_residual_sq", 3)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("set_background_weight", "get_background_weight", "als_residual_sq"))
    text = header[header.index("ALS for implicit feedback"):header.index("int cmf_set_background_weight")]
    assert "w_ic >= c0" in text and "cmf_mu_weighted_step" in text and "CMF_EUNSUPPORTED" in text and "exact route for V" in text


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    for name in (b"cmf_set_background_weight", b"cmf_get_background_weight", b"cmf_als_residual_sq", b"als_bg_excess_kernel",
                 b"als_bg_combine_kernel", b"als_bg_res_csr_kernel", b"als_bg_dot64_kernel"):
        assert name in blob, name
