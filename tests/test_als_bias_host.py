"""ALS with a global mean and row / column biases, host side: the yardstick (als_bias_yardstick.py) against als_yardstick.py where the
two must coincide, its optimality conditions, the monotone descent on all three routes, the float32 mirror with piece-ordered sums
against the rule of the project on the fixtures of the device tests, keyword validation before any device is opened, the planted
rating problem of the documentation, the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import als_bias_cases as C
import als_bias_yardstick as B
import als_yardstick as A

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
    X, Y = 2.0 + rng.randn(m, d), rng.randn(d, p) - 1.0
    Wx = (0.25 + 3.75 * rng.rand(m, d)) * (rng.rand(m, d) < 0.35)
    Wx[m // 4] = 0
    Wx[:, d // 3] = 0
    Wy = (0.25 + 3.75 * rng.rand(d, p)) * (rng.rand(d, p) < 0.5)
    F = [0.5 * rng.randn(n, k) for n in (m, d, p)]
    return A.Relation(X, sp.csr_matrix(Wx)), A.Relation(Y, sp.csr_matrix(Wy)), F


ROUTES = {"exact": dict(), "cg": dict(cg_steps=3), "nn": dict(nn_mask=7, nn_sweeps=4)}


# ------------------------------------------------------------------ the yardstick itself
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_zero_biases_and_zero_mean_leave_the_factor_sweeps_of_als_yardstick(route):
    Rx, Ry, F = _problem()
    kw = ROUTES[route]
    F = [np.abs(f) for f in F] if kw.get("nn_mask") else F
    for mask in (7, 1, 2, 4):
        want = A.step(Rx, Ry, None, None, *F, 0.1, mask=mask, **kw)
        got = B.step(Rx, Ry, None, None, *F, B.zero_bias(Rx), B.zero_bias(Ry), 0.1, 0.77, mask=mask, **kw)
        for w in range(3):
            assert (got[w] == want[w]).all(), (route, mask, w)
        got32 = B.step(Rx, Ry, None, None, *F, B.zero_bias(Rx), B.zero_bias(Ry), 0.1, 0.77, mask=mask, dtype=np.float32, **kw)
        want32 = A.step(Rx, Ry, None, None, *F, 0.1, mask=mask, dtype=np.float32, **kw)
        for w in range(3):
            assert (got32[w] == want32[w]).all(), (route, mask, w)


@pytest.mark.parametrize("lb", [0.0, 0.3, 5.0])
def test_every_bias_sweep_zeroes_its_block_of_the_gradient(lb):
    Rx, Ry, F = _problem(seed=6)
    rng = np.random.RandomState(1)
    for rel, Fa, Fb in ((Rx, F[0], F[1]), (Ry, F[1], F[2])):
        bias = (0.4, rng.randn(rel.shape[0]), rng.randn(rel.shape[1]))
        for axis in (0, 1):
            new = B.bias_sweep(rel, Fa, Fb, bias, lb, axis)
            moved = (bias[0], new, bias[2]) if axis == 0 else (bias[0], bias[1], new)
            assert np.abs(B.bias_gradient(rel, Fa, Fb, bias, lb, axis)).max() > 1e-2
            g = B.bias_gradient(rel, Fa, Fb, moved, lb, axis)
            assert np.abs(g).max() <= 1e-10, (lb, axis, np.abs(g).max())
            empty = rel.row_lengths(axis == 1) == 0
            assert (new[empty] == 0).all()
            for piece in (16, 64):     # piece order changes no float64 result beyond rounding
                assert np.abs(B.bias_sweep(rel, Fa, Fb, bias, lb, axis, piece=piece) - new).max() <= 1e-13
    assert (Rx.row_lengths(False) == 0).any() and (Rx.row_lengths(True) == 0).any()


def test_a_row_whose_weights_are_all_zero_gets_zero_when_lb_is_zero():
    W = sp.csr_matrix((np.array([0.0, 0.0, 2.0]), (np.array([0, 0, 1]), np.array([0, 2, 1]))), shape=(3, 3))
    rel = A.Relation(np.arange(9.0).reshape(3, 3), W)
    F = np.ones((3, 2))
    r = B.bias_sweep(rel, F, F, (0.0, np.zeros(3), np.zeros(3)), 0.0, 0)
    assert r[0] == 0 and r[2] == 0 and r[1] == 4.0 - 2.0


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_the_objective_never_rises_over_ten_iterations(route):
    Rx, Ry, F = _problem(seed=7)
    kw = ROUTES[route]
    U, V, Z = [np.abs(f) for f in F] if kw.get("nn_mask") else F
    bx, by = B.zero_bias(Rx, B.weighted_mean(Rx)), B.zero_bias(Ry, B.weighted_mean(Ry))
    seq = [B.objective(Rx, Ry, None, None, U, V, Z, bx, by, 0.1, 0.3)]
    for _ in range(10):
        U, V, Z, bx, by = B.step(Rx, Ry, None, None, U, V, Z, bx, by, 0.1, 0.3, **kw)
        seq.append(B.objective(Rx, Ry, None, None, U, V, Z, bx, by, 0.1, 0.3))
    assert all(b <= a * (1 + 1e-12) for a, b in zip(seq, seq[1:])) and seq[-1] < 0.5 * seq[0], seq


def test_the_mask_moves_the_bias_blocks_of_its_axis_only():
    Rx, Ry, F = _problem(seed=8)
    rng = np.random.RandomState(2)
    bx, by = (0.4, rng.randn(31), rng.randn(27)), (-0.2, rng.randn(27), rng.randn(13))
    for mask in (1, 2, 4, 7):
        out = B.step(Rx, Ry, None, None, *F, bx, by, 0.1, 0.3, mask=mask)
        for (name, new), (_, old) in zip(C.step_vectors(out), C.step_vectors((*F, bx, by))):
            assert (not (new == old).all()) == bool(C.MOVED[name] & mask), (mask, name)


# ------------------------------------------------------------------ the float32 mirror against the rule
def _ratio(y32, y64):
    m = float(np.abs(y64).max())
    return 4.0 * float(np.abs(y32 - y64).max()) / (B.CAP * m) if m > 0 else 0.0


def test_float32_sweeps_in_pieces_of_64_stay_inside_the_rule_and_the_cap():
    """Every bias sweep of every fixture: the cap holds, and summing in pieces of 64 moves the float32 result by far less than the
    tolerance -- the rule needs no extra term for the piece order.  Worst cap ratio 0.0016 (case A, k = 256, c_y)."""
    worst = 0.0
    for k in C.KS:
        for name in ("A", "B"):
            for which in (0, 1):
                for axis in (0, 1):
                    y64, y32 = C.sweep_reference(name, k, which, axis)
                    assert B.within_cap(y32, y64)
                    worst = max(worst, _ratio(y32, y64))
                    whole = C.sweep_reference(name, k, which, axis, piece=-1)[1]
                    assert np.abs(y32 - whole).max() <= 0.01 * B.tolerance(y32, y64, k)
                    assert ((y64 == 0) == (y32 == 0)).all()
    print("worst 4 max|y32 - y64| / (1e-3 max|y64|) over the sweeps: %.4f" % worst)
    assert worst <= 0.01


@pytest.mark.parametrize("name, k, mask, route", C.STEP_CASES)
def test_float32_steps_stay_inside_the_cap_on_the_cases_the_device_tests_use(name, k, mask, route):
    s64, s32 = C.step_reference(name, k, mask, route)
    for (name, a), (_, b) in zip(C.step_vectors(s64), C.step_vectors(s32)):
        if C.MOVED[name] & mask:
            assert B.within_cap(b, a), (name, _ratio(b, a))
        else:
            assert (a == b).all()


# ------------------------------------------------------------------ keywords
def _fit_args():
    rng = np.random.RandomState(0)
    X, Y = 3.0 + rng.randn(12, 9), rng.randn(9, 5)
    W = sp.csr_matrix((0.5 + rng.rand(12, 9)) * (rng.rand(12, 9) < 0.6))
    return X, Y, W


def _als(**kw):
    from pycmf_amd import CMF
    return CMF(n_components=3, solver="als", l2_reg=0.1, x_init="random", y_init="random", random_state=0, U_non_negative=False,
               V_non_negative=False, Z_non_negative=False, **kw)


def test_biases_need_entry_weights_that_resolve_to_csr(no_device):
    from pycmf_amd import HipALSSolver, collective_matrix_factorization
    X, Y, W = _fit_args()
    with pytest.raises(ValueError, match="x_biases=True needs x_entry_weights.*pass x_entry_weights='observed'"):
        _als().fit(X, Y, x_biases=True)
    with pytest.raises(ValueError, match="y_biases=True needs y_entry_weights"):
        _als().fit_transform(X, Y, x_entry_weights=W, y_biases=True)
    with pytest.raises(ValueError, match="x_biases=True needs x_entry_weights"):      # dense weights name no pattern
        _als().fit(X, Y, x_entry_weights=W.toarray(), x_biases=True)
    with pytest.raises(ValueError, match="x_biases=True needs x_entry_weights"):
        HipALSSolver(l2_reg=0.1, x_biases=True)
    with pytest.raises(ValueError, match="y_biases=True needs y_entry_weights"):
        collective_matrix_factorization(X, Y, n_components=3, solver="als", l2_reg=0.1, x_init="random", y_init="random", y_biases=True)
    with pytest.raises(ValueError, match="x_biases must be True or False"):
        _als().fit(X, Y, x_entry_weights=W, x_biases=1)


def test_biases_and_a_background_weight_are_refused_together(no_device):
    from pycmf_amd import HipALSSolver
    X, Y, W = _fit_args()
    with pytest.raises(ValueError, match="x_biases=True together with x_background_weight=0.25 is not built: pass x_background_weight=0"):
        _als().fit(X, Y, x_entry_weights=W, x_biases=True, x_background_weight=0.25)
    with pytest.raises(ValueError, match="y_biases=True together with y_background_weight"):
        HipALSSolver(l2_reg=0.1, y_entry_weights="observed", y_biases=True, y_background_weight=0.5)


@pytest.mark.parametrize("value", [True, np.nan, np.inf, -0.5, "1"])
def test_bad_bias_l2_values_are_refused(no_device, value):
    from pycmf_amd import HipALSSolver
    X, Y, W = _fit_args()
    with pytest.raises(ValueError, match="bias_l2 must be None .* or a finite number >= 0"):
        _als().fit(X, Y, x_entry_weights=W, x_biases=True, bias_l2=value)
    with pytest.raises(ValueError, match="bias_l2 must be None"):
        HipALSSolver(l2_reg=0.1, x_entry_weights=W, x_biases=True, bias_l2=value)


@pytest.mark.parametrize("solver", ["mu", "hals", "newton"])
def test_biases_need_the_als_solver(no_device, solver):
    from pycmf_amd import CMF
    X, Y, W = _fit_args()
    X, Y = np.abs(X), np.abs(Y)
    model = CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0)
    with pytest.raises(ValueError, match="x_biases is the rating model of solver='als'.*pass solver='als'"):
        model.fit(X, Y, x_entry_weights=(W if solver == "mu" else None), x_biases=True)
    with pytest.raises(ValueError, match="bias_l2 is the bias regulariser of solver='als'"):
        model.fit(X, Y, bias_l2=0.5)


def test_good_keywords_go_on_to_the_device(no_device):
    X, Y, W = _fit_args()
    with pytest.raises(AssertionError, match="device context was opened"):
        _als().fit(X, Y, x_entry_weights=W, x_biases=True, bias_l2=0.0)
    with pytest.raises(AssertionError, match="device context was opened"):
        _als().fit(sp.csr_matrix(X * (X > 3)), Y, x_entry_weights="observed", x_biases=True)


def test_prediction_arguments_fail_before_a_device_opens(no_device):
    import pycmf_amd
    A_, B_ = np.ones((4, 3)), np.ones((5, 3))
    with pytest.raises(ValueError, match="rows must lie in"):
        pycmf_amd.predict_products(A_, B_, [0, 4], [0, 0])
    with pytest.raises(ValueError, match="rows must lie in"):
        pycmf_amd.predict_products(A_, B_, [0, 1], [0, 5])
    with pytest.raises(ValueError, match="one length"):
        pycmf_amd.predict_products(A_, B_, [0, 1], [0])
    with pytest.raises(ValueError, match="integer index"):
        pycmf_amd.predict_products(A_, B_, [0.5], [0.0])
    with pytest.raises(ValueError, match="row_bias must hold 4 finite values"):
        pycmf_amd.predict_products(A_, B_, [0], [0], row_bias=np.ones(5))
    with pytest.raises(ValueError, match="No such link"):
        pycmf_amd.predict_products(A_, B_, [0], [0], link="probit")
    with pytest.raises(NotImplementedError, match="at most 256 components"):
        pycmf_amd.predict_products(np.ones((2, 257)), np.ones((2, 257)), [0], [0])
    assert pycmf_amd.predict_products(A_, B_, [], []).shape == (0,)              # nothing to do: no device either
    assert "predict_products" in pycmf_amd.__all__
    model = pycmf_amd.CMF(n_components=3)
    model.x_weights, model.components, model.y_weights = A_, B_, np.ones((2, 3))
    with pytest.raises(ValueError, match="relation must be 'x' or 'y'"):
        model.predict([0], [0], relation="z")
    with pytest.raises(ValueError, match="held_out must be a SciPy sparse matrix"):
        model.score_entries(np.ones((4, 5)))
    with pytest.raises(ValueError, match="held_out must have shape"):
        model.score_entries(sp.csr_matrix(np.ones((5, 4))))
    model.x_bias_ = type("Bias", (), dict(offset=1.0, rows=np.zeros(4), cols=np.zeros(5), as_tuple=lambda self: (1.0, np.zeros(4), np.zeros(5))))()
    with pytest.raises(ValueError, match="query_bias must hold one value per query"):
        model.top_n(n=2, queries=np.ones((3, 3)), query_bias=np.ones(2))
    big = pycmf_amd.CMF(n_components=255)
    big.x_weights, big.components, big.y_weights, big.x_bias_ = np.ones((4, 255)), np.ones((5, 255)), np.ones((2, 255)), model.x_bias_
    with pytest.raises(NotImplementedError, match=r"n_components \+ 2 <= 256"):
        big.top_n(n=2)


def test_get_params_and_clone_carry_nothing_new():
    from sklearn.base import clone
    from pycmf_amd import CMF
    model = CMF(n_components=4, solver="als", l2_reg=2.0, U_non_negative=False)
    assert not any("bias" in name for name in model.get_params())
    assert sorted(model.get_params()) == sorted(["n_components", "x_init", "y_init", "solver", "alpha", "beta_loss", "tol", "max_iter", "random_state",
                                                 "l1_reg", "l2_reg", "verbose", "U_non_negative", "V_non_negative", "Z_non_negative", "x_link", "y_link",
                                                 "hessian_pertubation", "sg_sample_ratio", "device", "sg_sampler", "n_gpus", "loss", "als_nn_sweeps",
                                                 "als_cg_steps"])
    assert clone(model).get_params() == model.get_params()


# ------------------------------------------------------------------ the planted rating problem
# The table of the proposal, as printed there: (density, noise, l2) -> RMSE on the unobserved cells of X after 10 iterations for
# seeds 3 / 5 / 7, in the columns (biases, k = 3), (no biases, k = 3), (no biases, k = 5).
PLANTED = [
    ((0.30, 0.05, 0.05), (("0.055", "0.055", "0.058"), ("1.13", "1.01", "0.94"), ("0.058", "0.059", "0.058"))),
    ((0.10, 0.30, 0.50), (("0.405", "0.401", "0.414"), ("1.47", "1.27", "1.14"), ("0.567", "0.520", "0.548"))),
    ((0.06, 0.30, 1.00), (("0.783", "0.774", "0.811"), ("3.59", "1.59", "2.45"), ("2.57", "1.18", "2.24"))),
]


def _as_printed(value, like):
    """``value`` with the digits of the table entry ``like``: rounded to three decimals, and where the table shows two, that
    three-decimal figure rounded half up once more -- how the proposal's table was made (0.934957 -> 0.935 -> "0.94")."""
    from decimal import Decimal, ROUND_HALF_UP
    three = Decimal(repr(float(value))).quantize(Decimal("0.001"), rounding=ROUND_HALF_UP)
    return str(three.quantize(Decimal(10) ** -len(like.split(".")[1]), rounding=ROUND_HALF_UP))


@pytest.mark.parametrize("setting, table", PLANTED)
def test_planted_ratings_table(setting, table):
    """120 x 150, rank 3 plus mu = 3.5 and unit-variance row and column offsets, Y 150 x 20 fully observed, 10 iterations from
    als_bias_yardstick.planted (one stream per seed, in the order of click_problem.clicks; Y's noise 0.05): every one of the 27
    entries of the proposal's table comes out to the digits shown.  The entries with two decimals are the three-decimal figures
    rounded once more (1.464570 -> 1.465 -> 1.47, 1.134985 -> 1.135 -> 1.14, 0.934957 -> 0.935 -> 0.94: the three entries a single
    rounding would print as 1.46, 1.13 and 0.93).  In every run of the biased fit the objective falls monotonically, and at 10 % and
    6 % it beats both fits without biases."""
    density, noise, l2 = setting
    for s, seed in enumerate((3, 5, 7)):
        got = []
        for col, (k, biased) in enumerate(((3, True), (3, False), (5, False))):
            X, Y, Wx, start = B.planted(seed, density, noise, k=k)
            Rx, Ry = A.Relation(X, Wx), A.Relation(Y, None)
            trace = []
            U, V, Z, bx, by = B.fit(Rx, Ry, None, None, *start, 10, l2, x_biases=biased, trace=trace)
            if biased:
                assert all(b <= a * (1 + 1e-12) for a, b in zip(trace, trace[1:]))
            got.append(B.heldout_rmse(X, Wx, U, V, bx))
            assert _as_printed(got[col], table[col][s]) == table[col][s], (setting, seed, col, got[col])
        if density < 0.30:
            assert got[0] < 0.85 * min(got[1], got[2])


# ------------------------------------------------------------------ ABI surface
ENTRY_POINTS = (("cmf_set_biases", 5), ("cmf_get_biases", 5), ("cmf_set_bias_f64", 4), ("cmf_get_bias_f64", 4), ("cmf_als_bias_step", 6),
                ("cmf_als_bias_rows", 4), ("cmf_als_bias_targets", 6), ("cmf_predict_pairs", 7))


def test_entry_points_are_declared_and_the_class_enums_stay():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11 and enum["CMF_K_END"] == 12
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, nargs in ENTRY_POINTS:
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
        assert name in doc, name
    assert all(callable(getattr(_lib.Context, n)) for n in ("set_biases", "get_biases", "set_bias", "get_bias", "als_bias_step", "als_bias_rows",
                                                             "als_bias_targets", "predict_pairs"))
    text = header[header.index("ALS for explicit ratings"):header.index("int cmf_set_biases")]
    assert "als_bias_piece" in text and "cmf_mu_weighted_step" in text and "CMF_EUNSUPPORTED" in text and "r_x with U" in text


def test_built_library_exports_the_entry_points_and_kernels():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    for name in [n.encode() for n, _ in ENTRY_POINTS] + [b"als_bias_piece_kernel", b"als_bias_combine_kernel", b"als_bias_targets_kernel",
                                                          b"predict_pairs_kernel"]:
        assert name in blob, name
