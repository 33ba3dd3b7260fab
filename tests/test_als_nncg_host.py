"""Matrix-free non-negative rows of the ALS solver (als_nn_cg_steps), host side: the NumPy yardstick (nncg_yardstick.py) -- descent
with non-negative factors, convergence to scipy's NNLS and its KKT conditions, float32 against float64 decisions on the fixtures of
the device tests --, keyword validation before any device is opened, the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.linalg
import scipy.optimize
import scipy.sparse as sp

import als_yardstick as A
import nncg_cases as C
import nncg_yardstick as N
from test_gpu_wmu import fit_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2 = 0.05


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _planted(seed=3, k=3):
    X, Y, Wx, _, U, V, Z = fit_inputs(seed, m=120, d=150, p=20, k=k, obs=.3)
    return X, Y, Wx, U, V, Z


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("steps", [2, 6])
@pytest.mark.parametrize("k", [3, 12])
@pytest.mark.parametrize("seed", [3, 5, 7])
def test_planted_problem_descends_at_every_iteration_with_non_negative_factors(seed, k, steps):
    """Planted rank 3, 120 x 150 with 30 % of X observed, Y unweighted (its sweeps keep 4 passes of coordinate descent), l2 = 0.05,
    all three factors non-negative, 10 iterations in float64: the objective falls at every iteration and the factors stay >= 0."""
    X, Y, Wx, U, V, Z = _planted(seed, k)
    Ws = sp.csr_matrix(Wx)
    trace = []
    Un, Vn, Zn = N.fit(X, Y, Ws, None, U, V, Z, 10, L2, nn_mask=7, nn_sweeps=4, nn_cg_steps=steps, trace=trace)
    seq = [A.objective(X, Y, Ws, None, U, V, Z, L2)] + trace
    print("seed %d k %d, %d steps: objective %s" % (seed, k, steps, " ".join("%.2f" % v for v in seq)))
    assert len(trace) == 10 and all(b < a for a, b in zip(seq, seq[1:])), seq
    assert all((F >= 0).all() and np.isfinite(F).all() for F in (Un, Vn, Zn))


def test_many_steps_reach_the_nnls_solution_and_its_kkt_conditions():
    """The U rows of the planted problem after 2000 steps against scipy.optimize.nnls on the Cholesky-transformed systems (the
    construction of test_als_nnls_host.py): within 1e-10 relative, f >= 0, (H f - g)_j >= -eps where f_j = 0 and |(H f - g)_j| <= eps
    where f_j > 0."""
    X, Y, Wx, U, V, Z = _planted()
    Rx, Ry = A.Relation(X, sp.csr_matrix(Wx)), A.Relation(Y, None)
    H, g = A.systems(Rx, Ry, U, V, Z, "U", L2)
    F, traces, _, passes = N.rows(Rx, Ry, U, V, Z, "U", L2, 2000)
    ref = np.empty_like(F)
    for i in range(len(F)):
        L = np.linalg.cholesky(H[i])
        ref[i] = scipy.optimize.nnls(L.T, scipy.linalg.solve_triangular(L, g[i], lower=True))[0]
    rel = np.abs(F - ref).max() / np.abs(ref).max()
    grad = np.einsum("nij,nj->ni", H, F) - g
    eps = 1e-10 * (np.abs(g).max() + np.abs(np.einsum("nij,nj->ni", H, F)).max())
    print("2000 steps against scipy nnls: %.2e relative; clipped coordinates %d of %d; passes per row at most %d" % (rel, int((F == 0).sum()), F.size, passes.max()))
    assert rel <= 1e-10
    assert (F >= 0).all() and (grad[F == 0] >= -eps).all() and (np.abs(grad[F > 0]) <= eps).all()
    assert (F == 0).any() and (F > 0).any()
    assert all(t[-1] == "stop" for t in traces)      # every row stopped by itself, long before 2000 steps


def test_a_row_is_read_at_most_twice_per_step_and_rows_without_information_are_zeros():
    c = C.case(40)
    Rx, Ry = C.relations(c)
    for steps in C.STEPS:
        F, traces, _, passes = N.rows(Rx, Ry, *c[4], "U", L2, steps)
        assert (passes[np.arange(len(F)) != 4] >= 2).all() and passes.max() <= 2 * steps + 1
        assert passes[4] == 0 and (F[4] == 0).all() and traces[4] == []          # the empty row of X
        assert (F >= 0).all()
    kinds = [s[0] for t in traces for s in t if s != "stop"]
    assert "free" in kinds and "proj" in kinds                                   # both kinds of step are exercised


def test_other_routes_are_kept():
    """A signed factor keeps CG or the exact rows, a non-negative one without an observed relation the route nn_sweeps names."""
    X, Y, Wx, U, V, Z = _planted()
    Ws = sp.csr_matrix(Wx)
    same = lambda a, b: all((x == y).all() for x, y in zip(a, b))
    assert same(N.step(X, Y, Ws, None, U, V, Z, L2, nn_cg_steps=3, cg_steps=4), A.step(X, Y, Ws, None, U, V, Z, L2, cg_steps=4))
    assert same(N.step(X, Y, Ws, None, U, V, Z, L2, nn_cg_steps=3, nn_mask=A.Z_BIT, nn_sweeps=2),
                A.step(X, Y, Ws, None, U, V, Z, L2, nn_mask=A.Z_BIT, nn_sweeps=2))
    assert not same(N.step(X, Y, Ws, None, U, V, Z, L2, nn_cg_steps=3, nn_mask=A.U_BIT, nn_sweeps=2),
                    A.step(X, Y, Ws, None, U, V, Z, L2, nn_mask=A.U_BIT, nn_sweeps=2))


@pytest.mark.parametrize("k", C.KS)
def test_float32_and_float64_take_the_same_decisions_on_the_device_fixtures(k):
    """Every comparison of test_gpu_als_nncg.py: the rows outside the asserted set of nncg_cases.py (a float32 trace that differs
    under one of four orders of summation, or a margin under 4 (k + 16) 2^-24) are at most a tenth of a comparison, the long rows
    of the piece tests are inside it, the float32 yardstick in stored order is inside its own envelope; all rows, in both
    precisions, are >= 0 and no higher on their quadratic than the start."""
    worst = total = differ = 0
    for yform, bg in (("full", False), ("observed", False), ("full", True)):
        c = C.case(k, yform, bg)
        cx = 1.0 if bg else 0.0
        for which in C.sweeps(yform):
            H, g = C.start_quadratic(c, which, cx)
            q0 = N.quadratic(H, g, np.maximum(c[4]["UVZ".index(which)], 0))
            lens = C.row_lengths(c, which)
            for steps in C.STEPS:
                r = C.reference(c, which, steps, cx)
                y64, y32, asserted = r["y64"], r["y32"], r["asserted"]
                out = int((~asserted).sum())
                total, differ, worst = total + len(asserted), differ + out, max(worst, out / len(asserted))
                assert out <= 0.1 * len(asserted), (yform, bg, which, steps, out)
                assert not (lens > 32).any() or asserted[lens > 32].any(), (yform, bg, which, steps)
                assert np.abs(y32 - y64)[asserted].max() <= r["envelope"]
                assert (y64 >= 0).all() and (y32 >= 0).all()
                assert (N.quadratic(H, g, y64) <= q0 + 1e-12 * np.abs(q0)).all()
                assert (N.quadratic(H, g, y32) <= q0 + 1e-5 * np.abs(q0)).all()
    print("k %d: %d of %d rows outside the asserted set, at most %.1f %% of a comparison" % (k, differ, total, 100 * worst))


# ------------------------------------------------------------------ validation before any device is opened
KW = dict(n_components=3, solver="als", l2_reg=0.05, x_init="random", y_init="random", random_state=0)


@pytest.mark.parametrize("value", [-1, 1025, 2.0, "4", None, True])
def test_bad_step_counts_are_refused_before_a_device_is_touched(no_device, value):
    from pycmf_amd import CMF, HipALSSolver
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_nn_cg_steps must be an integer 0 .. 1024"):
        CMF(**dict(KW, als_nn_cg_steps=value)).fit(X, Y)
    with pytest.raises(ValueError, match="als_nn_cg_steps must be an integer 0 .. 1024"):
        HipALSSolver(l2_reg=0.05, nn_cg_steps=value)


@pytest.mark.parametrize("solver", ["mu", "hals", "newton"])
def test_other_solvers_refuse_the_keyword(no_device, solver):
    from pycmf_amd import CMF
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_nn_cg_steps is the non-negative conjugate-gradient row solve of solver='als'"):
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, als_nn_cg_steps=4).fit(X, Y)
    with pytest.raises(AssertionError, match="device context was opened"):        # 0 is every solver's default: the fit goes on
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, als_nn_cg_steps=0).fit(X, Y)


def test_signed_factors_more_gpus_logistic_and_biases_refuse_the_keyword(no_device):
    from pycmf_amd import CMF, HipALSSolver
    from pycmf_amd.estimator import collective_matrix_factorization
    X, Y, Wx, U, V, Z = _planted()
    kw = dict(KW, als_nn_cg_steps=4)
    with pytest.raises(ValueError, match="acts on non-negative factors only"):
        CMF(U_non_negative=False, V_non_negative=False, Z_non_negative=False, **kw).fit(X, Y)
    with pytest.raises(ValueError, match="acts on non-negative factors only"):   # the one non-negative factor is not updated
        collective_matrix_factorization(X, Y, n_components=3, solver="als", l2_reg=0.05, U=U, V=V, Z=Z, x_init="custom", y_init="custom",
                                        U_non_negative=False, Z_non_negative=False, update_V=False, als_nn_cg_steps=4)
    with pytest.raises(ValueError, match="n_gpus must be 1"):
        CMF(n_gpus=2, **kw).fit(X, Y)
    Xl = sp.csr_matrix((X > np.median(X)) * Wx)
    with pytest.raises(ValueError, match="als_nn_cg_steps=4 with loss='logistic' is not built"):
        CMF(loss="logistic", x_link="logit", **kw).fit(Xl, Y, x_entry_weights=sp.csr_matrix(Wx))
    with pytest.raises(ValueError, match="als_nn_cg_steps=4 with loss='logistic' is not built"):
        HipALSSolver(l2_reg=0.05, nn_cg_steps=4, loss="logistic", x_link="logit", x_entry_weights="observed")
    with pytest.raises(ValueError, match="als_nn_cg_steps=4 with x_biases / y_biases is not built"):
        CMF(**kw).fit(sp.csr_matrix(X * Wx), Y, x_entry_weights="observed", x_biases=True)
    with pytest.raises(ValueError, match="als_nn_cg_steps=4 with x_biases / y_biases is not built"):
        HipALSSolver(l2_reg=0.05, nn_cg_steps=4, x_entry_weights="observed", x_biases=True)
    with pytest.raises(AssertionError, match="device context was opened"):        # the defaults (all non-negative) take it
        CMF(**kw).fit(sp.csr_matrix(X * Wx), Y, x_entry_weights="observed")
    with pytest.raises(AssertionError, match="device context was opened"):        # beside CG on a signed factor
        CMF(V_non_negative=False, als_cg_steps=3, **kw).fit(sp.csr_matrix(X * Wx), Y, x_entry_weights="observed")


def test_the_existing_checks_keep_their_messages(no_device):
    from pycmf_amd import CMF
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_cg_steps=4 acts on signed factors only"):
        CMF(**dict(KW, als_cg_steps=4, als_nn_cg_steps=4)).fit(X, Y)
    with pytest.raises(ValueError, match="als_cg_steps must be an integer 0 .. 1024"):
        CMF(**dict(KW, als_cg_steps=-1, als_nn_cg_steps=4)).fit(X, Y)


def test_zero_constructs_what_it_constructed_before_and_the_keyword_survives_clone(no_device):
    """The keyword is an option outside ``get_params`` (tests/test_als_bias_host.py pins that list): the default constructs what was
    constructed before; ``clone`` and ``set_params`` carry a value all the same."""
    from sklearn.base import clone
    from pycmf_amd import CMF, HipALSSolver
    X, Y, _, U, V, Z = _planted()
    assert CMF().als_nn_cg_steps == 0 and "als_nn_cg_steps" not in CMF(als_nn_cg_steps=4).get_params()
    assert CMF(solver="als", l2_reg=0.05, als_nn_sweeps=4).get_params() == CMF(solver="als", l2_reg=0.05, als_nn_sweeps=4, als_nn_cg_steps=0).get_params()
    assert vars(CMF(solver="als", als_nn_sweeps=4)) == vars(CMF(solver="als", als_nn_sweeps=4, als_nn_cg_steps=0))
    with pytest.raises(TypeError, match="unexpected keyword argument 'als_nn_cg_step'"):
        CMF(als_nn_cg_step=4)
    plain, zero = HipALSSolver(l2_reg=0.05, nn_sweeps=4, cg_steps=2), HipALSSolver(l2_reg=0.05, nn_sweeps=4, cg_steps=2, nn_cg_steps=0)
    assert plain.nn_cg_steps == zero.nn_cg_steps == 0 and vars(plain).keys() == vars(zero).keys()
    assert (plain.nn_sweeps, plain.cg_steps, plain.als_loss) == (zero.nn_sweeps, zero.cg_steps, zero.als_loss)
    first = CMF(n_components=3, solver="als", l2_reg=0.05, als_nn_cg_steps=4)
    model = clone(first)
    assert model is not first and model.als_nn_cg_steps == 4 and model._kwargs()["als_nn_cg_steps"] == 4
    assert model.get_params() == first.get_params() and clone(clone(model)).als_nn_cg_steps == 4
    assert model.set_params(als_nn_cg_steps=6, max_iter=7) is model and (model.als_nn_cg_steps, model.max_iter) == (6, 7)
    assert clone(CMF(n_components=3)).als_nn_cg_steps == 0 and "als_nn_cg_steps" not in repr(CMF(n_components=3))
    assert repr(model).endswith(", als_nn_cg_steps=6)") and repr(CMF(als_nn_cg_steps=2)) == "CMF(als_nn_cg_steps=2)"
    with pytest.raises(AssertionError, match="device context was opened"):
        model.set_params(x_init="random", y_init="random", random_state=0).fit(X, Y)
    with pytest.raises(ValueError, match="als_nn_cg_steps must be an integer 0 .. 1024"):
        clone(model).set_params(als_nn_cg_steps=-2).fit(X, Y)
    solver = HipALSSolver(l2_reg=0.05, nn_cg_steps=np.int64(4), nn_sweeps=2, cg_steps=3)
    assert (solver.nn_cg_steps, solver.nn_sweeps, solver.cg_steps) == (4, 2, 3)


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11                                              # (no new kernel class: CMF_K_ROWHESS)
    for name, nargs in (("cmf_als_nncg_step", 7), ("cmf_als_nncg_rows", 7), ("cmf_als_nncg_last", 2), ("cmf_als_nncg_passes", 2)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("als_nncg_step", "als_nncg_rows", "als_nncg_last", "als_nncg_passes"))
    bias = re.search(r"\bint\s+cmf_als_bias_step\s*\(([^;]*)\)\s*;", header)
    assert len(bias.group(1).split(",")) == 6                                     # keeps its signature


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    for name in (b"cmf_als_nncg_step", b"cmf_als_nncg_rows", b"cmf_als_nncg_last", b"als_nncg_kernel", b"als_nncg_combine_kernel"):
        assert name in blob, name
