"""Dual form of the exact ALS rows (als_dual_max), host side: the NumPy yardstick (als_dual_yardstick.py) against the primal rows of
als_yardstick.py in float64, the planner's class rule at its edges, keyword validation before any device is opened, the option
outside get_params(), the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import als_dual_cases as C
import als_dual_yardstick as D
import als_yardstick as A
from test_gpu_wmu import fit_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(n_components=3, solver="als", l2_reg=0.05, x_init="random", y_init="random", random_state=0)
SIGNED = dict(U_non_negative=False, V_non_negative=False, Z_non_negative=False)


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
@pytest.mark.parametrize("k", [7, 40, 100])
@pytest.mark.parametrize("which", ["U", "V", "Z"])
def test_dual_rows_equal_the_primal_rows_in_float64(which, k):
    """Two observed sides, stored zero weights, rows of 0, 1 and more than k entries: with every row sent through the dual formulas
    (k_pad ignored: ``dual_row`` directly) and through the planner, the rows equal the primal ones to 1e-10 relative."""
    X, Y, Wx, Wy, F = C.problem(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    primal = A.sweep(Rx, Ry, *F, which, C.L2)
    lens = D.lengths(Rx, Ry, which)
    # (a V row holds the three full rows of X and at most 48 + 40 entries)
    assert which == "V" or (lens.min() == 0 and (lens == 1).any() and lens.max() > k)
    planned = D.dual_rows(Rx, Ry, *F, which, C.L2, 128)
    scale = np.abs(primal).max()
    assert np.abs(planned - primal).max() <= 1e-10 * scale
    obs = A._observed_sides(Rx, Ry, *F, which, 0.0, 0.0, np.float64)
    zero_w = 0
    for i, n in enumerate(lens):
        if n == 0:
            assert (primal[i] == 0).all() and (planned[i] == 0).all()
            continue
        Bs, ws, pvs = zip(*[(B[idx[ip[i]:ip[i + 1]]], e[ip[i]:ip[i + 1]], pv[ip[i]:ip[i + 1]]) for B, ip, idx, pv, e in obs])
        zero_w += int(sum((w == 0).sum() for w in ws))
        K, z, f = D.dual_row(Bs, ws, pvs, C.L2)
        assert K.shape == (n, n) and np.abs(K - K.T).max() == 0 and np.linalg.eigvalsh(K).min() >= C.L2 * (1 - 1e-9)
        assert np.abs(f - primal[i]).max() <= 1e-10 * scale, (which, k, i, n)
        for order in D.ORDERS:
            assert np.abs(D.dual_row(Bs, ws, pvs, C.L2, order=order)[2] - primal[i]).max() <= 1e-10 * scale
    assert zero_w > 0                                                              # the stored zero weights are on the rows


def test_class_rule_at_the_edges():
    assert [D.class_width(n) for n in (1, 32, 33, 64, 65, 128)] == [32, 32, 64, 64, 128, 128]
    assert [D.k_pad(k) for k in (1, 32, 33, 64, 65, 128, 129, 256)] == [32, 32, 64, 64, 128, 128, 256, 256]
    # k_pad = 256: every class; 129 entries are beyond the largest
    assert [D.route(n, 200, 128) for n in (0, 1, 32, 33, 64, 65, 128, 129)] == [D.ZERO, 32, 32, 64, 64, 128, 128, D.FORMED]
    # NP(n) = k_pad is not dual: the dual system must be strictly the smaller one
    assert [D.route(n, 100, 128) for n in (32, 33, 64, 65, 128)] == [32, 64, 64, D.FORMED, D.FORMED]
    assert [D.route(n, 40, 128) for n in (1, 32, 33, 64)] == [32, 32, D.FORMED, D.FORMED]
    assert [D.route(n, 3, 128) for n in (0, 1, 32, 33)] == [D.ZERO, D.FORMED, D.FORMED, D.FORMED]      # k_pad = 32 never goes dual
    # the permission cuts inside a class; 0 is off
    assert [D.route(n, 200, 20) for n in (1, 20, 21, 32)] == [32, 32, D.FORMED, D.FORMED]
    assert [D.route(n, 200, 64) for n in (64, 65)] == [64, D.FORMED]
    assert [D.route(n, 200, 0) for n in (0, 1, 5)] == [D.ZERO, D.FORMED, D.FORMED]
    X, Y, Wx, Wy, F = C.problem(40)
    routes = D.plan(A.Relation(X, Wx), A.Relation(Y, Wy), "U", 200, 128)
    want = [D.route(n, 200, 128) for n in (C.LENGTHS * 4)[:C.M]]
    assert routes == want and D.counts(routes) == (want.count(32), want.count(64), want.count(128), want.count(D.FORMED), want.count(D.ZERO))
    assert sum(D.counts(routes)) == C.M and all(v > 0 for v in D.counts(routes))


# ------------------------------------------------------------------ keyword validation
@pytest.mark.parametrize("value", [-1, 129, 2.0, "4", None, True])
def test_bad_values_are_refused_before_a_device_is_touched(no_device, value):
    from pycmf_amd import CMF, HipALSSolver
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_dual_max must be an integer 0 .. 128"):
        CMF(**dict(KW, als_dual_max=value)).fit(X, Y)
    with pytest.raises(ValueError, match="als_dual_max must be an integer 0 .. 128"):
        HipALSSolver(l2_reg=0.05, dual_max=value)


@pytest.mark.parametrize("solver", ["mu", "hals", "newton"])
def test_other_solvers_refuse_the_keyword(no_device, solver):
    from pycmf_amd import CMF
    X, Y, _, U, V, Z = _planted()
    with pytest.raises(ValueError, match="als_dual_max is the dual row solve of solver='als'"):
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, als_dual_max=64).fit(X, Y)
    with pytest.raises(AssertionError, match="device context was opened"):        # 0 is every solver's default: the fit goes on
        CMF(n_components=3, solver=solver, x_init="random", y_init="random", random_state=0, als_dual_max=0).fit(X, Y)


def test_more_gpus_and_conjugate_gradients_refuse_the_keyword_and_the_rest_is_accepted(no_device):
    from pycmf_amd import CMF, HipALSSolver
    X, Y, Wx, U, V, Z = _planted()
    kw = dict(KW, als_dual_max=64)
    Xs = sp.csr_matrix(X * Wx)
    with pytest.raises(ValueError, match="n_gpus must be 1"):
        CMF(n_gpus=2, **kw).fit(X, Y)
    with pytest.raises(ValueError, match="conjugate gradients already take every sweep"):
        CMF(als_cg_steps=6, **SIGNED, **kw).fit(Xs, Y, x_entry_weights="observed")
    with pytest.raises(ValueError, match="conjugate gradients already take every sweep"):
        HipALSSolver(l2_reg=0.05, dual_max=64, cg_steps=6, **SIGNED)
    # accepted, each up to the first device call: signed and non-negative factors, the logistic loss, biases, a background weight
    Xl = sp.csr_matrix((X > np.median(X)) * Wx)
    for model, args, kwargs in ((CMF(**SIGNED, **kw), (Xs, Y), dict(x_entry_weights="observed")),
                                (CMF(als_nn_sweeps=4, **kw), (Xs, Y), dict(x_entry_weights="observed")),
                                (CMF(als_nn_cg_steps=4, **kw), (Xs, Y), dict(x_entry_weights="observed")),
                                (CMF(loss="logistic", x_link="logit", **SIGNED, **kw), (Xl, Y), dict(x_entry_weights=sp.csr_matrix(Wx))),
                                (CMF(**SIGNED, **kw), (Xs, Y), dict(x_entry_weights="observed", x_biases=True)),
                                (CMF(**SIGNED, **kw), (Xs, Y), dict(x_entry_weights="observed", x_background_weight=0.5))):
        with pytest.raises(AssertionError, match="device context was opened"):
            model.fit(*args, **kwargs)
    solver = HipALSSolver(l2_reg=0.05, dual_max=np.int64(128), nn_sweeps=2)
    assert (solver.dual_max, solver.nn_sweeps, solver.cg_steps) == (128, 2, 0)


def test_the_option_outside_get_params_survives_clone_set_params_and_repr(no_device):
    from sklearn.base import clone
    from pycmf_amd import CMF, HipALSSolver
    X, Y, _, U, V, Z = _planted()
    assert CMF().als_dual_max == 0 and "als_dual_max" not in CMF(als_dual_max=64).get_params()
    assert CMF(solver="als", l2_reg=0.05).get_params() == CMF(solver="als", l2_reg=0.05, als_dual_max=0).get_params()
    assert vars(CMF(solver="als")) == vars(CMF(solver="als", als_dual_max=0))
    with pytest.raises(TypeError, match="unexpected keyword argument 'als_dual_maxx'"):
        CMF(als_dual_maxx=4)
    plain, zero = HipALSSolver(l2_reg=0.05), HipALSSolver(l2_reg=0.05, dual_max=0)
    assert plain.dual_max == zero.dual_max == 0 and vars(plain).keys() == vars(zero).keys()
    first = CMF(n_components=3, solver="als", l2_reg=0.05, als_dual_max=64)
    model = clone(first)
    assert model is not first and model.als_dual_max == 64 and model._kwargs()["als_dual_max"] == 64
    assert model.get_params() == first.get_params() and clone(clone(model)).als_dual_max == 64
    assert model.set_params(als_dual_max=128, max_iter=7) is model and (model.als_dual_max, model.max_iter) == (128, 7)
    assert clone(CMF(n_components=3)).als_dual_max == 0 and "als_dual_max" not in repr(CMF(n_components=3))
    assert repr(model).endswith(", als_dual_max=128)") and repr(CMF(als_dual_max=2)) == "CMF(als_dual_max=2)"
    both = CMF(als_nn_cg_steps=3, als_dual_max=5)
    assert repr(both) == "CMF(als_nn_cg_steps=3, als_dual_max=5)" and (clone(both).als_nn_cg_steps, clone(both).als_dual_max) == (3, 5)
    with pytest.raises(AssertionError, match="device context was opened"):
        model.set_params(x_init="random", y_init="random", random_state=0).fit(X, Y)
    with pytest.raises(ValueError, match="als_dual_max must be an integer 0 .. 128"):
        clone(model).set_params(als_dual_max=-2).fit(X, Y)


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11                                              # (no new kernel class: CMF_K_ROWHESS)
    for name, nargs in (("cmf_als_dual_step", 7), ("cmf_als_dual_rows", 7), ("cmf_als_dual_last", 2)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("als_dual_step", "als_dual_rows", "als_dual_last"))
    step = re.search(r"\bint\s+cmf_als_step\s*\(([^;]*)\)\s*;", header)
    assert len(step.group(1).split(",")) == 4                                     # keeps its signature
