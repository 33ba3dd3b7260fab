"""The logistic loss of the ALS solver on every route (als_logit_pass), host side: keyword validation before any device is opened,
the NumPy yardstick (logit_pass_yardstick.py) -- its reweighted relations against the formed systems of logit_yardstick, descent
on every route --, the ABI surface."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
import logit_yardstick as L
import logit_pass_yardstick as LP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNED = dict(U_non_negative=False, V_non_negative=False, Z_non_negative=False)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _data(seed=0):
    rng = np.random.RandomState(seed)
    X = sp.csr_matrix((rng.rand(12, 9) < 0.5) * 1.0)
    Y = rng.rand(9, 5)
    return X, Y


def _fit(fit_kw=None, **kw):
    from pycmf_amd import CMF
    X, Y = _data()
    args = dict(n_components=3, solver="als", loss="logistic", l2_reg=0.5, max_iter=2, x_link="logit", random_state=0, **SIGNED)
    args.update(kw)
    return CMF(**args).fit(X, Y, **(dict(x_entry_weights="observed") if fit_kw is None else fit_kw))


# ------------------------------------------------------------------ the option is accepted up to the first device call
@pytest.mark.parametrize("route", [dict(als_cg_steps=6), dict(als_nn_cg_steps=4, U_non_negative=True, V_non_negative=True, Z_non_negative=True),
                                   dict(als_dual_max=128), dict(), dict(als_nn_sweeps=3, V_non_negative=True),
                                   dict(als_cg_steps=6, als_l2_scale=0.5)])
def test_the_option_is_accepted_up_to_the_first_device_call(no_device, route):
    with pytest.raises(AssertionError, match="device context was opened"):
        _fit(als_logit_pass=True, **route)


def test_the_solver_object_takes_the_option(no_device):
    from pycmf_amd import solver_shell as S
    s = S.HipALSSolver(l2_reg=0.5, loss="logistic", x_link="logit", x_entry_weights="observed", cg_steps=3, logit_pass=True, **SIGNED)
    assert s.logit_pass is True and s.cg_steps == 3 and s._weights_key()[-1] is True
    s = S.HipALSSolver(l2_reg=0.5, loss="logistic", x_link="logit", x_entry_weights="observed", nn_cg_steps=3, dual_max=64, logit_pass=True)
    assert (s.nn_cg_steps, s.dual_max, s.logit_pass) == (3, 64, True)
    assert S.HipALSSolver(l2_reg=0.5).logit_pass is False
    assert S.check_logistic("logit", "linear", "observed", None, 6, logit_pass=True) == (True, False)
    S.check_als_nn_cg_steps(4, loss="logistic", logit_pass=True)
    assert S.check_als_logit_pass(False, "mu", 4, "frobenius") is False and S.check_als_logit_pass(np.bool_(True)) is True


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw, fit_kw, match", [
    # ... of the option itself
    (dict(als_logit_pass=True, loss="frobenius", x_link="linear"), None, "als_logit_pass=True .* needs loss='logistic', got loss='frobenius'"),
    (dict(als_logit_pass=True, solver="mu", loss="frobenius", l2_reg=0.0), dict(), "als_logit_pass is the reweighting pass of solver='als'.*solver='mu'"),
    (dict(als_logit_pass=True, solver="hals", loss="frobenius", l2_reg=0.0), dict(), "must be False with solver='hals'"),
    (dict(als_logit_pass=True, n_gpus=2), None, "runs on one GPU"),
    (dict(als_logit_pass=1), None, "als_logit_pass must be True or False, got 1"),
    (dict(als_logit_pass="yes"), None, "als_logit_pass must be True or False"),
    (dict(als_logit_pass=None), None, "als_logit_pass must be True or False"),
    # ... that stay with the option on
    (dict(als_logit_pass=True, als_cg_steps=6), "biases", "x_biases=True on a logistic relation"),
    (dict(als_logit_pass=True, als_cg_steps=6), "background", "x_background_weight=1.0 on a logistic relation"),
    (dict(als_logit_pass=True, als_cg_steps=6), dict(), "needs x_entry_weights that name the observed entries.*got None"),
    (dict(als_logit_pass=True, als_cg_steps=6), "dense", "needs x_entry_weights that name the observed entries.*got a dense array"),
    (dict(als_logit_pass=True, als_cg_steps=6, x_huber_delta=1.0), None, "x_huber_delta=1.0 on a relation with x_link='logit' is not built"),
    (dict(als_logit_pass=True, als_cg_steps=6, x_link="linear"), None, "x_link or y_link must be 'logit'"),
    (dict(als_logit_pass=True, als_cg_steps=6, als_dual_max=64), None, "als_dual_max=64 together with als_cg_steps=6"),
    (dict(als_logit_pass=True, als_cg_steps=6, U_non_negative=True, V_non_negative=True, Z_non_negative=True), None,
     "als_cg_steps=6 acts on signed factors only"),
    (dict(als_logit_pass=True, als_nn_cg_steps=4), None, "als_nn_cg_steps=4 acts on non-negative factors only"),
    (dict(als_logit_pass=True, l2_reg=0.0), None, "solver='als' needs l2_reg > 0"),
    # ... without the option: the messages as they were
    (dict(als_cg_steps=6), None, r"als_cg_steps=6 with loss='logistic' is not built \(the conjugate-gradient rows have no reweighting pass\): "
                                 "als_cg_steps must be 0; use the exact rows or als_nn_sweeps"),
    (dict(als_nn_cg_steps=4, V_non_negative=True), None, r"als_nn_cg_steps=4 with loss='logistic' is not built \(the conjugate-gradient rows have no "
                                                         "reweighting pass\\): als_nn_cg_steps must be 0; use als_nn_sweeps"),
    (dict(als_logit_pass=False, als_cg_steps=6), None, "als_cg_steps=6 with loss='logistic' is not built"),
])
def test_refusals_by_their_message_before_a_device_is_touched(no_device, kw, fit_kw, match):
    X, _ = _data()
    if fit_kw == "biases":
        fit_kw = dict(x_entry_weights="observed", x_biases=True)
    elif fit_kw == "background":
        fit_kw = dict(x_entry_weights=sp.csr_matrix(X.toarray() + 1.0), x_background_weight=1.0)
    elif fit_kw == "dense":
        fit_kw = dict(x_entry_weights=np.ones(X.shape))
    with pytest.raises(ValueError, match=match):
        _fit(fit_kw, **kw)


def test_more_than_256_components_are_refused_under_the_option(no_device):
    with pytest.raises(NotImplementedError, match="n_components <= 256"):
        _fit(als_logit_pass=True, als_cg_steps=6, n_components=257)


def test_the_solver_object_refuses_too(no_device):
    from pycmf_amd import solver_shell as S
    with pytest.raises(ValueError, match="needs loss='logistic'"):
        S.HipALSSolver(l2_reg=0.5, logit_pass=True)
    with pytest.raises(ValueError, match="als_logit_pass must be True or False"):
        S.HipALSSolver(l2_reg=0.5, loss="logistic", x_link="logit", logit_pass=2)
    with pytest.raises(ValueError, match="als_cg_steps=3 with loss='logistic' is not built"):
        S.HipALSSolver(l2_reg=0.5, loss="logistic", x_link="logit", x_entry_weights="observed", cg_steps=3, **SIGNED)
    with pytest.raises(ValueError, match="als_nn_cg_steps=3 with loss='logistic' is not built"):
        S.HipALSSolver(l2_reg=0.5, loss="logistic", x_link="logit", x_entry_weights="observed", nn_cg_steps=3)
    with pytest.raises(ValueError, match="runs on one GPU: n_gpus must be 1, got 2"):
        S.check_als_logit_pass(True, "als", 2, "logistic")


def test_the_option_survives_clone_set_params_and_repr(no_device):
    from sklearn.base import clone
    from pycmf_amd import CMF
    assert CMF().als_logit_pass is False
    assert "als_logit_pass" not in CMF(als_logit_pass=True).get_params()
    assert CMF(solver="als").get_params() == CMF(solver="als", als_logit_pass=True).get_params()
    assert vars(CMF(solver="als")) == vars(CMF(solver="als", als_logit_pass=False))
    with pytest.raises(TypeError, match="unexpected keyword argument 'als_logit_passes'"):
        CMF(als_logit_passes=True)
    first = CMF(n_components=3, solver="als", loss="logistic", l2_reg=0.5, als_logit_pass=True, als_cg_steps=6)
    model = clone(first)
    assert model is not first and model.als_logit_pass is True and model._kwargs()["als_logit_pass"] is True
    assert model.get_params() == first.get_params() and clone(clone(model)).als_logit_pass is True
    assert model.set_params(als_logit_pass=False, max_iter=7) is model and (model.als_logit_pass, model.max_iter) == (False, 7)
    assert "als_logit_pass" not in repr(model) and repr(CMF(als_logit_pass=True)) == "CMF(als_logit_pass=True)"
    assert repr(first).endswith(", als_logit_pass=True)")


# ------------------------------------------------------------------ the yardstick agrees with the formed systems
def _planted(seed):
    pr = L.planted(seed)
    return pr, L.Relation(pr["T"], pr["Wsp"]), L.Relation(pr["Y"], None)


@pytest.mark.parametrize("which", "UVZ")
def test_reweighted_relations_give_the_systems_of_the_fused_form(which):
    """planted(3): the Frobenius systems of the reweighted relation are the majoriser's systems of logit_yardstick, to 1e-12."""
    pr, Rx, Ry = _planted(3)
    rng = np.random.RandomState(11)
    U, V, Z = (F + 0.5 * rng.randn(*F.shape) for F in pr["start"])             # scores of order 1: kappa varies
    H0, g0 = L.systems(Rx, Ry, U, V, Z, which, pr["l2"], logit=(True, False))
    H1, g1 = A.systems(LP.reweighted(Rx, U, V), Ry, U, V, Z, which, pr["l2"])
    assert np.abs(H1 - H0).max() <= 1e-12 * np.abs(H0).max() and np.abs(g1 - g0).max() <= 1e-12 * np.abs(g0).max()
    hw, hp = LP.weights(Rx, U, V)
    assert hw.min() > 0 and hw.max() / hw.min() > 2 and (np.abs(hp) == 0.5 * Rx.w).all()    # (labels 0 / 1: w t - w / 2 = +-w / 2)


def test_reweighted_writes_both_images_and_keeps_a_zero_weight():
    T = np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    # (the third entry: a stored zero weight)
    rel = A.Relation(T, sp.csr_matrix((np.array([2.0, 1.0, 0.0, 1.0, 3.0]), np.array([0, 1, 2, 1, 2]), np.array([0, 3, 5])), shape=(2, 3)))
    Fa, Fb = np.array([[1.0, 2.0], [0.5, -1.0]]), np.array([[1.0, 0.0], [0.0, 1.0], [2.0, 2.0]])
    out = LP.reweighted(rel, Fa, Fb)
    s = LP.scores(rel, Fa, Fb)
    assert (s == np.array([1.0, 2.0, 6.0, -1.0, -1.0])).all()
    np.testing.assert_allclose(out.w, rel.w * np.tanh(s / 2) / (2 * s), rtol=1e-15)
    assert out.w[2] == 0.0 and out.t[2] == 0.0
    np.testing.assert_allclose(out.w * out.t, rel.w * rel.t - 0.5 * rel.w, rtol=1e-15, atol=0)
    order = np.lexsort((rel.r, rel.c))
    assert (out.images[0][3] == out.w).all() and (out.images[1][3] == out.w[order]).all() and (out.images[1][2] == out.t[order]).all()
    assert (out.images[0][0] == rel.images[0][0]).all() and (out.images[1][1] == rel.images[1][1]).all()
    assert (rel.t == T[rel.r, rel.c]).all()                                      # the input is left alone
    with pytest.raises(ValueError, match="must be observed"):
        LP.reweighted(A.Relation(T, None), Fa, Fb)
    w32 = LP.weights(rel, Fa, Fb, np.float32)
    assert w32[0].dtype == np.float32 and w32[1].dtype == np.float32 and np.abs(w32[0] - out.w).max() <= 2.0 ** -23 * out.w.max()


# ------------------------------------------------------------------ descent
ROUTES = {"exact": (0, dict()), "cg": (0, dict(cg_steps=3)), "nncg": (7, dict(nn_cg_steps=3, nn_sweeps=4)), "nnls": (7, dict(nn_sweeps=4))}
# (nncg: U and V, which read the observed X, run projected CG; Z reads the full Y alone, where nn_cg_steps selects nothing: it keeps the
# coordinate descent of nn_sweeps)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("seed", [3, 5, 7])
def test_objective_never_rises_on_the_planted_problem(seed, route):
    """planted(seed), X logistic, Y full, l2 = 0.5, k = 4, 10 iterations V, U, Z in float64."""
    nn_mask, kw = ROUTES[route]
    pr, Rx, Ry = _planted(seed)
    start = [np.abs(F) if nn_mask else F for F in pr["start"]]
    trace = []
    LP.fit(Rx, Ry, *start, 10, pr["l2"], nn_mask=nn_mask, trace=trace, **kw)
    seq = [LP.objective(Rx, Ry, *start, pr["l2"])] + trace
    print("seed %d %s: %s" % (seed, route, " ".join("%.1f" % v for v in seq)))
    assert len(trace) == 10 and all(b <= a + 1e-9 * abs(a) for a, b in zip(seq, seq[1:])), seq
    assert seq[-1] < 0.75 * seq[0]
    if seed == 3 and route == "exact":
        assert [round(v, 1) for v in seq[:3]] == [10467.4, 4868.1, 2940.8]
        fused = list(pr["start"])
        for _ in range(10):
            fused = L.step(Rx, Ry, None, None, *fused, pr["l2"])
        assert abs(L.objective(Rx, Ry, None, None, *fused, pr["l2"]) - seq[-1]) <= 1e-9 * seq[-1]   # the pass IS the fused step


@pytest.mark.parametrize("seed", [3, 5, 7])
def test_dual_rows_descend_and_follow_the_exact_trace_at_k_40(seed):
    pr, Rx, Ry = _planted(seed)
    rng = np.random.RandomState(seed + 100)
    start = [0.1 * rng.randn(n, 40) for n in (pr["m"], pr["d"], pr["p"])]
    traces = {}
    for name, kw in (("exact", dict()), ("dual", dict(dual_max=128))):
        traces[name] = [LP.objective(Rx, Ry, *start, pr["l2"])]
        LP.fit(Rx, Ry, *start, 10, pr["l2"], trace=traces[name], **kw)
    print("seed %d dual: %s" % (seed, " ".join("%.2f" % v for v in traces["dual"])))
    assert all(b <= a + 1e-9 * abs(a) for a, b in zip(traces["dual"], traces["dual"][1:]))
    assert all(abs(a - b) <= 1e-9 * abs(a) for a, b in zip(traces["exact"], traces["dual"]))
    assert A.route(True, False, 0, 0, 0, 128, shared_term=False, logistic=False, k_pad=64) == A.ROWS_DUAL     # (U reads X alone: dual rows)


# ------------------------------------------------------------------ ABI surface
def test_entry_points_are_declared():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    for name, nargs in (("cmf_set_logit_pass", 3), ("cmf_get_logit_pass", 3), ("cmf_als_logit_weights", 6)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert all(callable(getattr(_lib.Context, n)) for n in ("set_logit_pass", "get_logit_pass", "als_logit_weights"))
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(CMF_K_\w+)\s*=\s*(\d+)", header)}
    assert enum["CMF_K_COUNT"] == 11                                              # (no new kernel class: CMF_K_KLMU)
    text = header[header.index("ALS with a logistic loss on every route"):header.index("int cmf_set_logit_pass")]
    assert "CMF_EUNSUPPORTED" in text and "background weight" in text and "biases" in text and "Huber" in text and "cmf_set_problem" in text


def test_built_library_exports_the_entry_points():
    from pycmf_amd import build
    if not os.path.exists(build.LIB):
        pytest.fail("libcmfhip.so has not been built")
    blob = open(build.LIB, "rb").read()
    for name in (b"cmf_set_logit_pass", b"cmf_get_logit_pass", b"cmf_als_logit_weights", b"als_logit_pass_kernel", b"als_logit_hp_kernel"):
        assert name in blob, name
