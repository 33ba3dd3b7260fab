"""The ALS solver's logistic loss without a device: the validation of loss='logistic' (every refusal, by message, before any device
is touched), the Jaakkola-Jordan bound itself, and the monotone descent, the recovery and the quality of the NumPy yardstick
(logit_yardstick.py) on the planted problem -- the numbers the device tests are held to."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
import logit_yardstick as L
from pycmf_amd import CMF
from pycmf_amd import solver_shell as S

SEEDS = (3, 5, 7)
SIGNED = dict(U_non_negative=False, V_non_negative=False, Z_non_negative=False)


# ------------------------------------------------------------------ validation
def test_losses_names_logistic():
    assert "logistic" in S.ALS_LOSSES and "logistic" in S.ALL_LOSSES
    with pytest.raises(ValueError, match="Invalid loss parameter.*'logistic'"):
        S.check_loss("hinge", "als")
    S.check_loss("logistic", "als", 1)
    S.check_als(loss="logistic")
    S.check_als(loss="frobenius")


@pytest.mark.parametrize("solver", ["mu", "newton", "hals"])
def test_logistic_needs_the_als_solver(solver):
    with pytest.raises(ValueError, match="loss='logistic' is implemented by the alternating-least-squares solver only: solver='als'"):
        S.check_loss("logistic", solver)


def test_logistic_needs_one_gpu():
    with pytest.raises(ValueError, match="loss='logistic' runs on one GPU"):
        S.check_loss("logistic", "als", 2)


def test_als_refuses_the_other_losses():
    with pytest.raises(ValueError, match="loss must be 'frobenius' or 'logistic'"):
        S.check_als(loss="kullback-leibler")


def _data(seed=0):
    rng = np.random.RandomState(seed)
    X = sp.csr_matrix((rng.rand(12, 9) < 0.5) * 1.0)
    Y = rng.rand(9, 5)
    return X, Y


def _fit(X, Y, fit_kw=None, **kw):
    args = dict(n_components=3, solver="als", loss="logistic", l2_reg=0.5, max_iter=2, x_link="logit", random_state=0, **SIGNED)
    args.update(kw)
    return CMF(**args).fit(X, Y, **(fit_kw or {}))


def test_a_logit_link_is_required():
    X, Y = _data()
    with pytest.raises(ValueError, match="x_link or y_link must be 'logit'"):
        _fit(X, Y, dict(x_entry_weights="observed"), x_link="linear")


def test_a_logistic_relation_needs_sparse_weights():
    X, Y = _data()
    with pytest.raises(ValueError, match="needs x_entry_weights that name the observed entries.*got None"):
        _fit(X, Y)
    with pytest.raises(ValueError, match="needs x_entry_weights that name the observed entries.*got a dense array"):
        _fit(X, Y, dict(x_entry_weights=np.ones(X.shape)))
    with pytest.raises(ValueError, match="needs y_entry_weights that name the observed entries"):
        _fit(X, Y, dict(x_entry_weights="observed"), y_link="logit")


def test_targets_must_lie_in_the_unit_interval():
    X, Y = _data()
    with pytest.raises(ValueError, match=r"targets in \[0, 1\]: the observed entries of X"):
        _fit(2.0 * X, Y, dict(x_entry_weights="observed"))
    with pytest.raises(ValueError, match=r"targets in \[0, 1\]: the observed entries of X"):
        _fit(-1.0 * X, Y, dict(x_entry_weights="observed"))
    S.check_logistic_data([0.0, 0.25, 1.0], "X")     # soft labels pass


def test_cg_background_and_biases_are_refused():
    X, Y = _data()
    W = sp.csr_matrix(X.toarray() + 1.0)
    with pytest.raises(ValueError, match="als_cg_steps=6 with loss='logistic' is not built"):
        _fit(X, Y, dict(x_entry_weights="observed"), als_cg_steps=6)
    with pytest.raises(ValueError, match="x_background_weight=1.0 on a logistic relation"):
        _fit(X, Y, dict(x_entry_weights=W, x_background_weight=1.0))
    with pytest.raises(ValueError, match="x_biases=True on a logistic relation"):
        _fit(X, Y, dict(x_entry_weights="observed", x_biases=True))


def test_the_solver_object_refuses_too():
    with pytest.raises(ValueError, match="x_link or y_link must be 'logit'"):
        S.HipALSSolver(l2_reg=0.5, loss="logistic")
    with pytest.raises(ValueError, match="is not built"):
        S.HipALSSolver(l2_reg=0.5, loss="logistic", x_link="logit", x_entry_weights="observed", cg_steps=3, **SIGNED)
    s = S.HipALSSolver(l2_reg=0.5, loss="logistic", x_link="logit", x_entry_weights=np.ones((12, 9)), **SIGNED)
    X, Y = _data()
    with pytest.raises(ValueError, match="got a dense array"):
        s.check_weights(X.toarray(), Y)


def test_frobenius_als_keeps_its_link_warning():
    X, Y = _data()
    with pytest.warns(UserWarning, match="als solver does not accept link functions other than linear"):
        with pytest.raises(ValueError, match="x_entry_weights='observed' needs a SciPy sparse"):   # (the next refusal: no device needed)
            CMF(n_components=3, solver="als", l2_reg=0.5, x_link="logit").fit(X.toarray(), Y, x_entry_weights="observed")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="got None"):      # loss='logistic' reads the links: no warning on the way to its refusal
            _fit(X, Y)


# ------------------------------------------------------------------ the bound
def test_the_bound_majorises_and_touches():
    rng = np.random.RandomState(0)
    s, xi, t = 12.0 * rng.randn(10000), 12.0 * rng.randn(10000), rng.rand(10000)
    xi[:100] = 0.0                                    # the guard of kappa
    xi[100:200] = 1e-5 * rng.randn(100)
    gap = L.bound(s, xi, t) - L.pointwise(s, t)
    assert gap.min() >= -1e-12 * np.maximum(1.0, np.abs(L.pointwise(s, t))).max()
    assert np.abs(L.bound(xi, xi, t) - L.pointwise(xi, t)).max() <= 1e-12
    assert np.abs(L.bound(-xi, xi, 0.5) - L.pointwise(-xi, 0.5)).max() <= 1e-12    # and at -xi (t = 1/2: the symmetric part)


def test_kappa():
    assert L.kappa(0.0) == 0.25 and L.kappa(5e-5) == 0.25
    s = np.array([1e-3, 0.5, -0.5, 30.0, -30.0])
    np.testing.assert_allclose(L.kappa(s), np.tanh(s / 2) / (2 * s), rtol=1e-15)
    assert (L.kappa(s) > 0).all() and (L.kappa(s) <= 0.25).all()
    assert L.kappa(np.float32(0.3), np.float32).dtype == np.float32


# ------------------------------------------------------------------ the planted problem
_RUNS = {}


def _run(seed, nn=False):
    """15 float64 iterations on the planted problem: (problem, objective trace incl. the start, U, V, Z)."""
    key = (seed, nn)
    if key not in _RUNS:
        pr = L.planted(seed)
        Rx, Ry = L.Relation(pr["T"], pr["Wsp"]), L.Relation(pr["Y"], None)
        U, V, Z = (np.abs(F) if nn else F.copy() for F in pr["start"])
        trace = [L.objective(Rx, Ry, None, None, U, V, Z, pr["l2"])]
        for _ in range(15):
            U, V, Z = L.step(Rx, Ry, None, None, U, V, Z, pr["l2"], nn_mask=7 if nn else 0, nn_sweeps=4 if nn else 0)
            trace.append(L.objective(Rx, Ry, None, None, U, V, Z, pr["l2"]))
        _RUNS[key] = (pr, trace, U, V, Z)
    return _RUNS[key]


@pytest.mark.parametrize("seed", SEEDS)
def test_descent_and_recovery_signed(seed):
    pr, trace, U, V, Z = _run(seed)
    print("seed %d objective %s" % (seed, " ".join("%.1f" % j for j in trace)))
    for a, b in zip(trace, trace[1:]):
        assert b <= a + 1e-9 * abs(a)
    agree = L.agreement(U, V, pr)
    print("seed %d agreement on the unobserved cells %.3f" % (seed, agree))
    assert agree >= 0.85


@pytest.mark.parametrize("seed", SEEDS)
def test_descent_non_negative(seed):
    """All factors non-negative, nn_sweeps = 4: descent only (the agreement is recorded in the README, no threshold)."""
    pr, trace, U, V, Z = _run(seed, nn=True)
    assert min(F.min() for F in (U, V, Z)) >= 0
    for a, b in zip(trace, trace[1:]):
        assert b <= a + 1e-9 * abs(a)
    print("seed %d non-negative: objective %.1f -> %.1f, agreement %.3f" % (seed, trace[0], trace[-1], L.agreement(U, V, pr)))


@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_float32_descent(seed, nn):
    """The yardstick's float32 mode, 8 iterations: J_{t+1} <= J_t + (k + 16) 2^-24 |J_t| -- the condition the device test reuses."""
    pr = L.planted(seed)
    Rx, Ry = L.Relation(pr["T"], pr["Wsp"]), L.Relation(pr["Y"], None)
    U, V, Z = (np.abs(F) if nn else F.copy() for F in pr["start"])
    j = L.objective(Rx, Ry, None, None, U, V, Z, pr["l2"])
    for _ in range(8):
        U, V, Z = L.step(Rx, Ry, None, None, U, V, Z, pr["l2"], nn_mask=7 if nn else 0, nn_sweeps=4 if nn else 0, dtype=np.float32)
        jn = L.objective(Rx, Ry, None, None, U, V, Z, pr["l2"])
        assert jn <= j + (pr["k"] + 16) * 2.0 ** -24 * abs(j)
        j = jn


@pytest.mark.parametrize("seed", SEEDS)
def test_logistic_beats_least_squares_on_held_out_log_loss(seed):
    """Held-out log-loss of the logistic fit beside a Frobenius ALS fit of the same 0/1 data (predictions clipped to
    [1e-6, 1 - 1e-6]), both 15 iterations from the same start with the same weights."""
    pr, _, U, V, Z = _run(seed)
    Rx, Ry = A.Relation(pr["T"], pr["Wsp"]), A.Relation(pr["Y"], None)
    Uf, Vf, Zf = (F.copy() for F in pr["start"])
    for _ in range(15):
        Uf, Vf, Zf = A.step(Rx, Ry, None, None, Uf, Vf, Zf, pr["l2"])
    off, T = ~pr["M"], pr["T"]

    def log_loss(Pr):
        Pr = np.clip(Pr, 1e-6, 1 - 1e-6)
        return float(-(T * np.log(Pr) + (1 - T) * np.log(1 - Pr))[off].mean())
    ll, lf = log_loss(L.sigmoid(U @ V.T)), log_loss(Uf @ Vf.T)
    print("seed %d held-out log-loss: logistic %.4f, least squares %.4f" % (seed, ll, lf))
    assert ll < lf


def test_mixed_v_sweep_system_matches_the_frobenius_yardstick_on_its_side():
    """X logistic + Y observed Frobenius: the V systems are the logistic X part plus als_yardstick's Y part."""
    pr = L.planted(3)
    rng = np.random.RandomState(1)
    Wy = sp.csr_matrix((rng.rand(pr["d"], pr["p"]) < 0.5) * (0.5 + rng.rand(pr["d"], pr["p"])))
    U, V, Z = pr["start"]
    l2 = pr["l2"]
    Rx, Ry = L.Relation(pr["T"], pr["Wsp"]), L.Relation(pr["Y"], Wy)
    H, g = L.systems(Rx, Ry, U, V, Z, "V", l2, logit=(True, False))
    Hx, gx = L.systems(Rx, L.Relation(np.zeros_like(pr["Y"]), sp.csr_matrix(Wy.shape)), U, V, Z, "V", l2, logit=(True, False))
    Hy, gy = A.systems(A.Relation(np.zeros_like(pr["T"]), sp.csr_matrix(pr["T"].shape)), Ry, U, V, Z, "V", l2)
    eye = l2 * np.eye(pr["k"])
    np.testing.assert_allclose(H, Hx + Hy - eye, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g, gx + gy, rtol=1e-12, atol=1e-12)
