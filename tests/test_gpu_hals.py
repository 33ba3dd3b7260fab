"""The HALS solver on the device (cmf_hals_sweep, cmf_hals_step, CMF(solver='hals')) against the float64 yardstick of
hals_yardstick.py on float32-rounded inputs.  Every comparison uses, per case,

    tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|)

with y32 / y64 the float32 / float64 yardstick on the same inputs (derivation: hals_yardstick.py); where y64 is exactly 0 and its
value before the max(0, .) lies below -tol the device value must be exactly 0.  Each test prints its worst |err| / tol."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import hals_yardstick as H

pytestmark = pytest.mark.gpu

U_, V_, Z_ = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _compare(gpu, y64, y32, k, label, raw=None):
    """|gpu - y64| <= tol everywhere; exact zeros where the yardstick's unclipped value is below -tol.  Returns |err| / tol."""
    tol = H.tolerance(y32, y64, k)
    assert gpu.shape == y64.shape and np.isfinite(gpu).all() and (gpu >= 0).all(), label
    err = float(np.max(np.abs(gpu - y64)))
    assert err <= tol, "%s: worst |err| = %.3e, tol %.3e" % (label, err, tol)
    worst = err / tol if tol > 0 else 0.0                 # (tol == 0: the yardstick is all zero, and so is the device)
    if raw is not None:
        must = (y64 == 0) & (raw < -tol)
        assert (gpu[must] == 0).all(), "%s: %d entries are not exactly 0 where the yardstick clips by more than tol" % (label, int((gpu[must] != 0).sum()))
    return worst, tol


# ------------------------------------------------------------------ 1. the sweep kernel alone
def sweep_inputs(rows, k, l1, l2, near, seed):
    """F, N, G (float32-rounded) of one sweep.  G = B^T B of a half-empty non-negative B (32 + 2 k rows) with, for k > 1, row and
    column k // 2 zero.  Fs >= 0 (40 % zeros) is the exact minimiser by construction: N = Fs (G + l2 I) + l1 - S with S >= 0 on the
    zeros of Fs only (the KKT conditions).  near: F = Fs (1 + 0.01 u), u uniform in [-1, 1] -- every step cancels to 1 % of its
    terms --, half of the zeros of Fs lifted to small positive values; else F = |N(0,1)| with 20 % exact zeros, which must revive
    where Fs > 0.  Row rows // 2 of F is zero."""
    r = np.random.RandomState(seed)
    B = np.abs(r.randn(32 + 2 * k, k)) * (r.rand(32 + 2 * k, k) < 0.5)
    dead = k // 2 if k > 1 else -1
    if dead >= 0:
        B[:, dead] = 0
    G = _f32(B.T @ B)
    Fs = np.abs(r.randn(rows, k)) * (r.rand(rows, k) < 0.6)
    S = np.abs(r.randn(rows, k)) * (Fs == 0) * G.diagonal().mean()
    N = _f32(Fs @ (G + l2 * np.eye(k)) + l1 - S)
    if near:
        F = Fs * (1 + 0.01 * (2 * r.rand(rows, k) - 1)) + 0.01 * r.rand(rows, k) * ((Fs == 0) & (r.rand(rows, k) < 0.5))
    else:
        F = np.abs(r.randn(rows, k)) * (r.rand(rows, k) < 0.8)
    F[rows // 2] = 0
    return _f32(F), N, G, dead


SWEEP_ROWS = [1, 63, 257, 300]
SWEEP_K = [1, 7, 32, 33, 40, 100, 128, 200, 256]


@pytest.mark.parametrize("near", [False, True], ids=["random", "near-minimiser"])
@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("k", SWEEP_K)
def test_sweep_kernel_against_the_yardstick(lib, k, l1, l2, near):
    """rows 1 / 63 / 257 / 300 (one row, a partial workgroup, more than one workgroup) x the k_pad boundaries and coordinate blocks
    that are partly padding.  The Jacobi variant of the yardstick (every coordinate from the old f) is further than 100 tol from
    it on these inputs, so the comparison tells the sweep order -- for k >= 2: with one coordinate the two are the same method.
    The sweep runs on U, V and Z in turn (rows 1 and 63 on V and Z)."""
    ctx = lib.Context(0)
    worst = 0.0
    for rows in SWEEP_ROWS:
        F, N, G, dead = sweep_inputs(rows, k, l1, l2, near, seed=1000 * k + rows)
        raw = np.empty_like(F)
        y64 = H.hals_sweep(F, N, G, l1, l2, unclipped=raw)
        y32 = H.hals_sweep(F, N, G, l1, l2, dtype=np.float32)
        tol = H.tolerance(y32, y64, k)
        if k >= 2:
            jac = np.max(np.abs(H.hals_sweep(F, N, G, l1, l2, jacobi=True) - y64))
            assert jac > 100 * tol, "rows %d: the Jacobi variant is only %.1f tol away" % (rows, jac / tol)
        if not near and rows > 1:
            assert ((F == 0) & (y64 > 0)).any() and (y64 == 0).any()
        which = {1: V_, 63: Z_}.get(rows, U_)
        dims = [2, 2, 2]
        dims[which] = rows
        ctx.set_problem(dims[0], dims[1], dims[2], k)
        ctx.set_factor(which, F)
        ctx.hals_sweep(which, N, G, l1, l2)
        got = ctx.get_factor(which)
        w, _ = _compare(got, y64, y32, k, "rows %d k %d" % (rows, k), raw)
        worst = max(worst, w)
        if dead >= 0 and l2 == 0:
            assert got[:, dead].tobytes() == F[:, dead].tobytes()       # zero curvature: the coordinate comes back bit-identical
        for other in range(3):                                         # the other factors (zero) are not touched
            if other != which:
                assert not ctx.get_factor(other).any()
    print("sweep k=%d l1=%g l2=%g %s: worst |err| / tol = %.3f" % (k, l1, l2, "near" if near else "random", worst))
    ctx.close()


# ------------------------------------------------------------------ 2. the full step
SHAPES = [(257, 1031, 77, 7), (300, 5000, 130, 256), (128, 3000, 150, 128), (70, 333, 129, 40), (100, 20000, 60, 16)]


@functools.lru_cache(maxsize=None)
def step_problem(m, d, p, k):
    """Data with zeros, an empty row and an empty column; factors with exact zeros and a zero row (test_gpu_wmu's)."""
    rng = np.random.RandomState(m + k)
    X, Y = (np.clip(np.abs(rng.randn(*s)) * (rng.rand(*s) < 0.8), 0, 1e3) for s in ((m, d), (d, p)))
    X[m // 3] = 0
    X[:, d // 2] = 0
    Y[d // 5] = 0
    Y[:, p // 2] = 0
    F = [np.abs(rng.randn(r, k)) * (rng.rand(r, k) < 0.9) for r in (m, d, p)]
    F[0][1] = 0
    out = _f32(X), _f32(Y), tuple(_f32(f) for f in F)
    for a in (out[0], out[1]) + out[2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def step_reference(m, d, p, k, l1, l2, mask):
    """(y64, y32, raw): both yardsticks of the step and, per swept factor 'U' / 'V' / 'Z', the float64 values before the max(0, .)"""
    X, Y, F = step_problem(m, d, p, k)
    raw = {}
    return H.hals_step(X, Y, *F, l1, l2, mask, unclipped=raw), H.hals_step(X, Y, *F, l1, l2, mask, dtype=np.float32), raw


def _context(lib, X, Y, F, sparse_x=False):
    ctx = lib.Context(0)
    if sparse_x:
        ctx.set_option("sparse_mode", 2)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], F[0].shape[1])
    ctx.set_data(0, sp.csr_matrix(X) if sparse_x else X)
    if sparse_x:
        assert ctx.data_layout(0) == (False, True)
        ctx.set_option("sparse_mode", 0)
    ctx.set_data(1, Y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    return ctx


def _check_step(ctx, m, d, p, k, l1, l2, mask, label):
    X, Y, F = step_problem(m, d, p, k)
    y64, y32, raw = step_reference(m, d, p, k, l1, l2, mask)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.hals_step(l1, l2, mask)
    worst = 0.0
    for w, bit in ((U_, 1), (V_, 2), (Z_, 4)):
        got = ctx.get_factor(w)
        if mask & bit:
            r = raw["UVZ"[w]]
            ratio, tol = _compare(got, y64[w], y32[w], k, "%s factor %d" % (label, w), r)
            # the exact-zero rule is not vacuous: every swept factor of every shape has entries the yardstick clips by more than tol
            assert ((y64[w] == 0) & (r < -tol)).any(), "%s factor %d: no entry is clipped by more than tol" % (label, w)
            worst = max(worst, ratio)
        else:
            assert got.tobytes() == F[w].tobytes(), "%s: factor %d is outside the mask and changed" % (label, w)
    return worst


@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("m, d, p, k", SHAPES)
def test_full_step_every_mask(lib, m, d, p, k, l1, l2):
    X, Y, F = step_problem(m, d, p, k)
    ctx = _context(lib, X, Y, F)
    worst = [_check_step(ctx, m, d, p, k, l1, l2, mask, "mask %d" % mask) for mask in range(1, 8)]
    print("step %s l1=%g l2=%g: worst |err| / tol per mask 1..7 = %s" % ((m, d, p, k), l1, l2, ["%.3f" % w for w in worst]))
    ctx.close()


@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
def test_full_step_with_x_as_native_csr(lib, l1, l2):
    m, d, p, k = 70, 333, 129, 40
    X, Y, F = step_problem(m, d, p, k)
    ctx = _context(lib, X, Y, F, sparse_x=True)
    worst = [_check_step(ctx, m, d, p, k, l1, l2, mask, "csr mask %d" % mask) for mask in (7, 2, 1)]
    print("step, X native CSR, l1=%g l2=%g: worst |err| / tol (masks 7, 2, 1) = %s" % (l1, l2, ["%.3f" % w for w in worst]))
    ctx.close()


# ------------------------------------------------------------------ 3. padding stays zero
def test_padding_stays_zero_under_l1(lib):
    """With l1 != 0 a sweep that touched padding rows or columns would leave max(0, -l1 / h) != 0 ... or garbage there; every other
    kernel relies on zero padding.  Three regularised HALS steps, then one MU step equals the oracle's on the pulled factors at the
    tolerance test_gpu_mu.py uses for a ragged MU step."""
    from oracle import cmf_oracle as O
    m, d, p, k = 70, 333, 129, 40
    X, Y, F = step_problem(m, d, p, k)
    ctx = _context(lib, X, Y, F)
    for _ in range(3):
        ctx.hals_step(0.05, 0.1, 7)
    Ur, Vr, Zr = (ctx.get_factor(w) for w in range(3))
    assert all(np.isfinite(a).all() and (a >= 0).all() for a in (Ur, Vr, Zr))
    ctx.mu_step(0.01, 0.02, 7)
    got = [ctx.get_factor(w) for w in range(3)]
    O.mu_update_step(np.array(X), np.array(Y), Ur, Vr, Zr, 0.01, 0.02)
    for a, b in zip(got, (Ur, Vr, Zr)):
        np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-6)
    ctx.close()


# ------------------------------------------------------------------ 4. a repeated step is bit-identical
@pytest.mark.parametrize("sparse_x", [False, True], ids=["dense", "csr"])
def test_a_repeated_step_is_bit_identical(lib, sparse_x):
    m, d, p, k = 300, 5000, 130, 256
    X, Y, F = step_problem(m, d, p, k)
    ctx = _context(lib, X, Y, F, sparse_x=sparse_x)
    runs = []
    for _ in range(2):
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.hals_step(0.01, 0.02, 7)
        ctx.hals_step(0.01, 0.02, 7)
        runs.append([ctx.get_factor(w).tobytes() for w in range(3)])
    assert runs[0] == runs[1]
    ctx.close()


# ------------------------------------------------------------------ 5. existing paths untouched
def test_existing_paths_are_untouched_by_hals_steps(lib):
    """Context a runs MU steps and residuals only; context b the same sequence with HALS steps (on other factor values, results
    thrown away) and a cmf_hals_sweep in between, the factors restored before each MU step.  mu_step from a captured graph and
    residual_sq agree byte for byte."""
    m, d, p, k = 200, 300, 90, 12
    X, Y, F = step_problem(m, d, p, k)
    a, b = _context(lib, X, Y, F), _context(lib, X, Y, F)
    other = [_f32(f * 0.5 + 0.25) for f in F]

    def reset(ctx, G):
        for w in range(3):
            ctx.set_factor(w, G[w])

    def factors(ctx):
        return [ctx.get_factor(w).tobytes() for w in range(3)]
    for ctx in (a, b):
        ctx.set_option("graph", 1)
    ra, rb = [], []
    for it in range(4):
        a.mu_step(0.01, 0.02, 7)
        ra.append(a.residual_sq())
        keep = [b.get_factor(w) for w in range(3)]
        reset(b, other)
        b.hals_step(0.05, 0.1, 7)
        b.hals_step(0.0, 0.0, 1 + (it % 7))
        b.hals_sweep(V_, np.ones((d, k)), np.eye(k), 0.0, 0.0)
        reset(b, keep)
        b.mu_step(0.01, 0.02, 7)
        rb.append(b.residual_sq())
        assert factors(b) == factors(a), "iteration %d" % it
    assert ra == rb
    a.close()
    b.close()


def test_refusals(lib):
    ctx = lib.Context(0)
    ctx.set_problem(40, 50, 30, 300)
    with pytest.raises(NotImplementedError, match="n_components <= 256"):
        ctx.hals_step(0.0, 0.0, 7)
    with pytest.raises(NotImplementedError, match="n_components <= 256"):
        ctx.hals_sweep(0, np.zeros((40, 300)), np.zeros((300, 300)), 0.0, 0.0)
    ctx.set_problem(40, 50, 30, 6)
    with pytest.raises(ValueError, match="update_mask"):
        ctx.hals_step(0.0, 0.0, 0)
    with pytest.raises(ValueError):
        ctx.hals_step(0.0, 0.0, 7)                                  # no data yet
    with pytest.raises(ValueError, match="hals_sweep"):
        ctx.hals_sweep(0, np.zeros((41, 6)), np.zeros((6, 6)), 0.0, 0.0)
    # per-entry weights bound at the C ABI: HALS has no weighted objective and does not run as if they were not there
    rng = np.random.RandomState(0)
    X, Y = _f32(np.abs(rng.randn(40, 50))), _f32(np.abs(rng.randn(50, 30)))
    F = [_f32(np.abs(rng.randn(r, 6))) for r in (40, 50, 30)]
    ctx.set_data(0, X)
    ctx.set_data(1, Y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.set_weight(0, np.ones((40, 50)))
    with pytest.raises(NotImplementedError, match="weights"):
        ctx.hals_step(0.0, 0.0, 7)
    assert all(ctx.get_factor(w).tobytes() == F[w].tobytes() for w in range(3))
    ctx.clear_weight(0)
    ctx.hals_step(0.0, 0.0, 7)                                      # the refusals left the context usable
    y64, y32 = H.hals_step(X, Y, *F), H.hals_step(X, Y, *F, dtype=np.float32)
    for w in range(3):
        _compare(ctx.get_factor(w), y64[w], y32[w], 6, "after the refusals, factor %d" % w)
    ctx.close()


# ------------------------------------------------------------------ 6. fits
def fit_inputs(seed, m=200, d=310, p=45, k=12, rank=4):
    r = np.random.RandomState(seed)
    Ut, Vt, Zt = (np.abs(r.randn(n, rank)) for n in (m, d, p))
    X = _f32(Ut @ Vt.T + .1 * np.abs(r.randn(m, d)))
    Y = _f32(Vt @ Zt.T + .1 * np.abs(r.randn(d, p)))
    U, V, Z = (_f32(np.abs(r.randn(n, k)) + .1) for n in (m, d, p))
    return X, Y, U, V, Z


def test_fit_matches_the_float64_yardstick(lib):
    from pycmf_amd import CMF
    X, Y, U, V, Z = fit_inputs(7)
    model = CMF(n_components=12, solver="hals", max_iter=30, tol=0, x_init="custom", y_init="custom")
    Ug, Vg, Zg = model.fit_transform(X, Y, U=U.copy(), V=V.copy(), Z=Z.copy())
    Ur, Vr, Zr, n_iter = H.hals_fit(X, Y, U, V, Z, max_iter=30, tol=0)
    assert model.n_iter_ == n_iter == 30
    ref = np.linalg.norm(X - Ur @ Vr.T) + np.linalg.norm(Y - Vr @ Zr.T)
    print("fit: reconstruction_err_ %.9g, yardstick %.9g, relative %.2e" % (model.reconstruction_err_, ref, abs(model.reconstruction_err_ - ref) / ref))
    assert abs(model.reconstruction_err_ - ref) <= 1e-4 * ref
    for G in (Ug, Vg, Zg):
        assert np.isfinite(G).all() and (G >= 0).all()
    # transform: V fixed, U re-fitted for new rows
    U2, V2, Z2 = model.transform(X[:50], None)
    assert V2.tobytes() == model.components.tobytes() and Z2.tobytes() == model.y_weights.tobytes()
    assert U2.shape == (50, 12) and np.isfinite(U2).all() and (U2 >= 0).all()


# (tol, seed, iteration the float64 yardstick stops at): chosen on the CPU so that (previous - error) / error_at_init stays at
# least 10 % of tol away from tol at every check up to the stop (asserted below) -- rounding cannot decide where the loop stops
STOPPING = [(1e-3, 7, 30), (3e-4, 3, 60)]   # distances to tol: 0.45 tol, 0.30 tol


@pytest.mark.parametrize("tol, seed, n_listed", STOPPING)
def test_fit_stops_at_the_yardsticks_iteration(lib, tol, seed, n_listed):
    from pycmf_amd import CMF
    X, Y, U, V, Z = fit_inputs(seed, m=60, d=90, p=20, k=5, rank=3)
    trace = []
    *_, n_ref = H.hals_fit(X, Y, U, V, Z, max_iter=200, tol=tol, trace=trace)
    margin = min(abs(t[2] - tol) for t in trace) / tol
    assert margin >= 0.1 and n_ref == n_listed, (n_ref, margin, trace)
    model = CMF(n_components=5, solver="hals", max_iter=200, tol=tol, x_init="custom", y_init="custom")
    model.fit(X, Y, U=U.copy(), V=V.copy(), Z=Z.copy())
    print("tol %g seed %d: stops at %d (yardstick %d), smallest distance to tol %.3f tol" % (tol, seed, model.n_iter_, n_ref, margin))
    assert model.n_iter_ == n_ref


# ------------------------------------------------------------------ 7. the point of it
def test_hals_after_100_iterations_beats_mu_after_200(lib):
    """The planted rank-12 problem of DESIGN section 14 (m, d, p = 300, 240, 40, noise 0.05, starts |N(0,1)|), on the device: the
    error 0.5 |X - U V^T| + 0.5 |Y - V Z^T| of HALS after 100 iterations is below MU's after 200 (float64 on the host: DESIGN
    section 14), and between the checks every 10 iterations HALS never goes up by more than 1e-6 relative."""
    X, Y, U, V, Z = (_f32(a) for a in H.planted())
    ctx = _context(lib, X, Y, [U, V, Z])

    def err():
        ex2, ey2 = ctx.residual_sq()
        return 0.5 * np.sqrt(ex2) + 0.5 * np.sqrt(ey2)
    hals = [err()]
    for it in range(100):
        ctx.hals_step(0.0, 0.0, 7)
        if (it + 1) % 10 == 0:
            hals.append(err())
    for w, F in enumerate((U, V, Z)):
        ctx.set_factor(w, F)
    for it in range(200):
        ctx.mu_step(0.0, 0.0, 7)
    mu = err()
    print("planted problem: HALS %s, MU after 200: %.3f" % (["%.3f" % e for e in hals], mu))
    assert all(b <= a * (1 + 1e-6) for a, b in zip(hals, hals[1:]))
    assert hals[-1] < mu
    ctx.close()
