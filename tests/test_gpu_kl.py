"""Kullback-Leibler multiplicative updates on the device (cmf_mu_kl_step, cmf_kl_divergence, CMF(loss='kullback-leibler')) against
the float64 yardstick of kl_yardstick.py on float32-rounded inputs.  The tolerances are derived there; EVERY element of every
updated factor is compared: exactly 0 where the yardstick is exactly 0, within tau relative elsewhere."""
import numpy as np
import pytest
import scipy.sparse as sp

import kl_yardstick as KL

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


def _problem(m, d, p, k, sparse, seed):
    """Non-zero values in [1e-3, 1e3]; zeros in the data, an empty row and an empty column; a zero factor row."""
    rng = np.random.RandomState(seed)
    if sparse:
        X, Y = rng.poisson(0.7, (m, d)).astype(float), rng.poisson(0.7, (d, p)).astype(float)
    else:
        X, Y = (np.clip(np.abs(rng.randn(*s)) * (rng.rand(*s) < 0.8), 0, 1e3) for s in ((m, d), (d, p)))
        X[(X > 0) & (X < 1e-3)] = 1e-3
        Y[(Y > 0) & (Y < 1e-3)] = 1e-3
    X[m // 3] = 0
    X[:, d // 2] = 0
    Y[d // 5] = 0
    Y[:, p // 2] = 0
    F = [np.clip(np.abs(rng.randn(r, k)), 1e-3, 1e3) for r in (m, d, p)]
    F[0][1] = 0
    X, Y, F = _f32(X), _f32(Y), [_f32(f) for f in F]
    if sparse:
        X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    return X, Y, F


def _context(lib, X, Y, F, native=False, split=0):
    ctx = lib.Context(0)
    if native:
        ctx.set_option("sparse_mode", 2)
    if split:
        ctx.set_option("kl_split", split)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], F[0].shape[1])
    if X is not None:
        ctx.set_data(0, X)
    if Y is not None:
        ctx.set_data(1, Y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    return ctx


def _check(gpu, ref, tol, label):
    """Every element: exact zero where the yardstick is exactly zero, |gpu - ref| <= tol * ref elsewhere.  Returns worst |err| / tol."""
    assert gpu.shape == ref.shape and np.isfinite(gpu).all(), label
    zero = ref == 0
    assert (gpu[zero] == 0).all(), "%s: %d elements are not exactly 0 where the yardstick is" % (label, int((gpu[zero] != 0).sum()))
    ratio = np.abs(gpu[~zero] - ref[~zero]) / (tol * ref[~zero])
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, "%s: worst |err| / tau = %.3f" % (label, worst)
    return worst


SHAPES = [(257, 1031, 77, 7), (300, 5000, 130, 256), (128, 3000, 150, 128), (70, 333, 129, 40), (100, 20000, 60, 16)]


@pytest.mark.parametrize("l1, l2", [(0.0, 0.0), (0.05, 0.1)])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("m, d, p, k", SHAPES)
def test_single_sweeps_and_the_full_step(lib, m, d, p, k, sparse, l1, l2):
    X, Y, F = _problem(m, d, p, k, sparse, seed=k + m)
    ctx = _context(lib, X, Y, F, native=sparse)
    if sparse:
        assert ctx.data_layout(0) == (False, True) and ctx.data_layout(1) == (False, True)
    lay = ctx.mu_kl_layout()
    if (m, d) == (100, 20000) and not sparse:
        assert lay[0] > 1 and lay[2] > 1, lay           # few output rows, long stream: the stream is cut into shares
    tU = tZ = KL.tau(k, d)
    tV = KL.tau(k, m + p)
    for mask, name in ((KL.V_BIT, "V"), (KL.U_BIT, "U"), (KL.Z_BIT, "Z"), (7, "full")):
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.mu_kl_step(l1, l2, mask)
        got = [ctx.get_factor(w) for w in range(3)]
        ref = KL.step(X, Y, F[0], F[1], F[2], l1, l2, mask)
        full = mask == 7
        tols = (tU + 3 * tV if full else tU, tV, tZ + 3 * tV if full else tZ)
        worst = []
        for w, bit in ((U_, KL.U_BIT), (V_, KL.V_BIT), (Z_, KL.Z_BIT)):
            if mask & bit:
                worst.append(_check(got[w], ref[w], tols[w], "%s sweep, factor %d" % (name, w)))
            else:
                assert got[w].tobytes() == F[w].tobytes()
        print("(%d, %d, %d, k=%d) %s l1=%g l2=%g %s: shares %s, worst |err| / tau = %s"
              % (m, d, p, k, "csr" if sparse else "dense", l1, l2, name, lay[:3], ["%.4f" % x for x in worst]))
    if sparse:
        assert ctx.data_layout(0) == (False, True) and ctx.data_layout(1) == (False, True)
    ctx.close()


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("m, d, p, k", SHAPES)
def test_divergence(lib, m, d, p, k, sparse):
    X, Y, F = _problem(m, d, p, k, sparse, seed=3 * k + 1)
    ctx = _context(lib, X, Y, F, native=sparse)
    dx, dy = ctx.kl_divergence()
    for name, got, (T, A, B) in (("x", dx, (X, F[0], F[1])), ("y", dy, (Y, F[1], F[2]))):
        st, ss, sl, sa = KL.divergence_terms(T, A, B)
        ref, tol = sl - st + ss, KL.div_tol(k, st, ss, sa)
        print("(%d, %d, %d, k=%d) %s D_%s: |err| / tol = %.4f" % (m, d, p, k, "csr" if sparse else "dense", name, abs(got - ref) / tol))
        assert abs(got - ref) <= tol
    assert ctx.kl_divergence(True, False)[0] == dx and ctx.kl_divergence(False, True) == (0.0, dy)
    if sparse:
        assert ctx.data_layout(0) == (False, True) and ctx.data_layout(1) == (False, True)   # no dense expansion
    ctx.close()


@pytest.mark.parametrize("k", [7, 100, 200])
@pytest.mark.parametrize("dense_owner", ["V", "UZ"])
def test_exact_arithmetic_pins_the_orientation_and_the_k_pairing(lib, k, dense_owner):
    """Every product A_r . B_c is a power of two (one factor of each pair has one-hot rows, all entries are powers of two) and T is
    that product times a power of two, so every quotient, every term and every sum is exact in float32 whatever the order: the
    result is determined bit for bit.  The factors are asymmetric (no two rows or columns alike), so a slip in the k pairing of
    the two products, in the transposed access or in the output column map changes it."""
    m, d, p = 70, 333, 40
    rng = np.random.RandomState(k)

    def dense(r):
        return 2.0 ** rng.randint(0, 4, size=(r, k))

    def onehot(r):
        F = np.zeros((r, k))
        F[np.arange(r), rng.randint(0, k, size=r)] = 2.0 ** rng.randint(0, 3, size=r)
        return F
    F = [onehot(m), dense(d), onehot(p)] if dense_owner == "V" else [dense(m), onehot(d), dense(p)]
    X = (F[0] @ F[1].T) * 2.0 ** rng.randint(-2, 3, size=(m, d)) * (rng.rand(m, d) < 0.7)
    Y = (F[1] @ F[2].T) * 2.0 ** rng.randint(-2, 3, size=(d, p)) * (rng.rand(d, p) < 0.7)
    f32 = np.float32

    def expect(Fw, num, den):
        den = np.broadcast_to(den, num.shape).astype(f32).copy()
        den[den == 0] = f32(KL.EPS)
        return (Fw.astype(f32) * (num.astype(f32) / den)).astype(np.float64)
    for native in (False, True):
        ctx = _context(lib, sp.csr_matrix(X) if native else X, sp.csr_matrix(Y) if native else Y, F, native=native)
        # V from the old U, Z
        ctx.mu_kl_step(0.0, 0.0, KL.V_BIT)
        numV = KL.numerator_t(X, F[0], F[1]) + KL.numerator(Y, F[1], F[2])
        Vn = expect(F[1], numV, F[0].sum(axis=0) + F[2].sum(axis=0))
        assert (ctx.get_factor(V_) == Vn).all()
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.mu_kl_step(0.0, 0.0, KL.U_BIT | KL.Z_BIT)
        assert (ctx.get_factor(U_) == expect(F[0], KL.numerator(X, F[0], F[1]), F[1].sum(axis=0))).all()
        assert (ctx.get_factor(Z_) == expect(F[2], KL.numerator_t(Y, F[1], F[2]), F[1].sum(axis=0))).all()
        ctx.close()


@pytest.mark.parametrize("sparse, split", [(False, 1), (False, 0), (False, 3), (True, 0)])
def test_a_repeated_step_is_bit_identical(lib, sparse, split):
    m, d, p, k = 300, 2100, 130, 40
    X, Y, F = _problem(m, d, p, k, sparse, seed=9)
    ctx = _context(lib, X, Y, F, native=sparse, split=split)
    lay = ctx.mu_kl_layout()
    if not sparse:
        assert (lay[0] == 1) == (split == 1) and (split != 3 or lay[0] == 3), lay
    runs = []
    for _ in range(2):
        for w in range(3):
            ctx.set_factor(w, F[w])
        ctx.mu_kl_step(0.01, 0.02, 7)
        ctx.mu_kl_step(0.01, 0.02, 7)
        runs.append([ctx.get_factor(w).tobytes() for w in range(3)] + [np.array(ctx.kl_divergence()).tobytes()])
    assert runs[0] == runs[1]
    # another share count regroups float32 sums: still within the tolerance of the yardstick (checked for split = 0 above)
    ctx.close()


def _fit_inputs(seed, m=60, d=90, p=20, k=5):
    rng = np.random.RandomState(seed)
    X, Y = rng.poisson(1.0, (m, d)).astype(float), rng.poisson(1.0, (d, p)).astype(float)
    U, V, Z = (_f32(np.abs(rng.randn(n, k)) + 0.1) for n in (m, d, p))
    return X, Y, U, V, Z


@pytest.mark.parametrize("sparse", [False, True])
def test_fit_matches_the_float64_yardstick(lib, sparse, monkeypatch):
    from pycmf_amd import CMF
    if sparse:
        monkeypatch.setenv("PYCMF_AMD_SPARSE_MODE", "native")
    X, Y, U, V, Z = _fit_inputs(7, m=200, d=310, p=45, k=12)
    Xi, Yi = (sp.csr_matrix(X), sp.csr_matrix(Y)) if sparse else (X, Y)
    model = CMF(n_components=12, solver="mu", loss="kullback-leibler", max_iter=20, tol=0, x_init="custom", y_init="custom")
    Ug, Vg, Zg = model.fit_transform(Xi, Yi, U=U.copy(), V=V.copy(), Z=Z.copy())
    Ur, Vr, Zr, n_iter, _ = KL.fit(X, Y, U, V, Z, 20, 0)
    assert model.n_iter_ == n_iter == 20
    ref = sum(KL.errors(X, Y, Ur, Vr, Zr))
    print("fit %s: reconstruction_err_ %.9g, yardstick %.9g, relative %.2e" % ("csr" if sparse else "dense", model.reconstruction_err_, ref,
                                                                              abs(model.reconstruction_err_ - ref) / ref))
    assert abs(model.reconstruction_err_ - ref) <= 1e-4 * ref
    for G, R in ((Ug, Ur), (Vg, Vr), (Zg, Zr)):
        assert np.isfinite(G).all() and (G >= 0).all() and np.abs(G - R).max() <= 1e-3 * np.abs(R).max()
    # per-iteration divergence through the C ABI: non-increasing up to twice the divergence tolerance
    ctx = _context(lib, Xi, Yi, [U, V, Z], native=sparse)
    prev = sum(ctx.kl_divergence())
    for it in range(20):
        ctx.mu_kl_step(0.0, 0.0, 7)
        F = [ctx.get_factor(w) for w in range(3)]
        tol = sum(KL.div_tol(12, *KL.divergence_terms(T, A, B)[:2], KL.divergence_terms(T, A, B)[3]) for T, A, B in ((X, F[0], F[1]), (Y, F[1], F[2])))
        cur = sum(ctx.kl_divergence())
        assert cur <= prev + 2 * tol, (it, prev, cur, tol)
        prev = cur
    ctx.close()
    # transform: V fixed, U re-fitted
    U2, V2, Z2 = model.transform(Xi, None)
    assert V2.tobytes() == model.components.tobytes() and Z2.tobytes() == model.y_weights.tobytes()
    assert U2.shape == Ug.shape and np.isfinite(U2).all() and (U2 >= 0).all()
    idx, val = model.top_n("x", n=3)
    assert idx.shape == (200, 3) and np.isfinite(val).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fit_stops_at_the_yardsticks_iteration(lib, seed):
    from pycmf_amd import CMF
    tol = 3e-3
    X, Y, U, V, Z = _fit_inputs(seed)
    _, _, _, n_ref, ratios = KL.fit(X, Y, U, V, Z, 200, tol, alpha=0.5)
    # the yardstick alone must be far from the crossing at every check, or rounding would decide the test
    margin = min(abs(r - tol) for r in ratios) / tol
    assert margin >= 0.2 and n_ref == 40, (n_ref, margin)
    model = CMF(n_components=5, solver="mu", loss="kullback-leibler", max_iter=200, tol=tol, x_init="custom", y_init="custom")
    model.fit(X, Y, U=U.copy(), V=V.copy(), Z=Z.copy())
    print("seed %d: stops at %d (yardstick %d), smallest distance to tol %.3f tol" % (seed, model.n_iter_, n_ref, margin))
    assert model.n_iter_ == n_ref


def test_frobenius_path_is_untouched_by_a_kl_step(lib):
    m, d, p, k = 200, 300, 90, 12
    X, Y, F = _problem(m, d, p, k, False, seed=41)
    a, b = _context(lib, X, Y, F), _context(lib, X, Y, F)
    for ctx in (a, b):
        ctx.set_option("graph", 1)
    for _ in range(3):
        a.mu_step(0.0, 0.0, 7)
    ra = a.residual_sq()
    for _ in range(3):                   # b: the same Frobenius steps first (its step graph is captured), then KL work in between
        b.mu_step(0.0, 0.0, 7)
    assert [b.get_factor(w).tobytes() for w in range(3)] == [a.get_factor(w).tobytes() for w in range(3)]
    for ctx in (a, b):
        for w in range(3):
            ctx.set_factor(w, F[w])
    b.mu_kl_step(0.0, 0.0, 7)
    b.kl_divergence()
    for w in range(3):
        b.set_factor(w, F[w])
    for _ in range(3):
        a.mu_step(0.0, 0.0, 7)
        b.mu_step(0.0, 0.0, 7)
    assert [b.get_factor(w).tobytes() for w in range(3)] == [a.get_factor(w).tobytes() for w in range(3)]
    assert b.residual_sq() == a.residual_sq() == ra
    a.close()
    b.close()


def test_refusals_leave_the_context_usable(lib):
    rng = np.random.RandomState(5)
    ctx = lib.Context(0)
    ctx.set_problem(40, 50, 30, 300)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.mu_kl_step(0.0, 0.0, 7)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.kl_divergence()
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.mu_kl_layout()
    X, Y, F = _problem(40, 50, 30, 6, False, seed=2)
    ctx.set_problem(40, 50, 30, 6)
    for w in range(3):
        ctx.set_factor(w, F[w])
    with pytest.raises(ValueError, match="X has not been set"):
        ctx.mu_kl_step(0.0, 0.0, 7)
    with pytest.raises(ValueError, match="X has not been set"):
        ctx.kl_divergence()
    ctx.set_data(0, X)
    with pytest.raises(ValueError, match="Y has not been set"):
        ctx.mu_kl_step(0.0, 0.0, KL.Z_BIT)
    ctx.mu_kl_step(0.0, 0.0, KL.U_BIT)                    # the X side alone serves a U sweep
    _check(ctx.get_factor(U_), KL.step(X, Y, *F, mask=KL.U_BIT)[0], KL.tau(6, 50), "U sweep without Y")
    ctx.set_data(1, Y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.mu_kl_step(0.0, 0.0, 7)
    ref = KL.step(X, Y, *F)
    _check(ctx.get_factor(V_), ref[1], KL.tau(6, 70), "V after the refusals")
    ctx.close()
    del rng


def test_full_size_c4_step(lib):
    """C4's shape: one full step on synthetic |N(0,1)| data and factors; 16 rows of each factor recomputed in float64 from what the
    device holds (data blocks, the factors before the step; U and Z from the V the step produced)."""
    m = d = 65536
    p, k = 256, 256
    ctx = lib.Context(0)
    ctx.set_problem(m, d, p, k)
    ctx.fill_data_synthetic(0, 11)
    ctx.fill_data_synthetic(1, 12)
    for w in range(3):
        ctx.fill_factor_synthetic(w, 20 + w)
    lay = ctx.mu_kl_layout()
    mp, dp, _, _ = ctx.geometry()
    assert lay[3] < 0.01 * 4.0 * mp * dp, lay
    assert lay[2] > 1, lay                                   # Z: two row blocks for 256 CUs
    U0, V0, Z0 = (ctx.get_factor(w) for w in range(3))
    ctx.mu_kl_step(0.0, 0.0, 7)
    U1, V1, Z1 = (ctx.get_factor(w) for w in range(3))
    rng = np.random.RandomState(0)
    E = KL.EPS
    den = U0.sum(axis=0) + Z0.sum(axis=0)
    worst = [0.0, 0.0, 0.0]
    for c in rng.choice(d, 16, replace=False):
        x = ctx.get_data_block(0, 0, m, int(c), 1)[:, 0].astype(np.float64)
        y = ctx.get_data_block(1, int(c), 1, 0, p)[0].astype(np.float64)
        num = (x / np.maximum(U0 @ V0[c], E)) @ U0 + (y / np.maximum(Z0 @ V0[c], E)) @ Z0
        ref = V0[c] * (num / np.where(den == 0, E, den))
        worst[1] = max(worst[1], _check(V1[c], ref, KL.tau(k, m + p), "V row %d" % c))
    den = V1.sum(axis=0)
    den = np.where(den == 0, E, den)
    for r in rng.choice(m, 16, replace=False):
        x = ctx.get_data_block(0, int(r), 1, 0, d)[0].astype(np.float64)
        ref = U0[r] * (((x / np.maximum(V1 @ U0[r], E)) @ V1) / den)
        worst[0] = max(worst[0], _check(U1[r], ref, KL.tau(k, d), "U row %d" % r))
    for r in rng.choice(p, 16, replace=False):
        y = ctx.get_data_block(1, 0, d, int(r), 1)[:, 0].astype(np.float64)
        ref = Z0[r] * (((y / np.maximum(V1 @ Z0[r], E)) @ V1) / den)
        worst[2] = max(worst[2], _check(Z1[r], ref, KL.tau(k, d), "Z row %d" % r))
    print("C4 full step: shares %s, scratch %.1f MB, worst |err| / tau U %.4f V %.4f Z %.4f" % (lay[:3], lay[3] / 2 ** 20, *worst))
    ctx.close()
