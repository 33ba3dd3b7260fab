"""The ALS solver's logistic loss on the device (cmf_set_relation_loss, cmf_als_normal / cmf_als_step / cmf_als_nnls_step on a
logistic relation, cmf_als_logistic_loss, CMF(solver="als", loss="logistic")) against the float64 yardstick of logit_yardstick.py on
float32-rounded inputs.  Tolerances are als_yardstick.tolerance, the project's rule: tol = max(4 max|y32 - y64|,
(k + 16) 2^-24 max|y64|) with y32 the yardstick's float32 mode.

The kernel-level pattern is 40 x 80, not the 40 x 50 the feature request names: it also asks for a row of 70 stored entries, which
50 columns cannot hold; 80 columns do, and every listed case is kept."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
import logit_yardstick as L

pytestmark = pytest.mark.gpu

U_, V_, Z_ = 0, 1, 2
M_, D_, P_ = 40, 80, 20
L2 = 0.5
KS = [3, 40, 100, 200]          # k_pad 32 / 64 / 128 / 256: one k per template


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _pattern():
    """(T, W) 40 x 80: row 0 empty, row 1 one entry, rows 2 / 3 of 32 / 33 entries (the tile edge), row 4 of 70 entries (three pieces
    under als_piece = 32, the last one ragged), the rest 5 .. 45 entries; targets 0 / 1 with a few soft labels, weights in
    [0.5, 2.5); a stored t = 0 under w > 0 (row 1) and a stored entry with w = 0 (row 2)."""
    rng = np.random.RandomState(11)
    lengths = [0, 1, 32, 33, 70] + list(rng.randint(5, 46, size=M_ - 5))
    indptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    indices = np.concatenate([np.sort(rng.permutation(D_)[:n]) for n in lengths]).astype(np.int32)
    nnz = int(indptr[-1])
    t = (rng.rand(nnz) < 0.5).astype(np.float64)
    soft = rng.rand(nnz) < 0.1
    t[soft] = _f32(rng.rand(int(soft.sum())))
    w = _f32(0.5 + 2.0 * rng.rand(nnz))
    t[indptr[1]] = 0.0                      # the one entry of row 1: a stored zero that counts
    w[indptr[2] + 3] = 0.0                  # a stored entry without weight
    W = sp.csr_matrix((w, indices, indptr), shape=(M_, D_))
    T = np.zeros((M_, D_))
    r = np.repeat(np.arange(M_), lengths)
    T[r, indices] = t
    return T, W


def _factors(k, seed=0):
    """Scores of order 1; row 5 of U all zeros (s = 0: the guard of kappa), row 6 scaled to |s| ~ 30 (saturated kappa); column 7 of
    X (a row of the V sweep) scaled likewise."""
    rng = np.random.RandomState(100 + k + seed)
    sc = k ** -0.25
    U, V, Z = (_f32(sc * rng.randn(n, k)) for n in (M_, D_, P_))
    _, W = _pattern()
    U[5] = 0.0
    cols = W.indices[W.indptr[6]:W.indptr[7]]
    U[6] = _f32(U[6] * 30.0 / np.abs(V[cols] @ U[6]).max())
    rows = sp.csc_matrix(W).indices[sp.csc_matrix(W).indptr[7]:sp.csc_matrix(W).indptr[8]]
    rows = rows[rows != 6]
    V[7] = _f32(V[7] * 30.0 / np.abs(U[rows] @ V[7]).max())
    return [U, V, Z]


def _y(kind):
    """(Y, Wy): a full dense Y, or a Frobenius-observed one."""
    rng = np.random.RandomState(5)
    Y = _f32(rng.randn(D_, P_))
    if kind == "full":
        return Y, None
    Wy = sp.csr_matrix(_f32((rng.rand(D_, P_) < 0.4) * (0.5 + rng.rand(D_, P_))))
    return Y, Wy


def _bind_csr(ctx, which, T, W):
    W = sp.csr_matrix(W)
    r = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
    ctx.set_weighted_csr(which, W.indptr, W.indices, np.asarray(T)[r, W.indices], W.data)


def _context(lib, T, W, Y, Wy, F, piece=32, logit=(True, False)):
    ctx = lib.Context(0)
    if piece:
        ctx.set_option("als_piece", piece)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], F[0].shape[1])
    _bind_csr(ctx, 0, T, W)
    if Wy is None:
        ctx.set_data(1, Y)
    else:
        _bind_csr(ctx, 1, Y, Wy)
    for which, on in enumerate(logit):
        if on:
            ctx.set_relation_loss(which, "logistic")
    for w in range(3):
        ctx.set_factor(w, F[w])
    return ctx


def _close(name, got, y32, y64, k):
    tol = A.tolerance(y32, y64, k)
    err = float(np.max(np.abs(np.asarray(got, np.float64) - y64)))
    print("%s k=%d: max error %.3e, tolerance %.3e" % (name, k, err, tol))
    assert err <= tol, "%s, k = %d: %.3e > %.3e" % (name, k, err, tol)


# ------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("ykind", ["full", "observed"])
@pytest.mark.parametrize("k", KS)
def test_normal_equations(lib, k, ykind):
    """cmf_als_normal returns the majoriser's system at the current rows: the U sweep (X logistic) and the V sweep (X logistic
    beside a full or a Frobenius-observed Y) in one context."""
    T, W = _pattern()
    Y, Wy = _y(ykind)
    F = _factors(k)
    Rx, Ry = L.Relation(T, W), L.Relation(Y, Wy)
    ctx = _context(lib, T, W, Y, Wy, F)
    assert ctx.als_layout()[1] == sum(-(-int(n) // 32) for n in np.diff(W.indptr))      # 33 entries -> 2 pieces, 70 -> 3
    for which, name in ((U_, "U"), (V_, "V")):
        if name == "U" and ykind == "observed":
            continue                                        # (the U sweep does not read Y: covered by the other case)
        n = F[which].shape[0]
        H, g = ctx.als_normal(which, 0, n, L2)
        H64, g64 = L.systems(Rx, Ry, *F, name, L2)
        H32, g32 = L.systems(Rx, Ry, *F, name, L2, dtype=np.float32)
        _close("H of the %s sweep, Y %s" % (name, ykind), H[:, :k, :k], H32, H64, k)
        _close("g of the %s sweep, Y %s" % (name, ykind), g[:, :k], g32, g64, k)
        pad = H.copy()
        pad[:, :k, :k] = 0
        idx = np.arange(k, H.shape[1])
        assert (pad[:, idx, idx] == 1).all() and pad.sum() == n * (H.shape[1] - k) and (g[:, k:] == 0).all()
        assert (H == np.transpose(H, (0, 2, 1))).all()
        H2, g2 = ctx.als_normal(which, 0, n, L2)            # a repeated call: the same bits
        assert (H2 == H).all() and (g2 == g).all()
        if name == "U":
            assert (H[0, :k, :k] == np.float32(L2) * np.eye(k, dtype=np.float32)).all() and (g[0] == 0).all()   # the empty row
            # the all-zero row sees kappa = 1/4 exactly: its matrix is the Frobenius one under the weights w / 4
            Hq, _ = A.systems(A.Relation(T, W * 0.25), Ry, *F, "U", L2, rows=[5])
            assert np.max(np.abs(H[5, :k, :k] - Hq[0])) <= A.tolerance(H32[5], H64[5], k)
    ctx.close()


def test_frobenius_relations_keep_their_kernel(lib):
    """Without a logistic relation cmf_als_normal returns the bits it returns when the relation loss was never touched, and a
    relation set back to Frobenius does too."""
    T, W = _pattern()
    Y, Wy = _y("observed")
    F = _factors(40)
    ctx = _context(lib, T, W, Y, Wy, F, logit=(False, False))
    H0, g0 = ctx.als_normal(V_, 0, D_, L2)
    ctx.set_relation_loss(0, "logistic")
    assert ctx.get_relation_loss(0) == 1 and ctx.get_relation_loss(1) == 0
    H1, _ = ctx.als_normal(V_, 0, D_, L2)
    assert not (H1 == H0).all()
    ctx.set_relation_loss(0, "frobenius")
    H2, g2 = ctx.als_normal(V_, 0, D_, L2)
    assert (H2 == H0).all() and (g2 == g0).all()
    ctx.close()


@pytest.mark.parametrize("ykind", ["observed", "long rows"])
@pytest.mark.parametrize("k", [40, 200])                    # k_pad 64 / 256: both wave maps
def test_frobenius_side_of_a_mixed_launch_is_the_frobenius_kernel(lib, k, ykind):
    """The V sweep reads X and a Frobenius-observed Y in one launch.  With every stored weight of X zero, a logistic X contributes
    sqrt(0 kappa) = 0 and p - 0.5 * 0 = 0 and a Frobenius X sqrt(0) = 0 and p = 0: X's pieces add exact zeros in the same piece order
    either way, and the two systems are the same object (held in float64 first).  Y's pieces went through the instance with the
    reweighting compiled in (its per-side flag off) in one call and through the instance without it in the other: the same bits.
    "observed": the file's Y, whose rows hold at most 14 entries (one piece each); "long rows": an 80 x 80 Y with the rows of the
    file's pattern, twice -- 0, 1, 32, 33 and 70 entries, the tile edge and a ragged third piece under als_piece = 32."""
    T, W = _pattern()
    W0 = sp.csr_matrix((np.zeros_like(W.data), W.indices, W.indptr), shape=W.shape)
    F = _factors(k)
    if ykind == "observed":
        Y, Wy = _y("observed")
    else:
        rng = np.random.RandomState(6)
        Y, Wy = _f32(rng.randn(D_, D_)), sp.vstack([W, W]).tocsr()
        F[2] = _f32(k ** -0.25 * rng.randn(D_, k))
    Rx, Ry = L.Relation(T, W0), L.Relation(Y, Wy)
    assert Rx.w.size == W.nnz                               # the pattern is kept: stored entries of weight 0
    Hl, gl = L.systems(Rx, Ry, *F, "V", L2)
    Hf, gf = A.systems(Rx, Ry, *F, "V", L2)
    assert (Hl == Hf).all() and (gl == gf).all()
    ctx = _context(lib, T, W0, Y, Wy, F, logit=(False, False))
    lengths = np.concatenate((Rx.row_lengths(True), Ry.row_lengths(False)))
    assert ctx.als_layout()[2] == sum(-(-int(n) // 32) for n in lengths)      # the pieces of both sides, X's included
    H0, g0 = ctx.als_normal(V_, 0, D_, L2)
    ctx.set_relation_loss(0, "logistic")
    H1, g1 = ctx.als_normal(V_, 0, D_, L2)
    ctx.close()
    H32, g32 = A.systems(Rx, Ry, *F, "V", L2, dtype=np.float32)
    _close("H of the V sweep, X without weight", H0[:, :k, :k], H32, Hf, k)
    _close("g of the V sweep, X without weight", g0[:, :k], g32, gf, k)
    assert (H1 == H0).all() and (g1 == g0).all()


# ------------------------------------------------------------------ step level
@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("k", [3, 40])
def test_one_step(lib, k, nn):
    """cmf_als_step (signed) and cmf_als_nnls_step (all factors non-negative, 4 sweeps): one step V, U, Z from a common start, X
    logistic and Y full; and a second step from the same state gives the same bits."""
    T, W = _pattern()
    Y, _ = _y("full")
    F = _factors(k, seed=1)
    if nn:
        F = [np.abs(M) for M in F]
    kw = dict(nn_mask=7, nn_sweeps=4) if nn else {}
    y64 = L.step(T, Y, W, None, *F, L2, **kw)
    y32 = L.step(T, Y, W, None, *F, L2, dtype=np.float32, **kw)
    ctx = _context(lib, T, W, Y, None, F)
    runs = []
    for _ in range(2):
        for w in range(3):
            ctx.set_factor(w, F[w])
        if nn:
            ctx.als_nnls_step(L2, 7, 7, 4)
        else:
            ctx.als_step(L2, 0, 7)
        runs.append([ctx.get_factor(w) for w in range(3)])
    ctx.close()
    for w in range(3):
        assert (runs[0][w] == runs[1][w]).all(), "factor %s: a repeated step differs" % "UVZ"[w]
        _close("%s after one %s step" % ("UVZ"[w], "non-negative" if nn else "signed"), runs[0][w], y32[w], y64[w], k)
        if nn:
            assert runs[0][w].min() >= 0


# ------------------------------------------------------------------ the loss
@pytest.mark.parametrize("k", [3, 40, 200])
def test_logistic_loss(lib, k):
    """cmf_als_logistic_loss against the float64 sum to 1e-6 relative, the saturated row (|s| ~ 30) included; 0 for the Frobenius
    relation."""
    T, W = _pattern()
    Y, Wy = _y("observed")
    F = _factors(k)
    ctx = _context(lib, T, W, Y, Wy, F)
    lx, ly = ctx.als_logistic_loss()
    want = L.loss(L.Relation(T, W), F[0], F[1])
    print("k=%d: loss %.9g, yardstick %.9g, relative error %.3e" % (k, lx, want, abs(lx - want) / want))
    assert abs(lx - want) <= 1e-6 * want and ly == 0.0
    assert ctx.als_logistic_loss() == (lx, ly)
    assert ctx.als_logistic_loss(False, True) == (0.0, 0.0)
    # Y as the logistic one (targets squeezed into [0, 1]), both sides at once
    Ys = _f32(L.sigmoid(Y))
    _bind_csr(ctx, 1, Ys, Wy)
    ctx.set_relation_loss(1, "logistic")
    lx2, ly2 = ctx.als_logistic_loss()
    wy = L.loss(L.Relation(Ys, Wy), F[1], F[2])
    assert lx2 == lx and abs(ly2 - wy) <= 1e-6 * wy
    ctx.close()


def test_logistic_loss_of_a_long_row(lib):
    """A row of 5000 stored entries is cut into pieces of 2048: the pieces are added in piece order."""
    rng = np.random.RandomState(2)
    m, d, p, k = 3, 6000, 2, 8
    W = sp.csr_matrix((rng.rand(m, d) < np.array([[5000.0 / d], [0.01], [0.3]])) * 1.0)
    T = (rng.rand(m, d) < 0.5) * 1.0
    F = [_f32(0.5 * rng.randn(n, k)) for n in (m, d, p)]
    ctx = _context(lib, T, W, np.zeros((d, p)), None, F, piece=0)
    lx, _ = ctx.als_logistic_loss()
    want = L.loss(L.Relation(T, W), F[0], F[1])
    assert abs(lx - want) <= 1e-6 * want
    ctx.close()


# ------------------------------------------------------------------ descent on the planted problem
@pytest.mark.parametrize("nn", [False, True])
def test_device_descent(lib, nn):
    """8 device iterations on the planted problem (seed 3): the float64 objective of the downloaded factors satisfies the condition
    the yardstick's float32 mode satisfies (test_als_logit_host.py), J' <= J + (k + 16) 2^-24 |J|."""
    pr = L.planted(3)
    Rx, Ry = L.Relation(pr["T"], pr["Wsp"]), L.Relation(pr["Y"], None)
    F = [np.abs(M) if nn else M.copy() for M in pr["start"]]
    ctx = _context(lib, pr["T"], pr["Wsp"], pr["Y"], None, F, piece=0)
    j = L.objective(Rx, Ry, None, None, *[_f32(M) for M in F], pr["l2"])
    trace = [j]
    for _ in range(8):
        if nn:
            ctx.als_nnls_step(pr["l2"], 7, 7, 4)
        else:
            ctx.als_step(pr["l2"], 0, 7)
        jn = L.objective(Rx, Ry, None, None, *[ctx.get_factor(w) for w in range(3)], pr["l2"])
        trace.append(jn)
    ctx.close()
    print("device objective (%s): %s" % ("non-negative" if nn else "signed", " ".join("%.2f" % v for v in trace)))
    for a, b in zip(trace, trace[1:]):
        assert b <= a + (pr["k"] + 16) * 2.0 ** -24 * abs(a)
    assert trace[-1] < 0.8 * trace[0]


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def fitted(lib):
    from pycmf_amd import CMF
    pr = L.planted(3)
    model = CMF(n_components=pr["k"], solver="als", loss="logistic", x_link="logit", l2_reg=pr["l2"], max_iter=15, tol=0, x_init="custom",
                y_init="custom", random_state=0, U_non_negative=False, V_non_negative=False, Z_non_negative=False)
    U, V, Z = (M.copy() for M in pr["start"])
    model.fit(pr["T"], pr["Y"], U=U, V=V, Z=Z, x_entry_weights=pr["Wsp"])
    return pr, model


def test_fit_recovers_what_the_yardstick_recovers(fitted):
    pr, model = fitted
    Rx, Ry = L.Relation(pr["T"], pr["Wsp"]), L.Relation(pr["Y"], None)
    U, V, Z = (M.copy() for M in pr["start"])
    for _ in range(15):
        U, V, Z = L.step(Rx, Ry, None, None, U, V, Z, pr["l2"])
    want, got = L.agreement(U, V, pr), L.agreement(model.x_weights, model.components, pr)
    print("agreement on the unobserved cells: device %.3f, yardstick %.3f" % (got, want))
    assert abs(got - want) <= 0.01 and model.n_iter_ == 15
    # the error metric: the cross-entropy sum of X plus the Frobenius norm of Y's residual
    lx = L.loss(Rx, _f32(model.x_weights), _f32(model.components))
    ey = np.sqrt(A.residual_sq(Ry, _f32(model.components), _f32(model.y_weights)))
    assert model.logistic_loss_[1] == 0.0 and abs(model.logistic_loss_[0] - lx) <= 1e-5 * lx
    assert abs(model.reconstruction_err_ - (lx + ey)) <= 1e-5 * (lx + ey)


def test_predict_applies_the_link(fitted):
    pr, model = fitted
    rng = np.random.RandomState(0)
    rows, cols = rng.randint(0, pr["m"], 500), rng.randint(0, pr["d"], 500)
    got = model.predict(rows, cols)
    want = L.sigmoid(np.einsum("ij,ij->i", _f32(model.x_weights)[rows], _f32(model.components)[cols]))
    assert got.dtype == np.float32 and (got > 0).all() and (got < 1).all()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)


def test_transform_folds_in_new_rows(fitted):
    """New rows of X against the fixed V under the same loss: the 15 U sweeps of the fold-in against 15 sweeps of the yardstick from
    the same start (the 'random' rule under the model's random_state, which a custom init without U falls back to)."""
    from pycmf_amd.factor_init import init_custom
    pr, model = fitted
    k = pr["k"]
    sel = np.arange(0, pr["m"], 4)
    Xn, Wn = pr["T"][sel], sp.csr_matrix(pr["Wsp"][sel])
    V0, Z0 = model.components.copy(), model.y_weights.copy()
    Un, Vn, Zn = model.transform(Xn, None, x_entry_weights=Wn)
    assert Un.shape == (len(sel), k) and np.isfinite(Un).all()
    assert (Vn == V0).all() and (Zn == Z0).all()
    Rn, Ry = L.Relation(Xn, Wn), L.Relation(pr["Y"], None)
    start = _f32(init_custom(None, Xn, k, 0, non_negative=False, random_state=model.random_state))
    Vf, Zf = _f32(V0), _f32(Z0)
    y64, y32 = start.copy(), start.astype(np.float32)
    for _ in range(model.max_iter):
        y64 = L.sweep(Rn, Ry, y64, Vf, Zf, "U", pr["l2"])
        y32 = L.sweep(Rn, Ry, y32, Vf, Zf, "U", pr["l2"], dtype=np.float32)
    _close("U of the fold-in", Un, y32, y64, k)


# ------------------------------------------------------------------ the C ABI's refusals
def test_relation_loss_is_validated_and_cleared(lib):
    ctx = lib.Context(0)
    ctx.set_problem(M_, D_, P_, 4)
    with pytest.raises(ValueError, match="which must be 0"):
        ctx.set_relation_loss(2, 1)
    with pytest.raises(ValueError, match="kind must be"):
        ctx.set_relation_loss(0, 2)
    ctx.set_relation_loss(1, 1)
    assert ctx.get_relation_loss(1) == 1
    ctx.set_problem(M_, D_, P_, 4)
    assert ctx.get_relation_loss(1) == 0
    ctx.close()


def test_unsupported_combinations_are_refused(lib):
    T, W = _pattern()
    Y, _ = _y("full")
    F = _factors(3)
    # a full relation, and dense weights
    ctx = lib.Context(0)
    ctx.set_problem(M_, D_, P_, 3)
    ctx.set_data(0, T)
    ctx.set_data(1, Y)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.set_relation_loss(0, "logistic")
    with pytest.raises(NotImplementedError, match="no CSR weights bound"):
        ctx.als_step(L2, 0, 7)
    with pytest.raises(NotImplementedError, match="no CSR weights bound"):
        ctx.als_normal(U_, 0, M_, L2)
    with pytest.raises(NotImplementedError, match="no CSR weights bound"):
        ctx.als_logistic_loss()
    ctx.als_step(L2, 0, 4)                                   # the Z sweep reads Y only: nothing to refuse
    ctx.set_weight(0, np.asarray(W.toarray() > 0, dtype=np.float64))
    with pytest.raises(NotImplementedError, match="no CSR weights bound"):
        ctx.als_nnls_step(L2, 7, 7, 4)
    ctx.close()
    # the conjugate-gradient rows, the bias step, a background weight, biases
    ctx = _context(lib, T, W, Y, None, F)
    with pytest.raises(NotImplementedError, match="conjugate-gradient"):
        ctx.als_cg_step(L2, 0, 7, 3)
    with pytest.raises(NotImplementedError, match="conjugate-gradient"):
        ctx.als_cg_rows(U_, 0, M_, L2, 3)
    with pytest.raises(NotImplementedError, match="logistic loss"):
        ctx.als_bias_step(L2, 0, 7)
    ctx.set_biases(0, True, 0.5, 0.1)
    with pytest.raises(NotImplementedError, match="biases"):
        ctx.als_step(L2, 0, 7)
    ctx.set_biases(0, False)
    Wb = W.copy()
    Wb.data[:] = np.maximum(Wb.data, 0.5)
    _bind_csr(ctx, 0, T, Wb)
    ctx.set_background_weight(0, 0.25)
    with pytest.raises(NotImplementedError, match="background weight"):
        ctx.als_step(L2, 0, 7)
    ctx.set_background_weight(0, 0.0)
    ctx.als_step(L2, 0, 7)                                   # and with neither, the step runs
    ctx.close()
