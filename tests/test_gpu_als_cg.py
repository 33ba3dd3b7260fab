"""The conjugate-gradient row solve of the ALS solver on the device (cmf_als_cg_rows, cmf_als_cg_step, CMF(als_cg_steps=n)) against
the float64 yardstick of als_yardstick.py on float32-rounded inputs.  All factor data is SIGNED: with positive factors one
eigenvalue dominates and float32 and float64 CG iterates part ways after three steps, which would make a comparison of iterates
vacuous.  Tolerance per comparison (als_yardstick.tolerance, the HALS rule): tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|)
with y32 the float32 run of the same formulas -- and the first term may not exceed 1e-3 max|y64| (``_tol`` asserts it), so the rule
cannot quietly widen.

Measured on an MI355X (worst |err| / tol and worst value of the cap of each group): see DESIGN section 17."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
from test_gpu_als import SHAPES, _case, _context, _f32
from test_gpu_wmu import fit_inputs

pytestmark = pytest.mark.gpu

NAMES = "UVZ"
L2 = 0.1
DOCUMENTED_STEPS = 6
CAP = 1e-3


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _tol(y32, y64, k, what=""):
    """The rule's tolerance; its float32-against-float64 term is capped at 1e-3 max|y64|."""
    spread = 4.0 * float(np.max(np.abs(np.asarray(y32, np.float64) - y64)))
    cap = spread / (CAP * float(np.max(np.abs(y64))))
    assert cap <= 1.0, "%s: 4 max|y32 - y64| is %.3f of the cap 1e-3 max|y64|" % (what, cap)
    return A.tolerance(y32, y64, k), cap


def _entry_bytes(ctx):
    return 4 * ctx.geometry()[3] + 4


# ------------------------------------------------------------------ 1. exact arithmetic
def _exact_problem(k):
    """U sweep from f = 0.  Column c of X gathers the one-hot row e_(c mod k) of V (d = 2 k columns); a row of X that hits
    coordinate j holds both columns j (weight 1/2) and j + k (weight 1/4), so with l2 = 1/4 H is the identity on every hit
    coordinate, g_j = t_j / 2 + t_(j+k) / 4 with integer t in [-8, 8], and one CG step lands on f = g with every intermediate a
    float32 (r.r <= 36 k in multiples of 1/16).  Rows: every coordinate (2 k entries), the even ones, one, none, all but three."""
    rng = np.random.RandomState(k)
    d, p = 2 * k, 3
    hits = [np.arange(k), np.arange(0, k, 2), np.array([k // 2]), np.array([], dtype=int), np.setdiff1d(np.arange(k), [0, k // 3, k - 1])]
    m = len(hits)
    W, X = np.zeros((m, d)), np.zeros((m, d))
    for i, h in enumerate(hits):
        W[i, h], W[i, h + k] = 0.5, 0.25
        X[i, h], X[i, h + k] = rng.randint(-8, 9, size=len(h)), rng.randint(-8, 9, size=len(h))
    V = np.zeros((d, k))
    V[np.arange(d), np.arange(d) % k] = 1.0
    F = [np.zeros((m, k)), V, _f32(rng.randn(p, k))]
    return X, np.zeros((d, p)), sp.csr_matrix(W), F


@pytest.mark.parametrize("k", [7, 40, 128, 256])
def test_exact_inputs_are_solved_exactly(lib, k):
    X, Y, Wx, F = _exact_problem(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, None)
    ctx = _context(lib, X, Y, F, Wx, None)
    for steps in (1, 3):
        ref = A.sweep(Rx, Ry, *F, "U", 0.25, cg_steps=steps)
        assert (ref == 0.5 * X[:, :k] + 0.25 * X[:, k:]).all() and (ref[3] == 0).all() and (ref != 0).any()
        got = ctx.als_cg_rows(0, 0, len(ref), 0.25, steps)
        assert (got[:, :k] == ref).all(), "k %d, %d steps: %d of %d coordinates differ" % (k, steps, int((got[:, :k] != ref).sum()), ref.size)
        assert (got[:, k:] == 0).all()
    assert all((ctx.get_factor(w) == F[w]).all() for w in range(3))               # the hook leaves the factors alone
    ctx.close()


# ------------------------------------------------------------------ 2. row lengths and sides
LENGTHS = [0, 1, 31, 32, 33, 70, 200]
# k = 7: CG ends after (distinct eigenvalues of H_i) steps in exact arithmetic, 5 .. 8 for the rows here; float64 drops onto the
# solution at that step while float32 needs one or two more, so at 5 .. 8 steps the two runs differ by up to 0.15 max|y| although
# both converge (measured on the CPU: 4 max|y32 - y64| = 107 .. 1917 times the cap at 5, 6, 7, 8 steps, 0.70 of it at 4) -- the
# step counts at k = 7 stay below that cliff; test 4 covers the far side of it
STEPS = {7: (1, 2, 3, 4), 40: (1, 2, 3, 8), 128: (1, 2, 3, 8), 256: (1, 2, 3, 8)}
SMALL_LDS_ENTRIES = 100         # "als_cg_lds" = 100 entries: classes of 12, 25, 50 and 100 entries, the row of 200 streams
_rows_cases = {}


def _pattern(lengths, cols, rng):
    W = np.zeros((len(lengths), cols))
    for i, n in enumerate(lengths):
        W[i, rng.permutation(cols)[:n]] = _f32(0.25 + 3.75 * rng.rand(n))
    return W


def _rows_case(k, yform):
    """X 40 x 260: rows 0 .. 6 hold LENGTHS entries, the others k / 4 .. 2 k (at most 120), non-unit weights.  Y 260 x 33: 'observed'
    (its TRANSPOSE has rows of LENGTHS[:6] entries and more; one empty row), 'dense' or 'csr' full.  Signed data and factors."""
    if (k, yform) in _rows_cases:
        return _rows_cases[(k, yform)]
    rng = np.random.RandomState(1000 + k)
    m, d, p = 40, 260, 33
    lens = LENGTHS + list(rng.randint(max(1, k // 4), min(2 * k, 120) + 1, size=m - len(LENGTHS)))
    Wx = sp.csr_matrix(_pattern(lens, d, rng))
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    Wy = None
    if yform == "observed":
        Wy = _pattern(LENGTHS[:6] + list(rng.randint(1, 100, size=p - 6)), d, rng).T.copy()
        Wy[d // 2] = 0
        Wy = sp.csr_matrix(Wy)
    elif yform == "csr":
        Y = Y * (rng.rand(d, p) < 0.3)
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    _rows_cases[(k, yform)] = (X, Y, Wx, Wy, F, {})
    return _rows_cases[(k, yform)]


def _rows_reference(case, which, steps):
    X, Y, Wx, Wy, F, refs = case
    if (which, steps) not in refs:
        Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
        refs[(which, steps)] = tuple(A.sweep(Rx, Ry, *F, which, L2, cg_steps=steps, dtype=dt) for dt in (np.float64, np.float32))
    return refs[(which, steps)]


ROWS_SWEEPS = {"observed": "UZV", "dense": "V", "csr": "V"}     # U: the row image; Z: Y's transposed image; V: two sides | S and N


@pytest.mark.parametrize("yform", ["observed", "dense", "csr"])
@pytest.mark.parametrize("k", [7, 40, 128, 256])
def test_rows_against_the_yardstick(lib, k, yform):
    case = _rows_case(k, yform)
    X, Y, Wx, Wy, F, _ = case
    ctx = _context(lib, X, Y, F, Wx, Wy, native_y=(yform == "csr"))
    ctx.set_option("als_cg_lds", SMALL_LDS_ENTRIES * _entry_bytes(ctx))
    worst = worst_cap = 0.0
    for which in ROWS_SWEEPS[yform]:
        w = NAMES.index(which)
        for steps in STEPS[k]:
            y64, y32 = _rows_reference(case, which, steps)
            tol, cap = _tol(y32, y64, k, "k %d Y %s sweep %s, %d steps" % (k, yform, which, steps))
            got = ctx.als_cg_rows(w, 0, F[w].shape[0], L2, steps)
            err = float(np.abs(got[:, :k] - y64).max())
            worst, worst_cap = max(worst, err / tol), max(worst_cap, cap)
            print("k %d Y %s sweep %s, %d steps: |err| / tol %.3f (tol %.3e), cap %.3f" % (k, yform, which, steps, err / tol, tol, cap))
            assert np.isfinite(got).all() and err <= tol
            assert (got[:, k:] == 0).all()
            assert (got[(y64 == 0).all(axis=1)] == 0).all()                       # rows without information
    if yform == "observed":
        assert (_rows_reference(case, "U", 1)[0][0] == 0).all()                    # the empty row of X
    print("k %d Y %s: worst |err| / tol %.3f, worst cap %.3f" % (k, yform, worst, worst_cap))
    ctx.close()


# ------------------------------------------------------------------ 3. bits
@pytest.mark.parametrize("k", [40, 256])
def test_results_do_not_depend_on_the_batch_the_call_or_the_lds_class(lib, k):
    X, Y, Wx, Wy, F, _ = _rows_case(k, "observed")
    ctx = _context(lib, X, Y, F, Wx, Wy)
    m = F[0].shape[0]
    runs = {}
    for lds in (-1, 0, SMALL_LDS_ENTRIES * _entry_bytes(ctx), 40 * _entry_bytes(ctx)):
        ctx.set_option("als_cg_lds", lds)
        for w in (0, 1):
            runs[(lds, w)] = ctx.als_cg_rows(w, 0, F[w].shape[0], L2, 3)
            assert ctx.als_cg_rows(w, 0, F[w].shape[0], L2, 3).tobytes() == runs[(lds, w)].tobytes()      # a repeated call
            assert runs[(lds, w)].tobytes() == runs[(-1, w)].tobytes(), "als_cg_lds = %d changes the rows of %s" % (lds, NAMES[w])
        full = runs[(lds, 0)]
        for i in (1, 5, 6, m - 1):                                                                       # a row solved alone
            assert ctx.als_cg_rows(0, i, 1, L2, 3).tobytes() == full[i:i + 1].tobytes()
        assert ctx.als_cg_rows(0, 2, 5, L2, 3).tobytes() == full[2:7].tobytes()
    ctx.close()


# ------------------------------------------------------------------ 4. enough steps
def test_twelve_steps_at_k_7_reach_the_exact_solve(lib):
    case = _rows_case(7, "observed")
    X, Y, Wx, Wy, F, _ = case
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    for w, which in enumerate(NAMES):
        H, g = A.systems(Rx, Ry, *F, which, L2)
        ref = np.linalg.solve(H, g[:, :, None])[:, :, 0]
        ref[A.no_information(Rx, Ry, *F, which)] = 0
        got = ctx.als_cg_rows(w, 0, F[w].shape[0], L2, 12)[:, :7]
        rel = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("sweep %s, 12 steps at k = 7: %.2e relative to the float64 exact solve" % (which, rel))
        assert rel <= 1e-4
    ctx.close()


# ------------------------------------------------------------------ 5. full steps
STEP_STEPS = 3
_refs = {}


def _start(shape, yform, nn):
    """test_gpu_als's signed case, with |F| for the factors in nn: a non-negative factor starts as one."""
    X, Y, Wx, Wy, F, _ = _case(shape, yform)
    return X, Y, Wx, Wy, [np.abs(F[w]) if nn & (1 << w) else F[w] for w in range(3)]


def _reference(shape, yform, mask, nn, nn_sweeps):
    key = (shape, yform, mask, nn, nn_sweeps)
    if key not in _refs:
        X, Y, Wx, Wy, F = _start(shape, yform, nn)
        Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
        _refs[key] = tuple(A.step(Rx, Ry, None, None, *F, L2, cg_steps=STEP_STEPS, mask=mask, nn_mask=nn, nn_sweeps=nn_sweeps, dtype=dt) for dt in (np.float64, np.float32)) + (
            [A.no_information(Rx, Ry, *F, w) for w in NAMES],)
    return _refs[key]


def _step_case(lib, shape, yform, mask, nn, nn_sweeps):
    k = shape[3]
    X, Y, Wx, Wy, F = _start(shape, yform, nn)
    y64, y32, empty = _reference(shape, yform, mask, nn, nn_sweeps)
    ctx = _context(lib, X, Y, F, Wx, Wy, native_y=(yform == "csr"))
    ctx.newton_clamp_stats(reset=True)
    before = [ctx.get_factor(w).tobytes() for w in range(3)]
    ctx.als_cg_step(L2, nn, mask, STEP_STEPS, nn_sweeps)
    got = [ctx.get_factor(w) for w in range(3)]
    report = []
    for w in range(3):
        if not mask & (1 << w):
            assert got[w].tobytes() == before[w], "factor %s was not swept and changed" % NAMES[w]
            continue
        tol, cap = _tol(y32[w], y64[w], k, "%s Y %s mask %d nn %d factor %s" % (shape, yform, mask, nn, NAMES[w]))
        err = float(np.abs(got[w] - y64[w]).max())
        report.append("%s %.3f (cap %.3f)" % (NAMES[w], err / tol, cap))
        assert np.isfinite(got[w]).all() and err <= tol, "%s: |err| / tol = %.3f (tol %.3e)" % (NAMES[w], err / tol, tol)
        assert (got[w][empty[w]] == 0).all() and (y64[w][empty[w]] == 0).all(), "%s: rows without information must be exact zeros" % NAMES[w]
        if nn & (1 << w):
            assert (got[w] >= 0).all()
    if mask & 1:
        assert empty[0][shape[0] // 3]                               # the unobserved row of X is such a row of U
    assert ctx.newton_clamp_stats()[0] == 0
    print("%s Y %s mask %d nn %d: |err| / tol %s" % (shape, yform, mask, nn, " ".join(report)))
    ctx.close()


@pytest.mark.parametrize("yform", ["dense", "csr", "observed"])
@pytest.mark.parametrize("shape", SHAPES)
def test_full_step_signed(lib, shape, yform):
    _step_case(lib, shape, yform, 7, 0, 0)


@pytest.mark.parametrize("shape, yform", list(zip(SHAPES, ["observed", "dense", "csr", "observed"])))
def test_full_step_with_a_non_negative_v(lib, shape, yform):
    """nn_mask = 2, nn_sweeps = 4: V goes through the normal equations and coordinate descent, U and Z through CG (Z through the
    shared inverse where Y is full), in one step."""
    _step_case(lib, shape, yform, 7, 2, 4)


@pytest.mark.parametrize("mask", [1, 2, 4])
@pytest.mark.parametrize("shape, yform, nn, nn_sweeps", [((257, 1031, 77, 7), "observed", 0, 0), ((70, 333, 129, 40), "dense", 0, 0),
                                                         ((70, 333, 129, 40), "observed", 2, 4)])
def test_masks(lib, shape, yform, nn, nn_sweeps, mask):
    _step_case(lib, shape, yform, mask, nn, nn_sweeps)


# ------------------------------------------------------------------ 6. nothing else moves
@pytest.mark.parametrize("nn_sweeps", [0, 4])
def test_with_every_factor_non_negative_the_step_is_the_one_without_cg(lib, nn_sweeps):
    shape = (70, 333, 129, 40)
    X, Y, Wx, Wy, F = _start(shape, "observed", 7)
    runs = []
    for cg in (False, True):
        ctx = _context(lib, X, Y, F, Wx, Wy)
        for mask in (7, 2):
            if cg:
                ctx.als_cg_step(L2, 7, mask, 5, nn_sweeps)
            elif nn_sweeps:
                ctx.als_nnls_step(L2, 7, mask, nn_sweeps)
            else:
                ctx.als_step(L2, 7, mask)
        runs.append([ctx.get_factor(w).tobytes() for w in range(3)])
        ctx.close()
    assert runs[0] == runs[1]


def test_other_solvers_are_untouched_by_cg_steps(lib):
    """Context b runs CG steps in between (CSR weights bound: CG for U and V beside the shared route for Z, then a mixed mask),
    its factors reset afterwards; context a never hears of them.  cmf_mu_step, cmf_newton_step (per-row Hessians: a logit link),
    cmf_als_step, cmf_als_nnls_step and cmf_hals_step agree byte for byte, and so do the clamp statistics of the Newton steps."""
    m, d, p, k = 200, 300, 90, 12
    rng = np.random.RandomState(41)
    X, Y = _f32(np.abs(rng.randn(m, d))), _f32(1.0 / (1.0 + np.exp(-rng.randn(d, p))))
    F = [_f32(np.abs(rng.randn(n, k)) * 0.3 + 0.01) for n in (m, d, p)]
    Wx = sp.csr_matrix(_f32(rng.rand(m, d) + 0.5) * (rng.rand(m, d) < 0.2))
    a, b = _context(lib, X, Y, F, None, None), _context(lib, X, Y, F, None, None)
    r = np.repeat(np.arange(m), np.diff(Wx.indptr))

    def reset(ctx):
        for w in range(3):
            ctx.set_factor(w, F[w])

    def factors(ctx):
        return [ctx.get_factor(w).tobytes() for w in range(3)]

    def bind(ctx):
        ctx.set_weighted_csr(0, Wx.indptr, Wx.indices, X[r, Wx.indices], Wx.data)

    def newton(ctx):
        ctx.newton_step(0.4, 0.0, 0.05, "linear", "logit", 0, 7, 0.2, 1.0, None, None, None, None)
    for ctx in (a, b):
        ctx.newton_clamp_stats(reset=True)
    for step in (lambda c: c.mu_step(0.0, 0.0, 7), newton, lambda c: c.mu_step(0.01, 0.02, 7)):
        bind(b)
        b.als_cg_step(0.1, 0, 7, 4, 0)
        b.als_cg_step(0.1, 2, 7, 2, 3)
        b.clear_weight(0)
        reset(a)
        reset(b)
        step(a)
        step(b)
        assert factors(a) == factors(b)
    assert a.newton_clamp_stats(full=True) == b.newton_clamp_stats(full=True)
    assert a.newton_clamp_routes() == b.newton_clamp_routes()
    for step in (lambda c: c.als_step(0.1, 0, 7), lambda c: c.als_step(0.1, 5, 7), lambda c: c.als_nnls_step(0.1, 7, 7, 2)):
        bind(a)
        bind(b)
        b.als_cg_step(0.1, 0, 7, 4, 0)
        reset(a)
        reset(b)
        step(a)
        step(b)
        assert factors(a) == factors(b)
    a.clear_weight(0)
    b.clear_weight(0)
    b.als_cg_step(0.1, 0, 7, 4, 0)                           # no weights bound: every sweep takes the shared route
    reset(a)
    reset(b)
    a.hals_step(0.01, 0.02, 7)
    b.hals_step(0.01, 0.02, 7)
    assert factors(a) == factors(b)
    a.close()
    b.close()


def test_refusals(lib):
    m, d, p, k = 40, 50, 30, 6
    rng = np.random.RandomState(2)
    ctx = lib.Context(0)
    ctx.set_problem(40, 50, 30, 300)
    with pytest.raises(NotImplementedError, match="k_pad"):
        ctx.als_cg_step(0.1, 0, 7, 4, 0)
    ctx.set_problem(m, d, p, k)
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    for w in range(3):
        ctx.set_factor(w, F[w])
    X = _f32(rng.randn(m, d))
    ctx.set_data(0, X)
    ctx.set_data(1, _f32(rng.randn(d, p)))
    with pytest.raises(ValueError, match="no observed relation"):
        ctx.als_cg_rows(0, 0, 1, 0.1, 4)
    Ws = sp.csr_matrix((rng.rand(m, d) < 0.5).astype(float))
    r = np.repeat(np.arange(m), np.diff(Ws.indptr))
    ctx.set_weighted_csr(0, Ws.indptr, Ws.indices, X[r, Ws.indices], Ws.data)
    for steps in (0, -1, 1025):
        with pytest.raises(ValueError, match="cg_steps must be 1 .. 1024"):
            ctx.als_cg_step(0.1, 0, 7, steps, 0)
        with pytest.raises(ValueError, match="cg_steps must be 1 .. 1024"):
            ctx.als_cg_rows(0, 0, 1, 0.1, steps)
    for sweeps in (-1, 1025):
        with pytest.raises(ValueError, match="nn_sweeps must be 0 .. 1024"):
            ctx.als_cg_step(0.1, 0, 7, 4, sweeps)
    with pytest.raises(ValueError, match="l2 must be positive"):
        ctx.als_cg_step(0.0, 0, 7, 4, 0)
    for mask in (0, 8):
        with pytest.raises(ValueError, match="update_mask"):
            ctx.als_cg_step(0.1, 0, mask, 4, 0)
    with pytest.raises(ValueError, match="rows out of range"):
        ctx.als_cg_rows(0, m - 1, 2, 0.1, 4)
    with pytest.raises(ValueError, match="no observed relation"):
        ctx.als_cg_rows(2, 0, 1, 0.1, 4)                     # the Z sweep reads Y alone, which is full
    ctx.als_cg_step(0.1, 0, 7, 1024, 0)                      # the largest count: rows stop when the residual vanishes
    assert all(np.isfinite(ctx.get_factor(w)).all() for w in range(3))
    ctx.close()


# ------------------------------------------------------------------ 7. fit through CMF
def test_fit_reaches_the_objective_of_exact_als(lib):
    """The planted problem of the documentation (120 x 150, 50 % of X observed, k = 12, l2 = 0.05, signed, 20 iterations): the
    float64 objective of the returned factors is within 2 % of exact ALS in float64 (measured on the CPU: 50.05 in float64 and
    49.85 in float32 against 50.46) and below the one of a fit with one CG step per row (144.7)."""
    from pycmf_amd import CMF
    X, Y, Wx, _, U, V, Z = fit_inputs(3, m=120, d=150, p=20, k=12, obs=.5)
    l2, iters = 0.05, 20
    Xi, Wref = sp.csr_matrix(X * Wx), sp.csr_matrix(Wx)
    assert Xi.nnz == Wref.nnz
    kw = dict(n_components=12, solver="als", l2_reg=l2, tol=0, max_iter=iters, x_init="custom", y_init="custom",
              U_non_negative=False, V_non_negative=False, Z_non_negative=False)
    obj = {}
    for steps in (DOCUMENTED_STEPS, 1):
        model = CMF(als_cg_steps=steps, **kw)
        Ug, Vg, Zg = model.fit_transform(Xi, Y, U=U.copy(), V=V.copy(), Z=Z.copy(), x_entry_weights="observed")
        assert model.n_iter_ == iters and all(np.isfinite(G_).all() for G_ in (Ug, Vg, Zg))
        obj[steps] = A.objective(X, Y, Wx, None, Ug, Vg, Zg, l2)
    Ur, Vr, Zr, _, _ = A.fit(X, Y, Wref, None, U, V, Z, iters, l2)
    exact = A.objective(X, Y, Wx, None, Ur, Vr, Zr, l2)
    print("objective after %d iterations: exact ALS (float64) %.2f, %d CG steps %.2f, 1 CG step %.2f" % (iters, exact, DOCUMENTED_STEPS, obj[DOCUMENTED_STEPS], obj[1]))
    assert obj[DOCUMENTED_STEPS] <= 1.02 * exact
    assert obj[DOCUMENTED_STEPS] < obj[1]
    # transform carries the keyword: V and Z fixed, U re-fitted by CG on the observed entries of new rows
    U2, V2, Z2 = model.transform(Xi[:50], None, x_entry_weights="observed")
    assert V2.tobytes() == model.components.tobytes() and Z2.tobytes() == model.y_weights.tobytes()
    assert U2.shape == (50, 12) and np.isfinite(U2).all()
