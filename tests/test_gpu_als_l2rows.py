"""Per-row l2 multipliers of the ALS solver on the device (cmf_set_l2_rows / cmf_get_l2_rows, CMF(als_l2_scale=nu)).

1 / 2.  The device forms lambda_i = (float)l2 * mult[row] as one float32 multiplication, so with l2 = 0.5 and multipliers drawn from
{0.5, 1, 2, 4} (exact products) a row under the multiplier v must have THE BITS the same call gives it with nothing bound and the
scalar l2 v -- on every route; all-ones multipliers, cleared multipliers and a problem bound anew must give the bits of the unbound
call, and a repeated call its own.  The scalar path is what the rest of the suite holds against float64, so these comparisons need
no tolerance.  3.  Multipliers max(n_i, 1)^0.5 (no powers of two), l2 = 0.05: the exact, coordinate-descent, conjugate-gradient and
dual rows and cmf_als_normal against the float64 yardstick (als_l2rows_yardstick.py) within als_yardstick.tolerance(y32, y64, k),
y32 the yardstick's float32 mode.  4.  The shared routes.  5.  The refusals of the C ABI.  6.  The estimator."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_bias_cases as BC
import als_cg_pieces_cases as P
import als_dual_cases as C
import als_l2rows_yardstick as LR
import als_yardstick as A
import nncg_cases as NC
from test_gpu_als import _context, _f32

pytestmark = pytest.mark.gpu

NAMES = "UVZ"
VALUES = (0.5, 1.0, 2.0, 4.0)
L2_BITS = 0.5          # times VALUES: exact in float32
L2_TOL = 0.05
_refs = {}


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _ragged(n, seed):
    """n multipliers from VALUES, each value present (n >= 4), in a fixed random order."""
    return np.random.RandomState(seed).permutation(np.resize(VALUES, n)).astype(np.float64)


def _bits(ctx, w):
    return ctx.get_factor(w).astype(np.float32)


class Route:
    """One way to sweep ONE factor of a bound context from a fixed state: ``step(ctx, l2, bit)``; ``reset(ctx)`` puts the state back."""

    def __init__(self, ctx, F, sweeps, step, reset=None, after=None):
        self.ctx, self.F, self.sweeps, self.step, self.after = ctx, F, sweeps, step, after
        self._reset = reset

    def reset(self):
        for w in range(3):
            self.ctx.set_factor(w, self.F[w])
        if self._reset:
            self._reset(self.ctx)

    def run(self, w, l2):
        self.reset()
        self.step(self.ctx, l2, 1 << w)
        if self.after:
            self.after(self.ctx, w)
        return _bits(self.ctx, w)


def _dual_problem(k, nn=False):
    X, Y, Wx, Wy, F = C.problem(k)
    return X, Y, Wx, Wy, ([np.abs(f) for f in F] if nn else F)


def _positive(W, floor=0.75):
    W = W.copy()
    W.data = np.where(W.data == 0, floor, W.data)      # (a background needs w >= c0 on every stored entry)
    return W


def _bias_reset(name, k):
    def reset(ctx):
        for which, bias in enumerate(BC.biases(name, k)):
            ctx.set_biases(which, True, bias[0], BC.LB)
            ctx.set_bias(which, 0, bias[1])
            ctx.set_bias(which, 1, bias[2])
    return reset


def _expect_dual(ctx, w):
    last = ctx.als_dual_last()
    assert sum(last[:3]) > 0, last
    if w == 0:                                          # the U sweep walks LENGTHS: dual rows, formed rows (129 and 160 entries, or a
        assert last[3] > 0 and last[4] > 0, last        # class no narrower than k_pad) and empty rows in the one sweep


def _expect_pieces(last):
    def after(ctx, w):
        assert getattr(ctx, last)()[0] > 0              # rows were cut into pieces
    return after


def _routes(lib, name, k):
    """The Route objects of one named route at k components (a list: some routes need two problems to reach all three sweeps)."""
    if name in ("exact", "nn_sweeps", "cg resident", "cg streaming", "dual", "logistic", "background"):
        X, Y, Wx, Wy, F = _dual_problem(k, nn=name == "nn_sweeps")
        if name == "logistic":
            X = (X > 0).astype(float)
        if name == "background":
            Wx = _positive(Wx)
        ctx = _context(lib, X, Y, F, Wx, Wy)
        if name == "exact":
            return [Route(ctx, F, "UVZ", lambda c, l2, bit: c.als_step(l2, 0, bit))]
        if name == "nn_sweeps":
            return [Route(ctx, F, "UVZ", lambda c, l2, bit: c.als_nnls_step(l2, 7, bit, 4))]
        if name == "cg resident":
            return [Route(ctx, F, "UVZ", lambda c, l2, bit: c.als_cg_step(l2, 0, bit, 3))]
        if name == "cg streaming":
            ctx.set_option("als_cg_lds", 0)             # no row stays resident
            return [Route(ctx, F, "UVZ", lambda c, l2, bit: c.als_cg_step(l2, 0, bit, 3))]
        if name == "dual":
            return [Route(ctx, F, "UVZ", lambda c, l2, bit: c.als_dual_step(l2, 0, bit, 128), after=_expect_dual)]
        if name == "logistic":
            ctx.set_relation_loss(0, "logistic")
            return [Route(ctx, F, "UV", lambda c, l2, bit: c.als_step(l2, 0, bit))]
        ctx.set_background_weight(0, 0.25)
        return [Route(ctx, F, "UV", lambda c, l2, bit: c.als_step(l2, 0, bit))]
    if name == "cg pieces":                             # the piece length and the patterns of als_cg_pieces_cases: A cuts U and Z rows, B V rows
        out = []
        for case, sweeps in (("A", "UZ"), ("B", "V")):
            X, Y, Wx, Wy, F, _ = P.case(case, k)
            ctx = _context(lib, X, Y, F, Wx, Wy)
            ctx.set_option("als_cg_piece", 64)
            out.append(Route(ctx, F, sweeps, lambda c, l2, bit: c.als_cg_step(l2, 0, bit, 3), after=_expect_pieces("als_cg_last")))
        return out
    if name in ("nn_cg short", "nn_cg cut"):
        X, Y, Wx, Wy, F, _ = NC.case(k, "observed")
        ctx = _context(lib, X, Y, F, Wx, Wy)
        if name == "nn_cg cut":
            ctx.set_option("als_cg_piece", 32)
        return [Route(ctx, F, "UVZ", lambda c, l2, bit: c.als_nncg_step(l2, 7, bit, 0, 3),
                      after=_expect_pieces("als_nncg_last") if name == "nn_cg cut" else None)]
    assert name == "bias"
    X, Y, Wx, Wy, F, _ = P.case("B", k)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    ctx.set_option("als_bias_piece", BC.PIECE)
    return [Route(ctx, F, "UVZ", lambda c, l2, bit: c.als_bias_step(l2, 0, bit, 0, 0), reset=_bias_reset("B", k))]


ROUTE_KS = [(name, k) for name in ("exact", "nn_sweeps", "cg resident", "cg streaming", "logistic", "background") for k in (3, 40, 100, 200)]
ROUTE_KS += [("dual", k) for k in (40, 100, 200)]       # (k_pad = 32 has no dual class)
ROUTE_KS += [("cg pieces", k) for k in P.KS] + [("bias", k) for k in P.KS]
ROUTE_KS += [(name, k) for name in ("nn_cg short", "nn_cg cut") for k in NC.KS]


# ------------------------------------------------------------------ 1 + 2. bits, route by route
@pytest.mark.parametrize("name, k", ROUTE_KS)
def test_rows_under_multipliers_have_the_bits_of_the_scalar_and_unbound_means_untouched(lib, name, k):
    for route in _routes(lib, name, k):
        ctx = route.ctx
        for which in route.sweeps:
            w = NAMES.index(which)
            n = route.F[w].shape[0]
            m = _ragged(n, 100 * k + w)
            assert all(ctx.get_l2_rows(f) is None for f in range(3))
            unbound = route.run(w, L2_BITS)
            assert np.isfinite(unbound).all()
            ctx.set_l2_rows(w, m)
            bound = route.run(w, L2_BITS)
            assert route.run(w, L2_BITS).tobytes() == bound.tobytes(), (name, which, "a repeated call")
            differ = 0
            for v in VALUES:                                                      # 1. the same rows under the scalar l2 v, nothing bound
                ctx.set_l2_rows(w, None)
                scalar = route.run(w, L2_BITS * v)
                ctx.set_l2_rows(w, m)
                assert (m == v).sum() > 0
                assert bound[m == v].tobytes() == scalar[m == v].tobytes(), (name, which, v)
                differ += int((scalar[m != v] != bound[m != v]).any())
            assert differ > 0, (name, which)                                      # (the multipliers do act)
            ctx.set_l2_rows(w, np.ones(n))                                        # 2. all ones: the unbound bits
            assert route.run(w, L2_BITS).tobytes() == unbound.tobytes(), (name, which, "all ones")
            ctx.set_l2_rows(w, m)
            other = (w + 1) % 3                                                   # multipliers of another factor are not read
            ctx.set_l2_rows(w, None)
            ctx.set_l2_rows(other, _ragged(route.F[other].shape[0], 7))
            assert ctx.get_l2_rows(w) is None
            assert route.run(w, L2_BITS).tobytes() == unbound.tobytes(), (name, which, "cleared")
            ctx.set_l2_rows(other, None)
        ctx.close()


def test_set_problem_clears_the_multipliers(lib):
    k = 40
    X, Y, Wx, Wy, F = C.problem(k)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    ctx.als_step(L2_BITS, 0, A.U_BIT)
    unbound = _bits(ctx, 0)
    for w in range(3):
        ctx.set_l2_rows(w, _ragged(F[w].shape[0], w))
    ctx.set_factor(0, F[0])
    ctx.als_step(L2_BITS, 0, A.U_BIT)
    assert _bits(ctx, 0).tobytes() != unbound.tobytes()
    ctx.set_problem(C.M, C.D, C.P, k)
    assert all(ctx.get_l2_rows(w) is None for w in range(3))
    from test_gpu_als import _bind
    _bind(ctx, 0, X, Wx)
    _bind(ctx, 1, Y, Wy)
    for w in range(3):
        ctx.set_factor(w, F[w])
    ctx.als_step(L2_BITS, 0, A.U_BIT)
    assert _bits(ctx, 0).tobytes() == unbound.tobytes()
    ctx.close()


def test_the_row_entries_and_the_normal_equations_honour_the_multipliers(lib):
    """cmf_als_cg_rows / cmf_als_nncg_rows / cmf_als_dual_rows / cmf_als_normal (the test and fold-in paths), a range inside the
    factor: the bits of the scalar call, row by row."""
    k = 40
    X, Y, Wx, Wy, F = C.problem(k)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    calls = {"cg": lambda w, r0, n, l2: ctx.als_cg_rows(w, r0, n, l2, 3), "nncg": lambda w, r0, n, l2: ctx.als_nncg_rows(w, r0, n, l2, 3),
             "dual": lambda w, r0, n, l2: ctx.als_dual_rows(w, r0, n, l2, 128),
             "H": lambda w, r0, n, l2: ctx.als_normal(w, r0, n, l2)[0], "g": lambda w, r0, n, l2: ctx.als_normal(w, r0, n, l2)[1]}
    for w in range(3):
        n = F[w].shape[0]
        r0, nr = 3, n - 7
        m = _ragged(n, 31 + w)
        for what, call in calls.items():
            ctx.set_l2_rows(w, m)
            bound = call(w, r0, nr, L2_BITS)
            ctx.set_l2_rows(w, None)
            for v in VALUES:
                sel = m[r0:r0 + nr] == v
                assert bound[sel].tobytes() == call(w, r0, nr, L2_BITS * v)[sel].tobytes(), (what, NAMES[w], v)
    ctx.close()


# ------------------------------------------------------------------ 3. multipliers that are no powers of two, against float64
def _pattern_mults(Wx, Wy, shape_x, shape_y):
    import pycmf_amd
    return pycmf_amd.l2_multipliers(shape_x, shape_y, Wx, Wy, nu=0.5)


def _reference(k, which, how):
    """(y64, y32) of one sweep of the dual-case problem under max(n, 1)^0.5, computed once."""
    key = (k, which, how)
    if key not in _refs:
        X, Y, Wx, Wy, F = _dual_problem(k, nn=how == "nn_sweeps")
        Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
        m = _pattern_mults(Wx, Wy, X.shape, Y.shape)[NAMES.index(which)]
        kw = {"nn_sweeps": dict(non_negative=True, nn_sweeps=4), "cg 1 step": dict(cg_steps=1), "cg 3 steps": dict(cg_steps=3)}.get(how, {})
        _refs[key] = tuple(LR.sweep(Rx, Ry, *F, which, L2_TOL, m, dtype=dt, **kw) for dt in (np.float64, np.float32))
    return _refs[key]


def _row_lengths(k, which):
    X, Y, Wx, Wy, F = C.problem(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    return sum(rel.row_lengths(trans) for rel, trans, _, _ in A._sides(Rx, Ry, None, None, None, which))


@pytest.mark.parametrize("k", [7, 40, 100, 200])
def test_ragged_multipliers_against_the_float64_yardstick(lib, k):
    """The conjugate-gradient rows: a row of n entries has at most n + 1 distinct eigenvalues (l2, and n from its entries), and CG
    lands on the solution at that step -- float64 drops onto it there while float32 needs a step or two more, so at and beyond that
    step the two yardstick runs are no roundings of one computation (test_gpu_als_cg.py, which keeps its step counts below that
    cliff).  The rows here hold 0, 1, 2, 5, ... entries: ONE step is below the cliff for every row and compares all of them; THREE
    steps compare the rows of at least 3 entries (and the empty ones).  The rows of 1 and 2 entries under 3 steps are held to the
    scalar path's bits by the first test of this file."""
    worst = 0.0
    for how in ("exact", "nn_sweeps", "cg 1 step", "cg 3 steps", "dual_max"):
        if how == "dual_max" and k <= 32:
            continue
        X, Y, Wx, Wy, F = _dual_problem(k, nn=how == "nn_sweeps")
        mults = _pattern_mults(Wx, Wy, X.shape, Y.shape)
        assert all(len(np.unique(m)) > 3 and not np.isin(np.log2(m[m > 1.5]) % 1, [0.0]).all() for m in mults)   # ragged, no powers of two
        ctx = _context(lib, X, Y, F, Wx, Wy)
        for w in range(3):
            ctx.set_l2_rows(w, mults[w])
            got = ctx.get_l2_rows(w)
            assert got.tobytes() == mults[w].tobytes()                           # the doubles round-trip
        step = {"exact": lambda bit: ctx.als_step(L2_TOL, 0, bit), "nn_sweeps": lambda bit: ctx.als_nnls_step(L2_TOL, 7, bit, 4),
                "cg 1 step": lambda bit: ctx.als_cg_step(L2_TOL, 0, bit, 1), "cg 3 steps": lambda bit: ctx.als_cg_step(L2_TOL, 0, bit, 3), "dual_max": lambda bit: ctx.als_dual_step(L2_TOL, 0, bit, 128)}[how]
        for which in NAMES:
            w = NAMES.index(which)
            y64, y32 = _reference(k, which, "exact" if how == "dual_max" else how)
            rows = np.ones(len(y64), dtype=bool)
            if how == "cg 3 steps":
                n = _row_lengths(k, which)
                rows = (n == 0) | (n >= 3)
                assert rows.sum() >= 0.8 * len(rows)                                  # (U: 8 of 48 rows hold 1 or 2 entries)
            tol = A.tolerance(y32[rows], y64[rows], k)
            for f in range(3):
                ctx.set_factor(f, F[f])
            step(1 << w)
            got = ctx.get_factor(w)
            err = float(np.abs(got - y64)[rows].max())
            worst = max(worst, err / tol)
            print("k %d %s sweep %s: |err| / tol %.3f (tol %.3e)" % (k, how, which, err / tol, tol))
            assert np.isfinite(got).all() and err <= tol, (how, which, err, tol)
        ctx.close()
    print("k %d: worst |err| / tol %.3f" % (k, worst))


@pytest.mark.parametrize("k", [7, 40, 100, 200])
def test_normal_equations_under_ragged_multipliers(lib, k):
    """cmf_als_normal's H and g: the systems of the yardstick with lambda_i on the diagonal, by the same rule."""
    X, Y, Wx, Wy, F = C.problem(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, Wy)
    mults = _pattern_mults(Wx, Wy, X.shape, Y.shape)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    for which in NAMES:
        w = NAMES.index(which)
        ctx.set_l2_rows(w, mults[w])
        H, g = ctx.als_normal(w, 0, F[w].shape[0], L2_TOL)
        ref = {}
        for dt in (np.float64, np.float32):
            Hr, gr = A.systems(Rx, Ry, *F, which, 0.0, dtype=dt)
            lam = (np.float32(L2_TOL) * mults[w].astype(np.float32)) if dt is np.float32 else L2_TOL * mults[w]
            Hr[:, np.arange(k), np.arange(k)] += lam[:, None].astype(dt)
            ref[dt] = (Hr, gr)
        for got, what, i in ((H[:, :k, :k], "H", 0), (g[:, :k], "g", 1)):
            tol = A.tolerance(ref[np.float32][i], ref[np.float64][i], k)
            err = float(np.abs(got - ref[np.float64][i]).max())
            print("k %d sweep %s %s: |err| / tol %.3f" % (k, which, what, err / tol))
            assert err <= tol, (which, what, err, tol)
    ctx.close()


# ------------------------------------------------------------------ 4. the shared routes
@pytest.mark.parametrize("k", [3, 40, 100, 200])
def test_shared_routes_take_equal_multipliers_and_refuse_others(lib, k):
    """Y full: the Z sweep reads no observed relation -- shared exact (signed) and shared HALS (non-negative, nn_sweeps = 4)."""
    X, Y, Wx, _, F, _ = NC.case(k, "full")
    ctx = _context(lib, X, Y, F, Wx, None)
    n = F[2].shape[0]
    steps = {"shared exact": lambda l2: ctx.als_step(l2, 0, A.Z_BIT), "shared hals": lambda l2: ctx.als_nnls_step(l2, 4, A.Z_BIT, 4)}
    for what, step in steps.items():
        def run(l2):
            for f in range(3):
                ctx.set_factor(f, F[f])
            step(l2)
            return _bits(ctx, 2).tobytes()
        unbound = run(L2_BITS)
        for v in (0.5, 2.0):
            ctx.set_l2_rows(2, np.full(n, v))
            bound = run(L2_BITS)
            ctx.set_l2_rows(2, None)
            assert bound == run(L2_BITS * v) and bound != unbound, (what, v)
        ctx.set_l2_rows(2, _ragged(n, 5))
        for f in range(3):
            ctx.set_factor(f, F[f])
        with pytest.raises(NotImplementedError, match="Z has per-row l2 multipliers that differ"):
            step(L2_BITS)
        assert (ctx.get_factor(2) == F[2]).all()                                  # nothing of the sweep has run
        ctx.set_l2_rows(2, None)
        assert run(L2_BITS) == unbound, what                                      # the context stays usable
    ctx.close()


# ------------------------------------------------------------------ 5. the refusals of the C ABI
def test_refusals_leave_the_state_unchanged(lib):
    k = 40
    X, Y, Wx, Wy, F = C.problem(k)
    ctx = _context(lib, X, Y, F, Wx, Wy)
    m = _ragged(C.M, 1)
    ctx.set_l2_rows(0, m)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60):                   # (1e-60: zero as float32)
        v = m.copy()
        v[5] = bad
        with pytest.raises(ValueError, match="finite and positive"):
            ctx.set_l2_rows(0, v)
        assert ctx.get_l2_rows(0).tobytes() == m.tobytes()
        with pytest.raises(ValueError, match="finite and positive"):
            ctx.set_l2_rows(1, np.full(C.D, bad))
        assert ctx.get_l2_rows(1) is None
    with pytest.raises(ValueError, match="bad factor selector"):
        ctx.set_l2_rows(3, m)
    with pytest.raises(ValueError, match="bad factor selector"):
        ctx.get_l2_rows(3)
    with pytest.raises(ValueError, match="bad factor selector"):
        ctx.set_l2_rows(-1, None)
    with pytest.raises(ValueError, match="expected 48 multipliers"):
        ctx.set_l2_rows(0, m[:-1])
    assert ctx.get_l2_rows(0).tobytes() == m.tobytes() and ctx.get_l2_rows(2) is None
    ctx.als_step(L2_BITS, 0, A.U_BIT)                                             # the bound multipliers still act
    bound = _bits(ctx, 0)
    ctx.set_l2_rows(0, None)
    assert ctx.get_l2_rows(0) is None
    ctx.set_factor(0, F[0])
    ctx.als_step(L2_BITS, 0, A.U_BIT)
    assert bound.tobytes() != _bits(ctx, 0).tobytes()
    ctx.close()
    fresh = lib.Context(0)
    with pytest.raises(ValueError, match="cmf_set_problem has not been called"):
        fresh.set_l2_rows(0, None)
    fresh.close()


# ------------------------------------------------------------------ 6. through the estimator
def test_the_estimator_runs_the_hand_driven_steps_to_the_bit(lib):
    import pycmf_amd
    from pycmf_amd import CMF
    rng = np.random.RandomState(4)
    m, d, p, k, l2, iters = 40, 60, 8, 5, 0.05, 3
    X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
    Wd = (rng.rand(m, d) < np.linspace(0.05, 0.7, m)[:, None]) * _f32(0.5 + rng.rand(m, d))
    Wd[3] = 0                                                                     # an empty row
    Wx = sp.csr_matrix(Wd)
    F = [_f32(0.3 * rng.randn(n, k)) for n in (m, d, p)]
    mults = pycmf_amd.l2_multipliers(X.shape, Y.shape, Wx, None, nu=0.5)
    assert len(np.unique(mults[0])) > 5 and len(np.unique(mults[2])) == 1        # (Y full: Z takes the shared route with equal multipliers)
    ctx = _context(lib, X, Y, F, Wx, None)
    for w in range(3):
        ctx.set_l2_rows(w, mults[w])
    for _ in range(iters):
        ctx.als_step(l2, 0, 7)
    hand = [ctx.get_factor(w) for w in range(3)]
    for w in range(3):
        ctx.set_l2_rows(w, None)
        ctx.set_factor(w, F[w])
    for _ in range(iters):
        ctx.als_step(l2, 0, 7)
    plain = [ctx.get_factor(w) for w in range(3)]
    ctx.close()
    kw = dict(n_components=k, solver="als", l2_reg=l2, max_iter=iters, tol=0, x_init="custom", y_init="custom", U_non_negative=False,
              V_non_negative=False, Z_non_negative=False)
    model = CMF(als_l2_scale=0.5, **kw)
    got = model.fit_transform(X, Y, U=F[0].copy(), V=F[1].copy(), Z=F[2].copy(), x_entry_weights=Wx)
    for w in range(3):
        assert got[w].tobytes() == hand[w].tobytes(), NAMES[w]
        assert got[w].tobytes() != plain[w].tobytes(), NAMES[w]
        assert model.l2_multipliers_[w].tobytes() == mults[w].tobytes()
    off = CMF(**kw)
    off.fit(X, Y, U=F[0].copy(), V=F[1].copy(), Z=F[2].copy(), x_entry_weights=Wx)
    assert off.l2_multipliers_ is None
    assert all(a.tobytes() == b.tobytes() for a, b in zip((off.x_weights, off.components, off.y_weights), plain))
    # transform: 5 new rows of 0, 2, 9, 20 and 45 entries are folded in under the multipliers of THEIR lengths
    Wn = np.zeros((5, d))
    for i, n in enumerate((0, 2, 9, 20, 45)):
        Wn[i, rng.permutation(d)[:n]] = 1.0
    Xn = _f32(rng.randn(5, d))
    Wns = sp.csr_matrix(Wn)
    U2, V2, Z2 = model.transform(Xn, None, x_entry_weights=Wns)
    assert V2.tobytes() == model.components.tobytes()
    mn = pycmf_amd.l2_multipliers(Xn.shape, None, Wns, None, nu=0.5)
    assert (mn[0] == np.array([1.0, 2.0, 9.0, 20.0, 45.0]) ** 0.5).all() and mn[2] is None
    ctx = _context(lib, Xn, np.zeros((d, p)), [np.zeros((5, k)), model.components, model.y_weights], Wns, None)
    ctx.set_l2_rows(0, mn[0])
    ctx.als_step(l2, 0, A.U_BIT)
    assert U2.tobytes() == ctx.get_factor(0).tobytes()
    ctx.set_l2_rows(0, None)
    ctx.als_step(l2, 0, A.U_BIT)
    assert U2.tobytes() != ctx.get_factor(0).tobytes() and (U2[0] == 0).all()
    ctx.close()
