"""Long rows of the CG route on the device (option "als_cg_piece", als_cg_piece_kernel / als_cg_combine_kernel, cmf_als_cg_last)
against the float64 yardstick of als_yardstick.py, unchanged, on the fixtures of als_cg_pieces_cases.py.  Tolerance per comparison:
als_yardstick.tolerance with the cap assertion of test_gpu_als_cg.py (``_tol``): 4 max|y32 - y64| <= 1e-3 max|y64|.  That the rule
needs no extra term for sums taken in piece order is checked on the CPU by test_als_cg_pieces_host.py.

Measured on an MI355X (worst |err| / tol and worst value of the cap of each group): see DESIGN section 19."""
import numpy as np
import pytest

import als_yardstick as A
import als_cg_pieces_cases as P
from test_gpu_als import _context
from test_gpu_als_cg import _exact_problem, _tol

pytestmark = pytest.mark.gpu

NAMES = "UVZ"
L2 = P.L2


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _ctx(lib, c, yform="observed", piece=64, F=None):
    X, Y, Wx, Wy, F0, _ = c
    ctx = _context(lib, X, Y, F0 if F is None else F, Wx, Wy, native_y=(yform == "csr"))
    ctx.set_option("als_cg_piece", piece)
    return ctx


def _background(ctx, c, bg):
    cx, cy = P.backgrounds(c, bg)
    ctx.set_background_weight(0, cx)
    if c[3] is not None:
        ctx.set_background_weight(1, cy)


# ------------------------------------------------------------------ 1. exact arithmetic
@pytest.mark.parametrize("k", [40, 128, 256])
def test_exact_inputs_are_solved_exactly_through_pieces_of_16(lib, k):
    """Rows of 2 k, k, 1, 0 and 2 k - 6 entries, pieces of 16: every product and partial sum is a float32, so any order gives ==."""
    X, Y, Wx, F = _exact_problem(k)
    Rx, Ry = A.Relation(X, Wx), A.Relation(Y, None)
    ctx = _context(lib, X, Y, F, Wx, None)
    ctx.set_option("als_cg_piece", 16)
    lens = np.array([2 * k, k, 1, 0, 2 * k - 6])
    ref = None
    for steps in (1, 3):
        ref = A.sweep(Rx, Ry, *F, "U", 0.25, cg_steps=steps)
        assert (ref == 0.5 * X[:, :k] + 0.25 * X[:, k:]).all() and (ref != 0).any()
        got = ctx.als_cg_rows(0, 0, len(ref), 0.25, steps)
        assert ctx.als_cg_last() == (int((lens > 16).sum()), int(((lens[lens > 16] + 15) // 16).sum()))
        assert (got[:, :k] == ref).all(), "k %d, %d steps: %d of %d coordinates differ" % (k, steps, int((got[:, :k] != ref).sum()), ref.size)
        assert (got[:, k:] == 0).all()
    ctx.set_factor(0, ref)                                                       # r = 0: every row stops and keeps what it has
    solved = ctx.get_factor(0)
    again = ctx.als_cg_rows(0, 0, len(ref), 0.25, 3)
    assert again[:, :k].tobytes() == np.ascontiguousarray(solved, dtype=np.float32).tobytes() and (again[:, k:] == 0).all()
    ctx.close()


# ------------------------------------------------------------------ 2. parity of cmf_als_cg_rows
@pytest.mark.parametrize("name, yform", sorted(P.SWEEPS))
@pytest.mark.parametrize("k", P.KS)
def test_rows_against_the_yardstick(lib, k, name, yform):
    c = P.case(name, k, yform)
    F = c[4]
    ctx = _ctx(lib, c, yform)
    worst = worst_cap = 0.0
    for bg in P.BACKGROUNDS:
        _background(ctx, c, bg)
        for which in P.SWEEPS[(name, yform)]:
            w = NAMES.index(which)
            for steps in P.STEPS[k]:
                y64, y32 = P.reference(c, which, steps, bg)
                what = "case %s Y %s k %d sweep %s bg %g, %d steps" % (name, yform, k, which, bg, steps)
                tol, cap = _tol(y32, y64, k, what)
                got = ctx.als_cg_rows(w, 0, F[w].shape[0], L2, steps)
                assert ctx.als_cg_last() == P.long_rows_and_pieces(c, which, 64) and ctx.als_cg_last()[0] > 0
                err = float(np.abs(got[:, :k] - y64).max())
                worst, worst_cap = max(worst, err / tol), max(worst_cap, cap)
                print("%s: |err| / tol %.3f (tol %.3e), cap %.3f" % (what, err / tol, tol, cap))
                assert np.isfinite(got).all() and err <= tol
                assert (got[:, k:] == 0).all()
                assert (got[(y64 == 0).all(axis=1)] == 0).all()                   # rows without information
    if name == "A":
        assert (P.reference(c, "U", 1, 0.0)[0][0] == 0).all()                     # the empty row of X
    print("case %s Y %s k %d: worst |err| / tol %.3f, worst cap %.3f" % (name, yform, k, worst, worst_cap))
    ctx.close()


# ------------------------------------------------------------------ 3. the route is taken
@pytest.mark.parametrize("k", [7, 256])
def test_the_long_rows_and_their_pieces_are_the_ones_the_lengths_give(lib, k):
    for name, sweeps in (("A", "UZ"), ("B", "V")):
        c = P.case(name, k)
        ctx = _ctx(lib, c)
        assert ctx.als_cg_last() == (0, 0)
        for which in sweeps:
            w = NAMES.index(which)
            for piece in (64, 128, 100, -1):                                      # 100 is rounded up to 112
                ctx.set_option("als_cg_piece", piece)
                ctx.als_cg_rows(w, 0, c[4][w].shape[0], L2, 2)
                want = (0, 0) if piece < 0 else P.long_rows_and_pieces(c, which, (piece + 15) // 16 * 16)
                assert ctx.als_cg_last() == want, (name, which, piece)
            ctx.set_option("als_cg_piece", 64)
            ctx.als_cg_rows(w, 3, 4, L2, 2)                                        # a sub-range counts its own rows
            n = P.row_lengths(c, which)[3:7]
            assert ctx.als_cg_last() == (int((n > 64).sum()), int(((n[n > 64] + 63) // 64).sum()))
        ctx.close()


# ------------------------------------------------------------------ 4. bits
@pytest.mark.parametrize("k", [40, 256])
def test_a_long_row_depends_on_the_row_and_the_piece_length_alone(lib, k):
    for name, which in (("A", "U"), ("B", "V")):
        c = P.case(name, k)
        w = NAMES.index(which)
        n = c[4][w].shape[0]
        lens = P.row_lengths(c, which)
        ctx = _ctx(lib, c)
        entry = 4 * ctx.geometry()[3] + 4
        full = ctx.als_cg_rows(w, 0, n, L2, 3)
        assert ctx.als_cg_rows(w, 0, n, L2, 3).tobytes() == full.tobytes()                          # a repeated call
        for i in np.flatnonzero(lens > 64)[[0, 1, -1]]:                                              # a long row solved alone
            assert ctx.als_cg_rows(w, int(i), 1, L2, 3).tobytes() == full[i:i + 1].tobytes()
        assert ctx.als_cg_rows(w, 2, 7, L2, 3).tobytes() == full[2:9].tobytes()                     # inside a sub-range
        for lds in (0, 40 * entry, -1):
            ctx.set_option("als_cg_lds", lds)
            assert ctx.als_cg_rows(w, 0, n, L2, 3).tobytes() == full.tobytes(), "als_cg_lds = %d" % lds
        ctx.set_option("als_cg_piece", -1)
        uncut = ctx.als_cg_rows(w, 0, n, L2, 3)
        short = lens <= 64
        assert short.any() and uncut[short].tobytes() == full[short].tobytes()                      # short rows: the parent's route
        ctx.set_option("als_cg_piece", 128)
        other = ctx.als_cg_rows(w, 0, n, L2, 3)
        assert uncut[lens <= 128].tobytes() == other[lens <= 128].tobytes()
        y64, y32 = P.reference(c, which, 3, 0.0)
        tol, _ = _tol(y32, y64, k, "case %s k %d sweep %s" % (name, k, which))
        for L, got in ((64, full), (128, other)):
            err = float(np.abs(got[:, :k] - y64).max())
            print("case %s k %d sweep %s L %d: |err| / tol %.3f" % (name, k, which, L, err / tol))
            assert err <= tol
        ctx.close()


# ------------------------------------------------------------------ 5. full steps
STEP_STEPS = 3
_step_refs = {}


def _step_start(k, nn):
    X, Y, Wx, Wy, F, _ = P.case("B", k)
    return [np.abs(F[w]) if nn & (1 << w) else F[w] for w in range(3)]


def _step_reference(k, mask, nn, nn_sweeps, bg):
    key = (k, mask, nn, nn_sweeps, bg)
    if key not in _step_refs:
        c = P.case("B", k)
        Rx, Ry = P.relations(c)
        F = _step_start(k, nn)
        _step_refs[key] = tuple(A.step(Rx, Ry, None, None, *F, L2, cg_steps=STEP_STEPS, mask=mask, nn_mask=nn, nn_sweeps=nn_sweeps, cx=bg,
                                       dtype=dt) for dt in (np.float64, np.float32))
    return _step_refs[key]


# The cases are the ones whose float32 and float64 yardstick runs agree within the cap (a property of the fixture alone, computed on
# the CPU): the rows of U and Z of case B hold at most 12 entries, and at k >= 128 (k = 40 once V is non-negative) three CG steps on
# those rows in float32 and in float64 part ways -- 4 max|y32 - y64| is 1.1 .. 460 times the cap there.  Those rows are short and
# take the single-launch route; at k = 128 and 256 the step is therefore run on V alone (mask 2: the long rows) and under the
# background weight, where the cap holds for all three factors.
STEP_CASES = [(7, 7, 0, 0, 0.0), (7, 1, 0, 0, 0.0), (7, 7, 2, 4, 0.0), (7, 7, 0, 0, 0.25),
              (40, 7, 0, 0, 0.0), (40, 1, 0, 0, 0.0), (40, 7, 0, 0, 0.25),
              (128, 2, 0, 0, 0.0), (128, 7, 0, 0, 0.25), (256, 2, 0, 0, 0.0), (256, 7, 0, 0, 0.25)]


@pytest.mark.parametrize("k, mask, nn, nn_sweeps, bg", STEP_CASES)
def test_full_step(lib, k, mask, nn, nn_sweeps, bg):
    """cmf_als_cg_step on case B, 3 steps, pieces of 64; bg: cmf_set_background_weight(x, 0.25)."""
    c = P.case("B", k)
    F = _step_start(k, nn)
    y64, y32 = _step_reference(k, mask, nn, nn_sweeps, bg)
    ctx = _ctx(lib, c, F=F)
    if bg:
        ctx.set_background_weight(0, bg)
    ctx.newton_clamp_stats(reset=True)
    before = [ctx.get_factor(w).tobytes() for w in range(3)]
    ctx.als_cg_step(L2, nn, mask, STEP_STEPS, nn_sweeps)
    got = [ctx.get_factor(w) for w in range(3)]
    report = []
    for w in range(3):
        if not mask & (1 << w):
            assert got[w].tobytes() == before[w], "factor %s was not swept and changed" % NAMES[w]
            continue
        tol, cap = _tol(y32[w], y64[w], k, "k %d mask %d nn %d bg %g factor %s" % (k, mask, nn, bg, NAMES[w]))
        err = float(np.abs(got[w] - y64[w]).max())
        report.append("%s %.3f (cap %.3f)" % (NAMES[w], err / tol, cap))
        assert np.isfinite(got[w]).all() and err <= tol, "%s: |err| / tol = %.3f (tol %.3e)" % (NAMES[w], err / tol, tol)
        if nn & (1 << w):
            assert (got[w] >= 0).all()
    assert ctx.newton_clamp_stats()[0] == 0
    print("k %d mask %d nn %d bg %g: |err| / tol %s" % (k, mask, nn, bg, " ".join(report)))
    ctx.close()


# ------------------------------------------------------------------ 6. descent
def test_five_steps_never_raise_the_objective(lib):
    """Case B at k = 40, 6 CG steps per row, pieces of 64: the float64 objective of the returned factors never rises by more than
    1e-6 relative -- the float32 rounding of a monotone method."""
    c = P.case("B", 40)
    X, Y, Wx, Wy, F, _ = c
    Rx, Ry = P.relations(c)
    ctx = _ctx(lib, c)
    seq = [A.objective(Rx, Ry, None, None, *F, L2)]
    for _ in range(5):
        ctx.als_cg_step(L2, 0, 7, 6, 0)
        seq.append(A.objective(Rx, Ry, None, None, *[ctx.get_factor(w) for w in range(3)], L2))
    print("objective: " + " ".join("%.6e" % v for v in seq))
    assert all(b <= a * (1 + 1e-6) for a, b in zip(seq, seq[1:])) and seq[-1] < seq[0]
    ctx.close()
