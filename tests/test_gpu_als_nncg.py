"""Matrix-free non-negative rows of the ALS solver on the device (cmf_als_nncg_step / cmf_als_nncg_rows / cmf_als_nncg_last,
als_nncg_kernel and the piece form) against the float64 yardstick of nncg_yardstick.py on the fixtures of nncg_cases.py: a 40 x 80 X
with rows of 70, 1, 3, 17 and 0 entries, an 80 x 20 Y full or observed, k = 3, 40, 100 and 200 (k_pad 32, 64, 128, 256).

Two assertions per comparison, both with als_yardstick.tolerance and no other constant (nncg_cases.py derives them): the rows whose
float32 and float64 yardstick traces agree and whose decision margin is at least 1e-3 within tolerance(y32, y64, k) -- the
issue's rule, which by the count of coordinates alone leaves most rows out at k >= 100 --, and EVERY row in which float32 decides
as float64 does under four orders of summation, margin at least 4 (k + 16) 2^-24, within the envelope of the float32 yardstick
over those orders.  At most a tenth of a comparison may be outside the second set; the long rows of the piece tests are inside it.
Every row at all must be >= 0 and no higher on its float64 quadratic 1/2 f^T H f - g^T f (als_yardstick.systems) than the start,
within 1e-5 relative."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_yardstick as A
import nncg_cases as C
import nncg_yardstick as N
from test_gpu_als import _context

pytestmark = pytest.mark.gpu

NAMES = "UVZ"
L2 = C.L2


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _ctx(lib, c, F=None):
    X, Y, Wx, Wy, F0, _ = c
    return _context(lib, X, Y, F0 if F is None else F, Wx, Wy)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


def _compare(c, which, steps, got, k, what, cx=0.0, inside=None):
    """The assertions of one comparison; ``inside``: rows of which at least one (every one: measured and printed) must be asserted."""
    r = C.reference(c, which, steps, cx)
    y64, compared, asserted = r["y64"], r["compared"], r["asserted"]
    assert (~asserted).sum() <= 0.1 * len(asserted), what
    assert np.isfinite(got).all() and (got >= 0).all(), what
    assert (got[:, k:] == 0).all(), what
    H, g = C.start_quadratic(c, which, cx)
    q0 = N.quadratic(H, g, np.maximum(c[4][NAMES.index(which)], 0))
    q1 = N.quadratic(H, g, got[:, :k])
    assert (q1 <= q0 + 1e-5 * np.abs(q0)).all(), "%s: the quadratic of row %d rose" % (what, int(np.argmax(q1 - q0)))
    assert (got[A.no_information(*C.relations(c), *c[4], which, cx=cx)] == 0).all(), what     # rows without information
    err = np.abs(got[:, :k] - y64).max(axis=1)
    worst = int(np.argmax(np.where(asserted, err, -1.0)))
    strict = int(np.argmax(np.where(compared, err, -1.0)))
    print("%s: envelope %.3f (%.3e) over %d of %d rows%s; the issue's rule %s over %d rows"
          % (what, err[worst] / r["envelope"], r["envelope"], int(asserted.sum()), len(asserted),
             "" if inside is None else ", %d of %d long rows among them" % (int(asserted[inside].sum()), int(inside.sum())),
             "%.3f (%.3e)" % (err[strict] / r["tol"], r["tol"]) if compared.any() else "-", int(compared.sum())))
    assert inside is None or asserted[inside].any(), what
    assert err[worst] <= r["envelope"], "%s: |err| / envelope = %.3f (%.3e) in row %d" % (what, err[worst] / r["envelope"], r["envelope"], worst)
    assert not compared.any() or err[strict] <= r["tol"], "%s: |err| / tol = %.3f (%.3e) in row %d" % (what, err[strict] / r["tol"], r["tol"], strict)


# ------------------------------------------------------------------ 1. parity of cmf_als_nncg_rows
@pytest.mark.parametrize("yform", ["full", "observed"])
@pytest.mark.parametrize("k", C.KS)
def test_rows_against_the_yardstick(lib, k, yform):
    c = C.case(k, yform)
    ctx = _ctx(lib, c)
    assert ctx.als_nncg_last() == (0, 0)
    for which in C.sweeps(yform):
        w = NAMES.index(which)
        n = c[4][w].shape[0]
        for steps in C.STEPS:
            got = ctx.als_nncg_rows(w, 0, n, L2, steps)
            assert ctx.als_nncg_last() == (0, 0)                                    # no row is longer than the default piece
            _compare(c, which, steps, got, k, "k %d Y %s sweep %s, %d steps" % (k, yform, which, steps))
            passes, entry_passes = ctx.als_nncg_passes()
            lens = C.row_lengths(c, which)
            ref_passes = N.rows(*C.relations(c), *c[4], which, L2, steps)[3]
            assert n <= passes <= (2 * steps + 1) * n and entry_passes <= (2 * steps + 1) * lens.sum()
            if C.reference(c, which, steps)["asserted"].all():
                assert passes == ref_passes.sum() and entry_passes == (ref_passes * lens).sum()
        if which == "U":
            assert (got[4] == 0).all()                                              # the empty row of X
    if yform == "full":
        with pytest.raises(ValueError, match="no observed relation"):
            ctx.als_nncg_rows(2, 0, 20, L2, 3)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="nn_cg_steps must be 1 .. 1024"):
            ctx.als_nncg_rows(0, 0, 40, L2, bad)
    assert all(_bits(ctx.get_factor(w)) == _bits(c[4][w]) for w in range(3))      # the factors are left alone
    ctx.close()


# ------------------------------------------------------------------ 2. bits
@pytest.mark.parametrize("k", C.KS)
def test_a_row_depends_on_the_row_alone(lib, k):
    c = C.case(k, "observed")
    ctx = _ctx(lib, c)
    entry = 4 * ctx.geometry()[3] + 4
    for which in "UV":
        w = NAMES.index(which)
        n = c[4][w].shape[0]
        full = ctx.als_nncg_rows(w, 0, n, L2, 6)
        assert ctx.als_nncg_rows(w, 0, n, L2, 6).tobytes() == full.tobytes()                       # a repeated call
        assert ctx.als_nncg_rows(w, 2, 7, L2, 6).tobytes() == full[2:9].tobytes()                  # inside a sub-range
        for lds in (0, 20 * entry, -1):                                                             # streamed, mixed, the default
            ctx.set_option("als_cg_lds", lds)
            assert ctx.als_nncg_rows(w, 0, n, L2, 6).tobytes() == full.tobytes(), "als_cg_lds = %d" % lds
    ctx.close()


# ------------------------------------------------------------------ 3. long rows
@pytest.mark.parametrize("yform", ["full", "observed"])
@pytest.mark.parametrize("k", C.KS)
def test_long_rows_through_pieces_of_32(lib, k, yform):
    """"als_cg_piece" 32: row 0 of X (70 entries: 3 pieces) in the U sweep, and under an observed Y the columns of X with more than
    12 entries in the V sweep (20 entries of Y behind them: the first piece straddles the two sides)."""
    c = C.case(k, yform)
    ctx = _ctx(lib, c)
    ctx.set_option("als_cg_piece", 32)
    for which in ("UVZ" if yform == "observed" else "U"):
        w = NAMES.index(which)
        n = c[4][w].shape[0]
        want = C.long_rows_and_pieces(c, which, 32)
        assert want[0] > 0
        if which == "V":
            Rx, _ = C.relations(c)
            n0 = Rx.row_lengths(True)
            assert ((n0 > 0) & (n0 < 32) & (n0 + 20 > 32)).any()                                   # a piece straddles the two sides
        lens = C.row_lengths(c, which)
        for steps in C.STEPS:
            got = ctx.als_nncg_rows(w, 0, n, L2, steps)
            assert ctx.als_nncg_last() == want
            _compare(c, which, steps, got, k, "pieces of 32, k %d Y %s sweep %s, %d steps" % (k, yform, which, steps), inside=lens > 32)
            assert ctx.als_nncg_rows(w, 0, n, L2, steps).tobytes() == got.tobytes()                 # a repeated call
        i = int(np.flatnonzero(lens > 32)[0])
        assert ctx.als_nncg_rows(w, i, 1, L2, steps).tobytes() == got[i:i + 1].tobytes()           # a long row solved alone
        ctx.set_option("als_cg_piece", 0)
        uncut = ctx.als_nncg_rows(w, 0, n, L2, steps)
        assert ctx.als_nncg_last() == (0, 0)
        assert uncut[lens <= 32].tobytes() == got[lens <= 32].tobytes()                            # short rows keep their bits
        ctx.set_option("als_cg_piece", 32)
    ctx.close()


# ------------------------------------------------------------------ 4. background weight
@pytest.mark.parametrize("k", C.KS)
def test_background_weight(lib, k):
    """c0 = 1 on X, weights 1 + rand: the excess weights and S = c0 V^T V (U sweep) / c0 U^T U + Z^T Z (V sweep, Y full)."""
    c = C.case(k, "full", bg=True)
    ctx = _ctx(lib, c)
    ctx.set_background_weight(0, 1.0)
    for which in "UV":
        w = NAMES.index(which)
        for steps in C.STEPS:
            got = ctx.als_nncg_rows(w, 0, c[4][w].shape[0], L2, steps)
            _compare(c, which, steps, got, k, "background 1, k %d sweep %s, %d steps" % (k, which, steps), cx=1.0)
    ctx.close()


# ------------------------------------------------------------------ 5. steps and fits
@pytest.mark.parametrize("k", [3, 40])
def test_one_step_against_the_yardstick(lib, k):
    """cmf_als_nncg_step, all factors non-negative, Y full: V and U by 3 projected CG steps, Z (no observed relation) by 2 passes of
    HALS; factor by factor against the yardstick's step, every factor from the device's previous ones so that one sweep is compared
    at a time."""
    c = C.case(k, "full")
    Rx, Ry = C.relations(c)
    ctx = _ctx(lib, c)
    F = [np.asarray(M, dtype=np.float64) for M in c[4]]
    for which, bit in (("V", 2), ("U", 1), ("Z", 4)):
        w = NAMES.index(which)
        ctx.als_nncg_step(L2, 7, bit, 0, 3, 2)
        got = ctx.get_factor(w)
        assert (got >= 0).all() and np.isfinite(got).all()
        y = [N.sweep(Rx, Ry, *F, which, L2, non_negative=True, nn_sweeps=2, nn_cg_steps=3, dtype=dt) for dt in (np.float64, np.float32)]
        if which == "Z":
            ok = np.ones(len(got), dtype=bool)
        else:
            t64, t32 = (N.rows(Rx, Ry, *F, which, L2, 3, dtype=dt)[1] for dt in (np.float64, np.float32))
            ok = np.array([a == b for a, b in zip(t64, t32)])
        assert (~ok).sum() <= 0.1 * len(ok)
        tol = A.tolerance(y[1][ok], y[0][ok], k)
        err = float(np.abs(got - y[0])[ok].max())
        print("k %d step, factor %s: |err| / tol %.3f (tol %.3e), %d rows left out" % (k, which, err / tol, tol, int((~ok).sum())))
        assert err <= tol
        F[w] = got.astype(np.float64)
        for other in range(3):
            if other != w:
                assert _bits(ctx.get_factor(other)) == _bits(F[other])
    ctx.close()


def test_ten_iterations_of_a_fit_never_raise_the_objective(lib):
    """CMF(solver="als", als_nn_cg_steps=4), every factor non-negative (the default), X observed, Y full with 2 passes of HALS for
    Z: the float64 objective of the returned factors after 1 .. 10 iterations never rises and ends below half the start; the
    factors are >= 0."""
    from pycmf_amd import CMF
    X, Y, Wx, Wy, F, _ = C.case(40, "full")
    Rx, Ry = C.relations(C.case(40, "full"))
    Xs = sp.csr_matrix(X * Wx.toarray())                                            # (X > 0: stored exactly on the pattern; weights 1)
    assert Xs.nnz == Wx.nnz
    seq = [A.objective(Rx, Ry, None, None, *F, L2)]
    for it in range(1, 11):
        model = CMF(n_components=40, solver="als", l2_reg=L2, als_nn_cg_steps=4, als_nn_sweeps=2, max_iter=it, tol=0, x_init="custom", y_init="custom")
        got = model.fit_transform(Xs, Y, U=F[0].copy(), V=F[1].copy(), Z=F[2].copy(), x_entry_weights="observed")
        assert model.n_iter_ == it and all((G >= 0).all() and np.isfinite(G).all() for G in got)
        seq.append(A.objective(Rx, Ry, None, None, *got, L2))
    print("objective: " + " ".join("%.6e" % v for v in seq))
    assert all(b <= a for a, b in zip(seq, seq[1:])) and seq[-1] < 0.5 * seq[0]
    # the fold-in honours the keyword: new rows of X against the fixed V, by the same route
    U2 = model.transform(Xs, None, x_entry_weights="observed")[0]
    assert U2.shape == got[0].shape and (U2 >= 0).all() and np.isfinite(U2).all()


@pytest.mark.parametrize("k", [3, 200])
def test_without_a_factor_on_the_new_route_the_step_is_the_parents(lib, k):
    c = C.case(k, "observed")
    ctx, ref = _ctx(lib, c), _ctx(lib, c)
    ctx.als_nncg_step(L2, 0, 7, 3, 5, 0)                                            # every factor signed: cmf_als_cg_step
    ref.als_cg_step(L2, 0, 7, 3, 0)
    assert all(ctx.get_factor(w).tobytes() == ref.get_factor(w).tobytes() for w in range(3))
    ctx.als_nncg_step(L2, 1, 6, 0, 5, 2)                                            # the non-negative factor is not swept: exact rows
    ref.als_step(L2, 1, 6)
    assert all(ctx.get_factor(w).tobytes() == ref.get_factor(w).tobytes() for w in range(3))
    ctx.close()
    ref.close()
    full = C.case(k, "full")
    ctx, ref = _ctx(lib, full), _ctx(lib, full)
    ctx.als_nncg_step(L2, 4, 4, 0, 5, 2)                                            # Z non-negative without an observed relation: HALS
    ref.als_nnls_step(L2, 4, 4, 2)
    assert all(ctx.get_factor(w).tobytes() == ref.get_factor(w).tobytes() for w in range(3))
    ctx.close()
    ref.close()


def test_logistic_and_biased_relations_are_refused_and_the_context_stays_usable(lib):
    from pycmf_amd import CMF
    c = C.case(3, "observed")
    X, Y, Wx, Wy, F, _ = c
    ctx = _ctx(lib, c)
    want = ctx.als_nncg_rows(0, 0, 40, L2, 3)
    ctx.set_relation_loss(0, "logistic")
    with pytest.raises(NotImplementedError, match="non-negative conjugate-gradient rows have no reweighting pass"):
        ctx.als_nncg_step(L2, 7, 1, 0, 3, 0)
    with pytest.raises(NotImplementedError, match="non-negative conjugate-gradient rows have no reweighting pass"):
        ctx.als_nncg_rows(0, 0, 40, L2, 3)
    before = ctx.get_factor(2).tobytes()
    ctx.als_nncg_step(L2, 7, 4, 0, 3, 0)                                            # the Z sweep reads Y alone, which is Frobenius
    assert ctx.get_factor(2).tobytes() != before
    ctx.set_relation_loss(0, "frobenius")
    ctx.set_biases(1, True, 0.5, 0.1)
    with pytest.raises(NotImplementedError, match="Y has biases bound"):
        ctx.als_nncg_step(L2, 7, 2, 0, 3, 0)
    with pytest.raises(NotImplementedError, match="Y has biases bound"):
        ctx.als_nncg_rows(2, 0, 20, L2, 3)
    for bad in (dict(cg=-1, nn=3, sw=0), dict(cg=0, nn=0, sw=0), dict(cg=0, nn=1025, sw=0), dict(cg=0, nn=3, sw=1025)):
        with pytest.raises(ValueError, match="must be . .. 1024"):
            ctx.als_nncg_step(L2, 7, 1, bad["cg"], bad["nn"], bad["sw"])
    assert ctx.als_nncg_rows(0, 0, 40, L2, 3).tobytes() == want.tobytes()           # the U sweep reads X alone: usable, same bits
    ctx.close()
    kw = dict(n_components=3, solver="als", l2_reg=L2, als_nn_cg_steps=3, max_iter=2)
    with pytest.raises(ValueError, match="with loss='logistic' is not built"):
        CMF(loss="logistic", x_link="logit", **kw).fit(sp.csr_matrix((X > 1) * Wx.toarray()), Y, x_entry_weights=Wx)
    with pytest.raises(ValueError, match="with x_biases / y_biases is not built"):
        CMF(**kw).fit(sp.csr_matrix(X * Wx.toarray()), Y, x_entry_weights="observed", x_biases=True)
