"""ALS with a global mean and row / column biases on the device (cmf_set_biases, cmf_als_bias_step, cmf_als_bias_rows,
cmf_predict_pairs; csrc/cmf_als_bias.hip.h) against the float64 yardstick of als_bias_yardstick.py on the fixtures of
als_bias_cases.py (the patterns of als_cg_pieces_cases.py: rows of 0, 1, 63, 64, 65, 128, 129, 200, 333, 640 entries; pieces of 64).
Tolerance per comparison: the rule of the project, als_yardstick.tolerance with the cap assertion of test_gpu_als_implicit.py
(``_tol``): 4 max|y32 - y64| <= 1e-3 max|y64|, per factor and per bias vector.

Measured on an MI355X (worst |err| / tol of each group): see DESIGN section 20."""
import numpy as np
import pytest
import scipy.sparse as sp

import als_bias_cases as C
import als_bias_yardstick as B
import als_cg_pieces_cases as P
import als_yardstick as A
from test_gpu_als import _context
from test_gpu_als_implicit import _tol

pytestmark = pytest.mark.gpu

L2, LB = C.L2, C.LB


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _bias_on(ctx, which, bias, lb=LB):
    ctx.set_biases(which, True, bias[0], lb)
    ctx.set_bias(which, 0, bias[1])
    ctx.set_bias(which, 1, bias[2])


def _ctx(lib, name, k, piece=C.PIECE, F=None, biased=True):
    X, Y, Wx, Wy, F0, _ = P.case(name, k)
    ctx = _context(lib, X, Y, F0 if F is None else F, Wx, Wy)
    ctx.set_option("als_bias_piece", piece)
    if biased:
        for which, bias in enumerate(C.biases(name, k)):
            _bias_on(ctx, which, bias)
    return ctx


def _state(ctx):
    return [ctx.get_factor(w) for w in range(3)] + [ctx.get_bias(which, axis) for which in (0, 1) for axis in (0, 1)]


# ------------------------------------------------------------------ 1. exact arithmetic
@pytest.mark.parametrize("k", C.KS)
def test_exact_inputs_give_the_float64_biases_and_targets(lib, k):
    """The patterns of cases A and B with one-hot factor rows times powers of two, weights in {1/2, 1, 2, 4}, targets, biases and mu
    multiples of 1/4: every term, every partial sum, bt and bp are exact in float32, so any order of summation gives the float64
    values and the device must return them with == (the biases: the float64 quotient rounded once).  Pins the roles of r and c on the
    transposed image, the column map and the pieces."""
    for name in ("A", "B"):
        X, Y, Wx, Wy, F0, _ = P.case(name, k)
        rng = np.random.RandomState(k)
        Ts = [rng.randint(-8, 9, size=T.shape) / 4.0 for T in (X, Y)]
        Ws = []
        for W in (Wx, Wy):
            W = W.copy()
            W.data = 2.0 ** rng.randint(-1, 3, size=W.nnz)
            Ws.append(W)
        F = []
        for n in (X.shape[0], X.shape[1], Y.shape[1]):
            f = np.zeros((n, k))
            f[np.arange(n), rng.randint(0, k, size=n)] = 2.0 ** rng.randint(-1, 2, size=n)
            F.append(f)
        rels = (A.Relation(Ts[0], Ws[0]), A.Relation(Ts[1], Ws[1]))
        bias = [(0.5 if which == 0 else -1.25, rng.randint(-4, 5, size=rel.shape[0]) / 4.0, rng.randint(-4, 5, size=rel.shape[1]) / 4.0)
                for which, rel in enumerate(rels)]
        ctx = _context(lib, Ts[0], Ts[1], F, Ws[0], Ws[1])
        ctx.set_option("als_bias_piece", 64)
        for which in (0, 1):
            _bias_on(ctx, which, bias[which], lb=0.25)
        for which, rel in enumerate(rels):
            Fa, Fb = (F[0], F[1]) if which == 0 else (F[1], F[2])
            adj = B.adjusted(rel, bias[which])
            for axis in (0, 1):
                want = B.bias_sweep(rel, Fa, Fb, bias[which], 0.25, axis)
                got = ctx.als_bias_rows(which, axis)
                assert (got == want.astype(np.float32)).all() and (want != 0).any(), (name, which, axis, int((got != want.astype(np.float32)).sum()))
                _, _, bt, w = adj.images[axis]
                gbt, gbp = ctx.als_bias_targets(which, axis, len(bt))
                assert (gbt.astype(np.float64) == bt).all() and (gbp.astype(np.float64) == w * bt).all(), (name, which, axis)
        ctx.close()


# ------------------------------------------------------------------ 2. bias sweeps against the yardstick
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("k", C.KS)
def test_bias_sweeps_against_the_yardstick(lib, k, name):
    ctx = _ctx(lib, name, k)
    rels = P.relations(P.case(name, k))
    worst = worst_cap = 0.0
    first = {}
    for piece in (64, 128, -1):
        ctx.set_option("als_bias_piece", piece)
        for which in (0, 1):
            for axis in (0, 1):
                y64, y32 = C.sweep_reference(name, k, which, axis, piece)
                what = "case %s k %d relation %d axis %d L %d" % (name, k, which, axis, piece)
                tol, cap = _tol(y32, y64, k, what)
                got = ctx.als_bias_rows(which, axis)
                err = float(np.abs(got - y64).max())
                worst, worst_cap = max(worst, err / tol), max(worst_cap, cap)
                print("%s: |err| / tol %.3f (tol %.3e), cap %.4f" % (what, err / tol, tol, cap))
                assert np.isfinite(got).all() and err <= tol
                empty = rels[which].row_lengths(axis == 1) == 0
                assert (got[empty] == 0).all() and ((y64 == 0) == empty).all()
                assert ctx.als_bias_rows(which, axis).tobytes() == got.tobytes()                      # a repeated call
                lens = rels[which].row_lengths(axis == 1)
                if piece == 64:
                    first[(which, axis)] = got
                else:                                                                                  # a row no longer than both piece lengths is cut the same way
                    same = lens <= 64
                    assert same.any() and got[same].tobytes() == first[(which, axis)][same].tobytes()
    assert any((rels[w].row_lengths(t) == 0).any() for w in (0, 1) for t in (False, True))
    print("case %s k %d: worst |err| / tol %.3f, worst cap %.4f" % (name, k, worst, worst_cap))
    ctx.close()


@pytest.mark.parametrize("k", [40, 256])
def test_a_bias_depends_on_its_own_row_alone(lib, k):
    """The same rows inside a sub-pattern (the other rows emptied; for the column sweep the other columns) give the same bytes."""
    for name in ("A", "B"):
        X, Y, Wx, Wy, F, _ = P.case(name, k)
        bias = C.biases(name, k)[0]
        full = _ctx(lib, name, k)
        for axis in (0, 1):
            whole = full.als_bias_rows(0, axis)
            n = Wx.shape[axis]
            keep = np.zeros(n, dtype=bool)
            keep[::3] = True
            keep[np.argmax(np.diff(Wx.indptr) if axis == 0 else np.diff(Wx.tocsc().indptr))] = True      # the longest row stays
            D = sp.diags(keep.astype(np.float64))
            Wsub = sp.csr_matrix(D @ Wx if axis == 0 else Wx @ D)
            Wsub.eliminate_zeros()
            ctx = _context(lib, X, Y, F, Wsub, Wy)
            ctx.set_option("als_bias_piece", C.PIECE)
            _bias_on(ctx, 0, bias)
            part = ctx.als_bias_rows(0, axis)
            assert part[keep].tobytes() == whole[keep].tobytes() and (part[~keep] == 0).all() and (whole[keep] != 0).any()
            ctx.close()
        full.close()


# ------------------------------------------------------------------ 3. full steps
@pytest.mark.parametrize("case, k, mask, route", C.STEP_CASES)
def test_full_step(lib, case, k, mask, route):
    """cmf_als_bias_step, pieces of 64: exact rows | 3 CG steps | V non-negative by 4 coordinate-descent passes; case B (long rows in
    the V sweep), and case A (long rows in the U and Z sweeps) for masks 1 and 4 of the CG route.  The cases are those whose float32
    and float64 yardstick runs agree within the cap (als_bias_cases.STEP_CASES says which are left out and by how much;
    test_als_bias_host.py asserts it on the CPU)."""
    kw = C.ROUTES[route]
    F = C.factors(case, k, kw["nn_mask"])
    s64, s32 = C.step_reference(case, k, mask, route)
    ctx = _ctx(lib, case, k, F=F)
    before = [a.tobytes() for a in _state(ctx)]
    ctx.als_bias_step(L2, kw["nn_mask"], mask, kw["cg_steps"], kw["nn_sweeps"])
    got = _state(ctx)
    report = []
    for i, ((name, y64), (_, y32)) in enumerate(zip(C.step_vectors(s64), C.step_vectors(s32))):
        if not C.MOVED[name] & mask:
            assert got[i].tobytes() == before[i], "%s is outside the mask and changed" % name
            continue
        tol, cap = _tol(y32, y64, k, "case %s k %d mask %d %s %s" % (case, k, mask, route, name))
        err = float(np.abs(got[i] - y64).max())
        report.append("%s %.3f" % (name, err / tol))
        assert np.isfinite(got[i]).all() and err <= tol, "%s: |err| / tol = %.3f (tol %.3e)" % (name, err / tol, tol)
    if kw["nn_mask"] & mask & 2:
        assert (got[1] >= 0).all()
    print("case %s k %d mask %d %s: |err| / tol %s" % (case, k, mask, route, " ".join(report)))
    ctx.close()


# ------------------------------------------------------------------ 4. no biases bound: the present bytes
@pytest.mark.parametrize("k", [7, 256])
def test_without_biases_every_route_keeps_its_bytes(lib, k):
    def run(prepare, step):
        ctx = _ctx(lib, "B", k, biased=False)
        prepare(ctx)
        out = step(ctx)
        state = b"".join(ctx.get_factor(w).tobytes() for w in range(3))
        ctx.close()
        return state, out

    def nothing(ctx):
        pass

    def on_and_off(ctx):
        for which, bias in enumerate(C.biases("B", k)):
            _bias_on(ctx, which, bias)
        ctx.als_bias_step(L2, 0, 7, 0, 0)
        for w in range(3):
            ctx.set_factor(w, P.case("B", k)[4][w])
        for which in (0, 1):
            ctx.set_biases(which, False)
            assert ctx.get_biases(which) == (0.0, 0.0, False)

    steps = {"als_step": lambda ctx: ctx.als_step(L2, 0, 7), "als_cg_step": lambda ctx: ctx.als_cg_step(L2, 0, 7, 3, 0),
             "als_nn": lambda ctx: ctx.als_cg_step(L2, 2, 7, 3, 4), "residual": lambda ctx: ctx.als_residual_sq()}
    fresh = {name: run(nothing, step) for name, step in steps.items()}
    # cmf_als_bias_step with no relation biased IS the step with the same arguments
    assert run(nothing, lambda ctx: ctx.als_bias_step(L2, 0, 7, 3, 0))[0] == fresh["als_cg_step"][0]
    assert run(nothing, lambda ctx: ctx.als_bias_step(L2, 2, 7, 3, 4))[0] == fresh["als_nn"][0]
    assert run(nothing, lambda ctx: ctx.als_bias_step(L2, 0, 7, 0, 0))[0] == fresh["als_step"][0]
    # after cmf_set_biases(..., enable = 0) the context is one that never had biases
    for name, step in steps.items():
        assert run(on_and_off, step) == fresh[name], name
    assert len(set(v[0] for v in fresh.values())) >= 3


# ------------------------------------------------------------------ 5. descent
@pytest.mark.parametrize("route", sorted(C.ROUTES))
def test_five_steps_never_raise_the_objective(lib, route):
    """Case B at k = 40, pieces of 64: the float64 objective of the device's factors and biases never rises by more than 1e-6
    relative -- the float32 rounding of a monotone method."""
    kw = dict(C.ROUTES[route])
    if route == "cg":
        kw["cg_steps"] = 6
    if route == "nn":
        kw["nn_mask"] = 7
    F = C.factors("B", 40, kw["nn_mask"])
    Rx, Ry = P.relations(P.case("B", 40))
    bx, by = C.biases("B", 40)
    ctx = _ctx(lib, "B", 40, F=F)
    seq = [B.objective(Rx, Ry, None, None, *F, bx, by, L2, LB)]
    for _ in range(5):
        ctx.als_bias_step(L2, kw["nn_mask"], 7, kw["cg_steps"], kw["nn_sweeps"])
        s = _state(ctx)
        seq.append(B.objective(Rx, Ry, None, None, s[0], s[1], s[2], (bx[0], s[3], s[4]), (by[0], s[5], s[6]), L2, LB))
    print("%s objective: %s" % (route, " ".join("%.6e" % v for v in seq)))
    assert all(b <= a * (1 + 1e-6) for a, b in zip(seq, seq[1:])) and seq[-1] < seq[0]
    ctx.close()


# ------------------------------------------------------------------ 6. prediction of given cells
@pytest.mark.parametrize("k", C.KS)
def test_predict_pairs(lib, k):
    F = P.case("B", k)[4]
    rng = np.random.RandomState(k)
    worst = 0.0
    for biased in (False, True):
        ctx = _ctx(lib, "B", k, biased=biased)
        for which in (0, 1):
            Fa, Fb = (F[0], F[1]) if which == 0 else (F[1], F[2])
            bias = C.biases("B", k)[which] if biased else None
            n = 1000
            rows, cols = rng.randint(0, Fa.shape[0], size=n), rng.randint(0, Fb.shape[0], size=n)
            rows[100:110], cols[100:110] = rows[5], cols[5]                                          # repeated pairs
            rows[-1], cols[-1] = Fa.shape[0] - 1, Fb.shape[0] - 1
            bound = B.predict_bound(Fa, Fb, rows, cols, k, bias)
            for link in ("linear", "logit"):
                want = B.predict(Fa, Fb, rows, cols, bias, link)
                got = ctx.predict_pairs(which, rows, cols, link=link)
                assert got.dtype == np.float32 and np.isfinite(got).all()
                ratio = float((np.abs(got - want) / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (k, biased, which, link, ratio)
                assert ctx.predict_pairs(which, rows, cols, link=link).tobytes() == got.tobytes()  # a repeated call
                assert (got[100:110] == got[5]).all()
                sub = np.r_[7:300:3, 999]                                                          # ... does not depend on the other pairs
                assert ctx.predict_pairs(which, rows[sub], cols[sub], link=link).tobytes() == got[sub].tobytes()
                assert ctx.predict_pairs(which, rows[:1], cols[:1], link=link)[0] == got[0]
            assert ctx.predict_pairs(which, [], []).shape == (0,)
        ctx.close()
    print("k %d: worst |err| / bound %.3f" % (k, worst))


def test_top_n_and_ranks_of_a_biased_model_are_the_predictions(lib):
    from pycmf_amd import CMF
    from pycmf_amd.estimator import FittedBias
    k = 40
    X, Y, Wx, Wy, F, _ = P.case("B", k)
    bx, by = C.biases("B", k)
    model = CMF(n_components=k, solver="als", l2_reg=L2)
    model.x_weights, model.components, model.y_weights = F
    model.x_bias_, model.y_bias_ = FittedBias(*bx), FittedBias(*by)
    for relation, axis, seen, bias in (("x", 0, Wx, bx), ("x", 1, Wx, bx), ("y", 0, Wy, by)):
        Fa, Fb = (F[0], F[1]) if relation == "x" else (F[1], F[2])
        rows = np.arange(0, (Fa if axis == 0 else Fb).shape[0], 7) if relation == "x" else np.array([1, 7])  # (row 0 of Y stores all 300 cells)
        idx, val = model.top_n(relation=relation, axis=axis, rows=rows, n=5, exclude=seen)
        assert (idx >= 0).all()
        q = np.repeat(rows, 5)
        r_, c_ = (q, idx.ravel()) if axis == 0 else (idx.ravel(), q)
        pred = model.predict(r_, c_, relation=relation)
        want = B.predict(Fa, Fb, r_, c_, bias)
        bound = B.predict_bound(Fa, Fb, r_, c_, k, bias)                                             # (k + 16) 2^-24 (|offset| + |r| + |c| + sum |a||b|)
        worst = max(float((np.abs(val.ravel().astype(np.float64) - want) / bound).max()), float((np.abs(pred - want) / bound).max()))
        print("%s axis %d: top_n and predict against float64, worst |err| / bound %.3f" % (relation, axis, worst))
        assert worst <= 1.0
        S = seen.toarray() if axis == 0 else seen.toarray().T
        assert (S[q, idx.ravel()] == 0).all()
        # ranks agree with top_n place for place
        shape = (Fa.shape[0], Fb.shape[0])
        held = sp.csr_matrix((np.ones(q.size), (r_, c_)), shape=shape)
        indptr, indices, rank, eligible = model.ranks(held, relation=relation, axis=axis, exclude=seen, rows=rows)
        for i in range(len(rows)):
            got = dict(zip(indices[indptr[i]:indptr[i + 1]], rank[indptr[i]:indptr[i + 1]]))
            assert [got[j] for j in idx[i]] == list(range(5)), (relation, axis, i)
    # queries with their own biases: the fitted rows handed back as queries give the same lists
    rows = np.arange(0, 700, 50)
    idx, val = model.top_n(rows=rows, n=5)
    idx2, val2 = model.top_n(queries=F[0][rows], query_bias=bx[1][rows], n=5)
    assert (idx == idx2).all() and val.tobytes() == val2.tobytes()
    idx3, _ = model.top_n(queries=F[0][rows], n=5)                                                  # default query bias 0: the order is the same, the values shift
    assert (idx3 == idx).all()


# ------------------------------------------------------------------ 7. end to end
def test_fit_score_and_fold_in_through_the_estimator(lib):
    """The planted rating problem at 10 % observed (seed 3, noise 0.3, l2 = 0.5), rank 3, 10 iterations from the problem's start: the
    fit ends within 1e-4 relative of the yardstick's objective, score_entries gives its RMSE on the unobserved cells to three digits,
    and transform of 16 held-back rows reproduces the yardstick's fold-in (U and r) inside the rule."""
    from pycmf_amd import CMF
    l2 = 0.5
    X, Y, Wx, (U0, V0, Z0) = B.planted(3, 0.10, 0.30, k=3)
    fit_rows, new_rows = np.arange(104), np.arange(104, 120)
    Xf, Wf = X[fit_rows], sp.csr_matrix(Wx[fit_rows])
    Rx, Ry = A.Relation(Xf, Wf), A.Relation(Y, None)
    trace = []
    Uy, Vy, Zy, bxy, _ = B.fit(Rx, Ry, None, None, U0[fit_rows], V0, Z0, 10, l2, x_biases=True, trace=trace)
    signed = dict(U_non_negative=False, V_non_negative=False, Z_non_negative=False)
    model = CMF(n_components=3, solver="als", l2_reg=l2, max_iter=10, tol=0, x_init="custom", y_init="custom", **signed)
    model.fit(Xf, Y, U=U0[fit_rows].copy(), V=V0.copy(), Z=Z0.copy(), x_entry_weights=Wf, x_biases=True)
    assert model.y_bias_ is None and model.x_bias_.rows.shape == (104,) and model.x_bias_.cols.shape == (150,)
    assert model.x_bias_.offset == B.weighted_mean(Rx)
    obj = B.objective(Rx, Ry, None, None, model.x_weights, model.components, model.y_weights, model.x_bias_.as_tuple(), None, l2, l2)
    print("objective: device %.8e, yardstick %.8e" % (obj, trace[-1]))
    assert abs(obj - trace[-1]) <= 1e-4 * trace[-1]
    miss = sp.csr_matrix(np.where(Wf.toarray() == 0, Xf, 0.0))
    assert miss.nnz == int((Wf.toarray() == 0).sum())
    score = model.score_entries(miss)
    want = B.heldout_rmse(Xf, Wf, Uy, Vy, bxy)
    print("held-out RMSE: device %.5f, yardstick %.5f" % (score["rmse"], want))
    assert score["n"] == miss.nnz and abs(score["rmse"] - want) <= 0.5e-3 and 0.35 < want < 0.5
    # fold-in of the 16 held-back rows against the DEVICE's V, c and mu
    Xn, Wn = X[new_rows], sp.csr_matrix(Wx[new_rows])
    Un, _, _ = model.transform(Xn, None, x_entry_weights=Wn)
    rn = model.transform_x_row_bias_
    Rn = A.Relation(Xn, Wn)
    start = (model.x_bias_.offset, np.zeros(16), model.x_bias_.cols)
    refs = [B.fit(Rn, Ry, None, None, np.zeros((16, 3)), model.components, model.y_weights, 10, l2, bx=start, mask=1, dtype=dt,
                  piece=(2048 if dt is np.float32 else None)) for dt in (np.float64, np.float32)]
    for name, got, y64, y32 in (("U", Un, refs[0][0], refs[1][0]), ("r", rn, refs[0][3][1], refs[1][3][1])):
        tol, cap = _tol(y32, y64, 3, "fold-in %s" % name)
        err = float(np.abs(got - y64).max())
        print("fold-in %s: |err| / tol %.3f (tol %.3e), cap %.4f" % (name, err / tol, tol, cap))
        assert err <= tol and np.abs(y64).max() > 0.1
    assert (refs[0][3][2] == model.x_bias_.cols).all() and model.transform_y_col_bias_ is None


# ------------------------------------------------------------------ 8. refusals leave the context usable
def test_refusals_leave_the_context_usable(lib):
    k = 7
    bx, by = C.biases("B", k)
    F = P.case("B", k)[4]
    ctx = _ctx(lib, "B", k)
    good = ctx.als_bias_rows(0, 0).tobytes()
    with pytest.raises(NotImplementedError, match=r"cmf_set_background_weight: X has biases bound.*cmf_set_biases\(ctx, 0, 0, 0, 0\)"):
        ctx.set_background_weight(0, 0.25)
    assert ctx.get_background_weight(0) == 0.0 and ctx.get_biases(0) == (bx[0], LB, True) and ctx.als_bias_rows(0, 0).tobytes() == good
    ctx.set_background_weight(0, 0.0)                                                                 # clearing what is not there is fine
    with pytest.raises(NotImplementedError, match=r"cmf_mu_weighted_step: X has biases bound.*cmf_set_biases\(ctx, 0, 0, 0, 0\)"):
        ctx.mu_weighted_step(0.0, 0.0, 1)
    assert ctx.als_bias_rows(0, 0).tobytes() == good
    for rows, cols in (([0, 700], [0, 0]), ([0, 1], [0, 12]), ([-1], [0])):
        with pytest.raises(ValueError, match="cmf_predict_pairs: pair . = .* lies outside the 700 x 12 relation"):
            ctx.predict_pairs(0, rows, cols)
    with pytest.raises(ValueError, match="which must be 0"):
        ctx.predict_pairs(2, [0], [0])
    assert ctx.predict_pairs(0, [699], [11]).shape == (1,) and ctx.als_bias_rows(0, 0).tobytes() == good
    for bad in (dict(mu=np.nan), dict(mu=np.inf), dict(lb=-1.0), dict(lb=np.nan)):
        with pytest.raises(ValueError, match="cmf_set_biases: mu must be finite"):
            ctx.set_biases(0, True, **bad)
        assert ctx.get_biases(0) == (bx[0], LB, True)
    ctx.set_biases(0, False)
    with pytest.raises(ValueError, match="X has no biases bound"):
        ctx.als_bias_rows(0, 0)
    ctx.set_background_weight(0, 0.25)                                                                # the other order
    with pytest.raises(NotImplementedError, match=r"cmf_set_biases: X has a background weight bound.*cmf_set_background_weight\(ctx, 0, 0\)"):
        ctx.set_biases(0, True, 0.5, LB)
    assert ctx.get_biases(0) == (0.0, 0.0, False) and ctx.get_background_weight(0) == 0.25
    ctx.als_cg_step(L2, 0, 7, 3, 0)                                                                   # the background fit goes on
    ctx.set_background_weight(0, 0.0)
    _bias_on(ctx, 0, bx)
    for w in range(3):
        ctx.set_factor(w, F[w])
    assert ctx.als_bias_rows(0, 0).tobytes() == good
    # new weights drop the biases, as they drop a background
    X, Y, Wx, Wy, _, _ = P.case("B", k)
    r = np.repeat(np.arange(Wx.shape[0]), np.diff(Wx.indptr))
    ctx.set_weighted_csr(0, Wx.indptr, Wx.indices, X[r, Wx.indices], Wx.data)
    assert ctx.get_biases(0) == (0.0, 0.0, False) and ctx.get_biases(1) == (by[0], LB, True)
    ctx.close()
    # a relation without CSR weights cannot carry biases; k_pad > 256 has no pair kernel
    ctx = lib.Context(0)
    ctx.set_problem(20, 30, 10, 300)
    ctx.set_data(0, np.ones((20, 30)))
    with pytest.raises(ValueError, match="X has no CSR weights bound"):
        ctx.set_biases(0, True, 0.0, 0.0)
    with pytest.raises(NotImplementedError, match="cmf_predict_pairs: n_components <= 256 only"):
        ctx.predict_pairs(0, [0], [0])
    assert ctx.get_factor(0).shape == (20, 300) and ctx.get_biases(0) == (0.0, 0.0, False)
    ctx.close()
