"""Held-out ranking evaluation on the device (cmf_rank / cmf_rank_queries, CMF.ranks / evaluate, rank_products): exact ranks
against NumPy on exact arithmetic, bit-consistency with top-n, and a derived band around the float64 ranks on float factors."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import topk_yardstick as Y

pytestmark = pytest.mark.gpu

U_, V_, Z_ = 0, 1, 2
PAIRS = [(U_, V_), (V_, U_), (V_, Z_), (Z_, V_)]


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _factors(m, d, p, k, signed, seed):           # test_gpu_topk._factors
    rng = np.random.RandomState(seed)
    if signed:
        return [0.3 * rng.randn(r, k) for r in (m, d, p)]
    return [np.abs(rng.randn(r, k)) for r in (m, d, p)]


def _context(lib, F):
    ctx = lib.Context(0)
    ctx.set_problem(F[0].shape[0], F[1].shape[0], F[2].shape[0], F[0].shape[1])
    for w in range(3):
        ctx.set_factor(w, F[w])
    return ctx


def _csr(mask):
    """CSR pair of a boolean mask (rows ascending by construction)."""
    m = sp.csr_matrix(mask.astype(float))
    m.sort_indices()
    return m.indptr.astype(np.int64), m.indices.astype(np.int32)


def _lists(rows):
    """CSR pair of a list of per-query index lists (sorted, merged)."""
    indptr, indices = [0], []
    for r in rows:
        indices += sorted(set(int(x) for x in r))
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32)


def _exact_positions(S, excl_mask=None):
    """pos[i, c] = place of candidate c in np.argsort(-S[i], kind='stable') after removing the excluded candidates."""
    order = np.argsort(-S, axis=1, kind="stable")
    kept = np.ones(S.shape, dtype=bool) if excl_mask is None else ~np.take_along_axis(excl_mask, order, axis=1)
    pos = np.empty(S.shape, dtype=np.int64)
    np.put_along_axis(pos, order, np.cumsum(kept, axis=1) - 1, axis=1)
    return pos


def _rows_of(indptr):
    return np.repeat(np.arange(indptr.size - 1), np.diff(indptr))


@pytest.mark.parametrize("k, C", [(5, 2000), (64, 2500), (33, 4100)])
def test_exact_arithmetic_pins_the_tie_rule_and_the_count(lib, k, C):
    """Small integer entries: every float32 score is exact and ties are everywhere, so every rank is the entry's place in the
    stable argsort of the scores after removing the excluded candidates -- index for index -- and every score is exact."""
    rng = np.random.RandomState(k)
    m = 300
    F = [rng.randint(0, 4, size=(r, k)).astype(float) for r in (m, C, 50)]
    F2 = [rng.randint(-3, 4, size=(r, k)).astype(float) for r in (m, C, 50)]     # a -0 + 0 tie or a sign slip would show
    ctx = _context(lib, F)
    for fac, qf, cf in ((F, U_, V_), (F2, V_, U_)):
        for w in range(3):
            ctx.set_factor(w, fac[w])
        S = fac[qf] @ fac[cf].T
        nq, nc = S.shape
        held = np.zeros(S.shape, dtype=bool)
        held[:, [0, nc - 1, 255, 256 % nc, 70, 71, 72]] = True                    # the ends, a tile edge, three in one 32-block
        held[np.arange(nq)[:, None], rng.randint(0, nc, size=(nq, 4))] = True
        excl = (rng.rand(nq, nc) < 0.1) & ~held
        excl[::9] = False                                                          # rows without a list
        hp, hi = _csr(held)
        for mask in (None, excl):
            rank, score, eligible = ctx.rank(qf, cf, (hp, hi), exclude=None if mask is None else _csr(mask))
            want = _exact_positions(S, mask)[_rows_of(hp), hi]
            assert rank.dtype == np.int32 and (rank == want).all()
            assert score.tobytes() == S[_rows_of(hp), hi].astype(np.float32).tobytes()
            assert (eligible == nc - (0 if mask is None else mask.sum(axis=1))).all()
    ctx.close()


@pytest.mark.parametrize("m, d, p, k", [(300, 5000, 130, 256), (257, 1031, 77, 7)])
def test_ranks_and_top_n_are_one_arithmetic(lib, m, d, p, k):
    """Entries 0, 4 and 9 of a row's top-10 list have ranks exactly 0, 4 and 9 and the list's score bits; no other candidate has a
    rank below 10."""
    F = _factors(m, d, p, k, True, seed=k + 1)
    ctx = _context(lib, F)
    rng = np.random.RandomState(k)
    for qf, cf in ((U_, V_), (V_, U_)):
        nq, nc = F[qf].shape[0], F[cf].shape[0]
        excl = rng.rand(nq, nc) < 0.05
        xl = _csr(excl)
        idx, val = ctx.topk(qf, cf, 10, exclude=xl)
        assert (idx >= 0).all()
        held_rows, others = [], []
        for i in range(nq):
            free = np.setdiff1d(np.flatnonzero(~excl[i]), idx[i])
            extra = rng.choice(free, 3, replace=False)
            others.append(set(extra.tolist()))
            held_rows.append(idx[i, [0, 4, 9]].tolist() + extra.tolist())
        hp, hi = _lists(held_rows)
        rank, score, _ = ctx.rank(qf, cf, (hp, hi), exclude=xl)
        for i in range(nq):
            got = dict(zip(hi[hp[i]:hp[i + 1]].tolist(), zip(rank[hp[i]:hp[i + 1]].tolist(), score[hp[i]:hp[i + 1]])))
            for t in (0, 4, 9):
                r, s = got[int(idx[i, t])]
                assert r == t, "row %d: entry %d of top-n has rank %d" % (i, t, r)
                assert np.float32(s).tobytes() == val[i, t].tobytes()
            assert all(got[c][0] >= 10 for c in others[i])
    ctx.close()


@pytest.mark.parametrize("m, d, p, k, signed", [
    (257, 1031, 77, 7, False),
    (257, 1031, 77, 7, True),
    (70, 333, 129, 40, False),
    (128, 3000, 150, 128, True),
    (300, 5000, 130, 256, True),
    (300, 5000, 130, 256, False),
])
def test_float_parity_on_ragged_shapes_all_four_pairs(lib, m, d, p, k, signed):
    """s = float64 scores of the float32-rounded factors, tau_i = Y.tau: every float32 score is within tau_i of s (yardstick
    docstring), so a candidate with s_c > s_j + 2 tau_i certainly precedes j on the device and one with s_c < s_j - 2 tau_i certainly
    does not: lo <= rank <= hi with lo = #{eligible c: s_c > s_j + 2 tau_i}, hi = #{eligible c != j: s_c >= s_j - 2 tau_i}.
    That the band cannot carry a miscount is asserted from the float64 scores alone: hi - lo <= 16 everywhere (under half a
    32-candidate sub-tile) and, for k <= 40, lo == hi for at least 95 % of the entries."""
    F = _factors(m, d, p, k, signed, seed=k + 5)
    ctx = _context(lib, F)
    tight = total = 0
    for qf, cf in PAIRS:
        nq, nc = F[qf].shape[0], F[cf].shape[0]
        rng = np.random.RandomState(3)
        cols = np.stack([rng.choice(nc, 5, replace=False) for _ in range(nq)])
        held = np.zeros((nq, nc), dtype=bool)
        held[np.arange(nq)[:, None], cols] = True
        excl = (np.random.RandomState(4).rand(nq, nc) < 0.03) & ~held
        hp, hi = _csr(held)
        rank, score, eligible = ctx.rank(qf, cf, (hp, hi), exclude=_csr(excl))
        S = Y.exact_scores(F[qf], F[cf])
        tau = Y.tau(F[qf], F[cf])
        assert (eligible == nc - excl.sum(axis=1)).all()
        ri = _rows_of(hp)
        sj = S[ri, hi]
        assert (np.abs(score.astype(np.float64) - sj) <= tau[ri]).all()
        Se = np.where(excl, -np.inf, S)[ri]                                      # one row of eligible scores per entry
        lo = (Se > (sj + 2 * tau[ri])[:, None]).sum(axis=1)
        hi_ = (Se >= (sj - 2 * tau[ri])[:, None]).sum(axis=1) - 1               # j itself is in the count
        print("pair (%d, %d) k=%d: lo == hi for %.1f %%, widest band %d" % (qf, cf, k, 100.0 * (lo == hi_).mean(), (hi_ - lo).max()))
        assert (hi_ - lo <= 16).all()
        assert ((lo <= rank) & (rank <= hi_)).all(), "pair (%d, %d): %d ranks outside [lo, hi]" % (qf, cf, ((rank < lo) | (rank > hi_)).sum())
        tight += int((lo == hi_).sum())
        total += lo.size
    if k <= 40:
        assert tight >= 0.95 * total
    ctx.close()


def test_lists_and_chunking(lib):
    """Held-out lists of 0, 1, HB, HB + 1 and 3 HB + 5 entries, rows without / with everything-but / edge-touching exclusion lists,
    row subsets with repeats and caller-supplied queries -- on integer factors, so every rank is exact."""
    m, d, k = 150, 1200, 24
    rng = np.random.RandomState(17)
    F = [rng.randint(-3, 4, size=(r, k)).astype(float) for r in (m, d, 40)]
    ctx = _context(lib, F)
    HB = ctx.rank_layout(m, V_, 5 * m)[0]
    assert HB >= 1
    held = rng.rand(m, d) < 0.004
    sizes = {0: 0, 1: 1, 2: HB, 3: HB + 1, 4: 3 * HB + 5, 5: 0, 6: 3 * HB + 5}
    for i, h in sizes.items():
        held[i] = False
        held[i, rng.choice(d, h, replace=False)] = True
    excl = (rng.rand(m, d) < 0.05) & ~held
    excl[::7] = False                                        # rows without a list
    excl[4] = ~held[4]                                       # everything but the held-out entries
    excl[8, [0, d - 1]] = True                               # a list that touches both ends
    held[8, [0, d - 1]] = False
    hl, xl = _csr(held), _csr(excl)
    assert np.diff(hl[0])[:5].tolist() == [0, 1, HB, HB + 1, 3 * HB + 5]
    S = F[0] @ F[1].T
    rank, score, eligible = ctx.rank(U_, V_, hl, exclude=xl)
    want = _exact_positions(S, excl)[_rows_of(hl[0]), hl[1]]
    assert (rank == want).all()
    assert score.tobytes() == S[_rows_of(hl[0]), hl[1]].astype(np.float32).tobytes()
    assert (eligible == d - np.diff(xl[0])).all()
    h4 = 3 * HB + 5
    assert eligible[4] == h4 and sorted(rank[hl[0][4]:hl[0][5]].tolist()) == list(range(h4))
    # without exclusion lists at all
    r0, _, e0 = ctx.rank(U_, V_, hl)
    assert (r0 == _exact_positions(S)[_rows_of(hl[0]), hl[1]]).all() and (e0 == d).all()
    # a row subset with repeats = the gathered full result
    rows = np.array([4, 3, 149, 3, 0, 6, 8, 4])
    sub_h, sub_x = _csr(held[rows]), _csr(excl[rows])
    r_s, s_s, e_s = ctx.rank(U_, V_, sub_h, rows=rows, exclude=sub_x)
    gather = np.concatenate([np.arange(hl[0][i], hl[0][i + 1]) for i in rows])
    assert r_s.tobytes() == rank[gather].tobytes() and s_s.tobytes() == score[gather].tobytes() and e_s.tobytes() == eligible[rows].tobytes()
    # caller-supplied queries = the fitted rows
    r_q, s_q, e_q = ctx.rank(U_, V_, sub_h, exclude=sub_x, queries=ctx.get_factor(U_)[rows])
    assert r_q.tobytes() == r_s.tobytes() and s_q.tobytes() == s_s.tobytes() and e_q.tobytes() == e_s.tobytes()
    QT = np.asfortranarray(ctx.get_factor(U_)[rows])         # strided query storage
    assert ctx.rank(U_, V_, sub_h, exclude=sub_x, queries=QT)[0].tobytes() == r_s.tobytes()
    # no held-out entry at all: nothing to rank, eligible still answered
    none = (np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    r_n, s_n, e_n = ctx.rank(U_, V_, none, exclude=xl)
    assert r_n.size == 0 and s_n.size == 0 and e_n.tobytes() == eligible.tobytes()
    # a NaN query row: its entries have no rank
    Fn = F[0].copy()
    Fn[2, 5] = np.nan
    ctx.set_factor(U_, Fn)
    r_nan, s_nan, _ = ctx.rank(U_, V_, hl, exclude=xl)
    a, b = hl[0][2], hl[0][3]
    assert (r_nan[a:b] == -1).all() and np.isnan(s_nan[a:b]).all()
    assert np.delete(r_nan, np.arange(a, b)).tobytes() == np.delete(rank, np.arange(a, b)).tobytes()
    ctx.close()


def test_determinism_and_candidate_split(lib):
    m, d, p, k = 4096, 200000, 10, 20
    rng = np.random.RandomState(21)
    F = [0.3 * rng.randn(r, k) for r in (m, d, p)]
    ctx = _context(lib, F)
    cols = np.sort(rng.randint(0, d, size=(m, 5)), axis=1)
    hl = _lists(cols)
    a = ctx.rank(U_, V_, hl)
    b = ctx.rank(U_, V_, hl)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert (a[0] >= 0).all() and (a[0] < d).all() and (a[2] == d).all()
    # 32 queries against 200 000 candidates: the candidates are cut across workgroups, however they are cut
    few = np.arange(100, 132)
    sub = (hl[0][100:133] - hl[0][100], hl[1][hl[0][100]:hl[0][132]])
    nnz = int(sub[0][-1])
    f = ctx.rank(U_, V_, sub, rows=few)
    assert f[0].tobytes() == a[0][hl[0][100]:hl[0][132]].tobytes() and f[1].tobytes() == a[1][hl[0][100]:hl[0][132]].tobytes()
    seen = {ctx.rank_layout(32, V_, nnz)[1]}
    assert ctx.rank_layout(32, V_, nnz)[1] != ctx.rank_layout(m, V_, 5 * m)[1]
    for split in (1, 3, 97):
        ctx.set_option("topk_split", split)
        seen.add(ctx.rank_layout(32, V_, nnz)[1])
        g = ctx.rank(U_, V_, sub, rows=few)
        for x, y in zip(f, g):
            assert x.tobytes() == y.tobytes()
    assert len(seen) == 4 and 1 in seen and 3 in seen
    ctx.set_option("topk_split", 0)
    # and the ranks are right: float64 band on the 32 rows
    S = Y.exact_scores(F[0][few], F[1])
    tau = Y.tau(F[0][few], F[1])
    ri = _rows_of(sub[0])
    sj = S[ri, sub[1]]
    lo = (S[ri] > (sj + 2 * tau[ri])[:, None]).sum(axis=1)
    hi = (S[ri] >= (sj - 2 * tau[ri])[:, None]).sum(axis=1) - 1
    assert ((lo <= f[0]) & (f[0] <= hi)).all()
    ctx.close()


def test_rank_leaves_the_context_as_it_was(lib):
    m, d, p, k = 200, 300, 90, 12
    rng = np.random.RandomState(41)
    X, Yd = np.abs(rng.randn(m, d)), np.abs(rng.randn(d, p))
    F = _factors(m, d, p, k, False, seed=42)
    twins = []
    for _ in range(2):
        ctx = _context(lib, F)
        ctx.set_data(0, X)
        ctx.set_data(1, Yd)
        twins.append(ctx)
    a, b = twins
    a.mu_step(0.0, 0.0, 7)
    b.mu_step(0.0, 0.0, 7)
    before = [a.get_factor(w) for w in range(3)]
    opts = a.get_option("topk_split") if hasattr(a, "get_option") else None
    for qf, cf in PAIRS:
        nq, nc = F[qf].shape[0], F[cf].shape[0]
        a.rank(qf, cf, _csr(rng.rand(nq, nc) < 0.05), exclude=_csr(rng.rand(nq, nc) < 0.05))
    a.rank(U_, V_, _lists([[1, 2], [], [299], [0], [5]]), queries=rng.randn(5, k))
    after = [a.get_factor(w) for w in range(3)]
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    assert a.shape == b.shape
    if opts is not None:
        assert a.get_option("topk_split") == opts
    assert a.topk_layout(m, V_, 5) == b.topk_layout(m, V_, 5) and a.rank_layout(m, V_, 50) == b.rank_layout(m, V_, 50)
    a.mu_step(0.0, 0.0, 7)
    b.mu_step(0.0, 0.0, 7)
    for w in range(3):
        assert a.get_factor(w).tobytes() == b.get_factor(w).tobytes()
    a.close()
    b.close()
    # no data at all: problem + factors suffice
    c = _context(lib, F)
    r, s, e = c.rank(Z_, V_, _lists([[7]] * p))
    assert (r >= 0).all() and (r < d).all() and (e == d).all()
    c.close()


def test_refusals_are_einval_with_a_message_and_leave_the_context_usable(lib):
    m, d, p, k = 40, 60, 30, 6
    F = _factors(m, d, p, k, True, seed=51)
    ctx = _context(lib, F)
    L = ctx._lib
    rank = np.empty(400, dtype=np.int32)
    score = np.empty(400, dtype=np.float32)
    elig = np.empty(m + d, dtype=np.int32)
    pr, ps, pe = rank.ctypes.data_as(C.POINTER(C.c_int32)), score.ctypes.data_as(C.POINTER(C.c_float)), elig.ctypes.data_as(C.POINTER(C.c_int32))
    P64, P32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)

    def refused(rc):
        assert rc == 1, "expected CMF_EINVAL, got %d" % rc
        assert len(L.cmf_last_error()) > 10

    def arr(x, dt, pt):
        if x is None:
            return None, None
        a = np.asarray(x, dtype=dt)
        return a, a.ctypes.data_as(pt)

    def raw(query=U_, cand=V_, rows=(0, 1), nq=2, hp=(0, 2, 3), hi=(1, 4, 5), xp=None, xi=None, o_r=pr, o_s=ps, o_e=pe):
        keep = [arr(rows, np.int64, P64), arr(hp, np.int64, P64), arr(hi, np.int32, P32), arr(xp, np.int64, P64), arr(xi, np.int32, P32)]
        return L.cmf_rank(ctx._h, query, cand, keep[0][1], nq, keep[1][1], keep[2][1], keep[3][1], keep[4][1], o_r, o_s, o_e)

    assert raw() == 0 and raw(o_s=None) == 0                                     # the valid call; the score is optional
    for pair in [(U_, U_), (U_, Z_), (Z_, U_), (Z_, Z_), (V_, V_), (3, V_), (U_, -1)]:
        refused(raw(query=pair[0], cand=pair[1]))
    refused(raw(rows=[0, 40]))
    refused(raw(rows=[-1, 0]))
    refused(raw(nq=-1))
    refused(raw(o_r=None))
    refused(raw(o_e=None))
    refused(raw(hp=None))
    refused(raw(hi=None))                                                        # entries without indices
    refused(raw(hi=[4, 1, 5]))                                                   # not sorted
    refused(raw(hi=[4, 4, 5]))                                                   # repeated
    refused(raw(hi=[4, 60, 5]))                                                  # out of range
    refused(raw(hi=[-1, 4, 5]))
    refused(raw(hp=[0, 2, 1]))                                                   # indptr decreases
    refused(raw(hp=[1, 2, 3]))                                                   # indptr[0] != 0
    refused(raw(xp=[0, 2, 3], xi=None))                                          # one pointer of the pair
    refused(raw(xp=[0, 2, 3], xi=[5, 4, 1]))
    refused(raw(xp=[0, 2, 3], xi=[4, 4, 1]))
    refused(raw(xp=[0, 2, 3], xi=[4, 60, 1]))
    refused(raw(xp=[0, 2, 1], xi=[4, 5, 1]))
    refused(raw(xp=[1, 2, 3], xi=[4, 5, 1]))
    Q = np.zeros((2, k))
    pq = Q.ctypes.data_as(C.POINTER(C.c_double))
    hp, hpp = arr([0, 2, 3], np.int64, P64)
    hi, hip = arr([1, 4, 5], np.int32, P32)
    bad, badp = arr([4, 1, 5], np.int32, P32)
    assert L.cmf_rank_queries(ctx._h, pq, k, 1, 2, V_, hpp, hip, None, None, pr, ps, pe) == 0
    refused(L.cmf_rank_queries(ctx._h, pq, k, 1, 2, 3, hpp, hip, None, None, pr, ps, pe))
    refused(L.cmf_rank_queries(ctx._h, None, k, 1, 2, V_, hpp, hip, None, None, pr, ps, pe))
    refused(L.cmf_rank_queries(ctx._h, pq, k, 1, 2, V_, hpp, badp, None, None, pr, ps, pe))
    refused(L.cmf_rank_queries(ctx._h, pq, k, 1, 2, V_, hpp, hip, None, None, None, ps, pe))
    out4 = (C.c_int64 * 4)()
    refused(L.cmf_rank_layout(ctx._h, 0, V_, 5, -1, 0, out4))
    refused(L.cmf_rank_layout(ctx._h, 4, 3, 5, -1, 0, out4))
    refused(L.cmf_rank_layout(ctx._h, 4, V_, -1, -1, 0, out4))
    refused(L.cmf_rank_layout(ctx._h, 4, V_, 5, -1, 0, None))
    with pytest.raises(ValueError, match="rank"):
        ctx.rank(U_, Z_, _lists([[0]] * m))
    fresh = lib.Context(0)
    refused(L.cmf_rank(fresh._h, U_, V_, None, 0, hpp, hip, None, None, pr, ps, pe))   # no problem set
    fresh.close()
    # a valid call after all that
    held = np.zeros((m, d), dtype=bool)
    held[:, [3, 59]] = True
    hl = _csr(held)
    r, s, e = ctx.rank(U_, V_, hl)
    S = Y.exact_scores(F[0], F[1])
    tau = Y.tau(F[0], F[1])
    ri = _rows_of(hl[0])
    sj = S[ri, hl[1]]
    lo = (S[ri] > (sj + 2 * tau[ri])[:, None]).sum(axis=1)
    hi_ = (S[ri] >= (sj - 2 * tau[ri])[:, None]).sum(axis=1) - 1
    assert ((lo <= r) & (r <= hi_)).all() and (e == d).all()
    ctx.close()


def test_estimator_ranks_evaluate_and_rank_products(lib):
    import pycmf_amd
    from pycmf_amd import CMF
    rng = np.random.RandomState(61)
    m, d, p, k = 90, 70, 33, 6
    X = np.abs(rng.randn(m, d)) * (rng.rand(m, d) < 0.4)
    Yd = np.abs(rng.randn(d, p))
    test = (X != 0) & (rng.rand(m, d) < 0.25)
    X_train, X_test = sp.csr_matrix(np.where(test, 0.0, X)), sp.csr_matrix(np.where(test, X, 0.0))
    model = CMF(n_components=k, solver="mu", max_iter=30, random_state=0).fit(X_train.toarray(), Yd)
    indptr, indices, rank, eligible = model.ranks(X_test, exclude=X_train)
    assert indptr[-1] == test.sum() == rank.size and (eligible == d - np.diff(X_train.indptr)).all()
    got = model.evaluate(X_test, n=(5, 10), exclude=X_train)
    assert got == pycmf_amd.ranking_metrics(indptr, rank, eligible, n=(5, 10))
    # recall@10 recomputed from top_n on the same model: the two share their arithmetic, so exactly
    idx, _ = model.top_n(n=10, exclude=X_train)
    per_row = [np.isin(indices[indptr[i]:indptr[i + 1]], idx[i]).sum() / (indptr[i + 1] - indptr[i]) for i in range(m) if indptr[i + 1] > indptr[i]]
    assert got["rows_evaluated"] == len(per_row) and got["recall@10"] == float(np.mean(per_row))
    assert 0.0 < got["auc"] <= 1.0 and 0.0 <= got["ndcg@10"] <= 1.0
    # rank_products on the same factors
    ip2, ix2, rk2, el2 = pycmf_amd.rank_products(model.x_weights, model.components, X_test, exclude=X_train)
    assert ip2.tobytes() == indptr.tobytes() and ix2.tobytes() == indices.tobytes() and rk2.tobytes() == rank.tobytes() and el2.tobytes() == eligible.tobytes()
    # the other axis, the other relation, a row subset, queries from transform
    ipT, ixT, rkT, elT = model.ranks(X_test, axis=1, exclude=X_train)
    ip3, ix3, rk3, el3 = pycmf_amd.rank_products(model.components, model.x_weights, X_test.T, exclude=X_train.T)
    assert ipT.tobytes() == ip3.tobytes() and ixT.tobytes() == ix3.tobytes() and rkT.tobytes() == rk3.tobytes() and elT.tobytes() == el3.tobytes()
    rows = np.array([3, 80, 3])
    ipr, ixr, rkr, elr = model.ranks(X_test, exclude=X_train, rows=rows)
    want = np.concatenate([rank[indptr[i]:indptr[i + 1]] for i in rows])
    assert rkr.tobytes() == want.tobytes() and elr.tobytes() == eligible[rows].tobytes()
    ytest = sp.csr_matrix((rng.rand(d, p) < 0.1).astype(float))
    ipy, ixy, rky, ely = model.ranks(ytest, relation="y")
    assert rky.size == ytest.nnz and (rky >= 0).all() and (rky < p).all() and (ely == p).all()
    Unew = model.transform(np.abs(rng.randn(11, d)), None)[0]
    hq = sp.csr_matrix((rng.rand(11, d) < 0.1).astype(float))
    ipq, ixq, rkq, elq = model.ranks(hq, queries=Unew)
    ip4, ix4, rk4, el4 = pycmf_amd.rank_products(Unew, model.components, hq)
    assert rkq.tobytes() == rk4.tobytes() and ixq.tobytes() == ix4.tobytes()
