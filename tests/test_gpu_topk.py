"""Top-n prediction on the device (cmf_topk / cmf_topk_queries, CMF.top_n, top_n_products) against NumPy float64 on the
float32-rounded factors.  The tolerance is derived in topk_yardstick.py; it is checked on every row of every case."""
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


def _factors(m, d, p, k, signed, seed):
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


@pytest.mark.parametrize("m, d, p, k, n, signed", [
    (257, 1031, 77, 7, 5, False),
    (257, 1031, 77, 7, 1, True),
    (300, 5000, 130, 256, 10, True),
    (300, 5000, 130, 256, 10, False),
    (128, 3000, 150, 128, 100, True),
    (70, 333, 129, 40, 128, False),
])
def test_four_pairs_both_links_on_ragged_shapes(lib, m, d, p, k, n, signed):
    F = _factors(m, d, p, k, signed, seed=k + n)
    ctx = _context(lib, F)
    for qf, cf in PAIRS:
        if n > F[cf].shape[0]:
            continue
        for link in ("linear", "logit"):
            idx, val = ctx.topk(qf, cf, n, link=link)
            worst = Y.check_top_n(idx, val, F[qf], F[cf], n, link, label="pair (%d, %d) %s" % (qf, cf, link))
            print("pair (%d, %d) %s k=%d n=%d: max |r_t - s_t| / tau = %.4f" % (qf, cf, link, k, n, worst))
    ctx.close()


@pytest.mark.parametrize("k, C", [(5, 2000), (64, 2500), (33, 4100)])
def test_exact_arithmetic_pins_the_tie_rule_and_the_k_order(lib, k, C):
    """Small integer entries: every float32 score is exact and ties are everywhere, so the answer is unique under the stated
    order -- larger score first, equal scores by smaller index -- and must be reproduced index for index, bit for bit."""
    rng = np.random.RandomState(k)
    m, n = 300, 10
    F = [rng.randint(0, 4, size=(r, k)).astype(float) for r in (m, C, 50)]
    ctx = _context(lib, F)
    S = F[0] @ F[1].T
    want = np.argsort(-S, axis=1, kind="stable")[:, :n]
    idx, val = ctx.topk(U_, V_, n)
    assert (idx == want).all()
    assert val.tobytes() == np.take_along_axis(S, want, axis=1).astype(np.float32).tobytes()
    # signed integers (a -0 + 0 tie or a sign slip would show) and the other orientation
    F2 = [rng.randint(-3, 4, size=(r, k)).astype(float) for r in (m, C, 50)]
    for w in range(3):
        ctx.set_factor(w, F2[w])
    S = F2[1] @ F2[0].T
    want = np.argsort(-S, axis=1, kind="stable")[:, :n]
    idx, val = ctx.topk(V_, U_, n)
    assert (idx == want).all()
    assert val.tobytes() == np.take_along_axis(S, want, axis=1).astype(np.float32).tobytes()
    ctx.close()


def test_exclusion_lists(lib):
    m, d, p, k, n = 150, 1200, 40, 24, 10
    F = _factors(m, d, p, k, True, seed=11)
    rng = np.random.RandomState(12)
    mask = rng.rand(m, d) < 0.05
    mask[::7] = False                                        # rows without a list
    S = Y.exact_scores(F[0], F[1])
    top = np.argsort(-S, axis=1, kind="stable")[:, :n]
    for i in range(3, m, 5):                                 # rows that exclude their entire float64 top-n
        mask[i, top[i]] = True
    mask[10] = True
    mask[10, rng.choice(d, n - 3, replace=False)] = False    # all but n - 3 candidates: three empty places
    mask[20] = True                                          # nothing left at all
    csr = sp.csr_matrix(mask.astype(float))
    excl = (csr.indptr.astype(np.int64), csr.indices.astype(np.int32))
    ctx = _context(lib, F)
    for link in ("linear", "logit"):
        idx, val = ctx.topk(U_, V_, n, link=link, exclude=excl)
        Y.check_top_n(idx, val, F[0], F[1], n, link, excl, label="exclusion " + link)
        assert (idx[10, n - 3:] == -1).all() and (idx[10, :n - 3] >= 0).all()
        assert (idx[20] == -1).all() and np.isneginf(val[20]).all()
        assert not mask[np.repeat(np.arange(m), n)[idx.ravel() >= 0], idx.ravel()[idx.ravel() >= 0]].any()
    # a row subset with its own lists
    rows = np.array([20, 3, 10, 3, 149, 0])
    sub = csr[rows]
    idx, val = ctx.topk(U_, V_, n, rows=rows, exclude=(sub.indptr.astype(np.int64), sub.indices.astype(np.int32)))
    full, fval = ctx.topk(U_, V_, n, exclude=excl)
    assert idx.tobytes() == full[rows].tobytes() and val.tobytes() == fval[rows].tobytes()
    ctx.close()


def test_determinism_subsets_and_candidate_split(lib):
    m, d, p, k, n = 4096, 200000, 10, 20, 10
    rng = np.random.RandomState(21)
    F = [0.3 * rng.randn(r, k) for r in (m, d, p)]
    ctx = _context(lib, F)
    a_idx, a_val = ctx.topk(U_, V_, n)
    b_idx, b_val = ctx.topk(U_, V_, n)
    assert a_idx.tobytes() == b_idx.tobytes() and a_val.tobytes() == b_val.tobytes()
    rows = rng.permutation(m)[:200]
    rows[17] = rows[3]                                       # rows may repeat
    s_idx, s_val = ctx.topk(U_, V_, n, rows=rows)
    assert s_idx.tobytes() == a_idx[rows].tobytes() and s_val.tobytes() == a_val[rows].tobytes()
    # 32 queries against 200 000 candidates: the candidates are cut across workgroups and the lists merged
    assert ctx.topk_layout(32, V_, n)[1] > 1 and ctx.topk_layout(32, V_, n)[1] != ctx.topk_layout(m, V_, n)[1]
    few = np.arange(100, 132)
    f_idx, f_val = ctx.topk(U_, V_, n, rows=few)
    assert f_idx.tobytes() == a_idx[few].tobytes() and f_val.tobytes() == a_val[few].tobytes()
    # ... and however they are cut
    seen = {ctx.topk_layout(32, V_, n)[1]}
    for split in (1, 3, 97):
        ctx.set_option("topk_split", split)
        seen.add(ctx.topk_layout(32, V_, n)[1])
        g_idx, g_val = ctx.topk(U_, V_, n, rows=few)
        assert g_idx.tobytes() == f_idx.tobytes() and g_val.tobytes() == f_val.tobytes()
    assert len(seen) == 4 and 1 in seen and 3 in seen
    ctx.set_option("topk_split", 0)
    Y.check_top_n(f_idx, f_val, F[0][few], F[1], n, label="32 x 200000")
    ctx.close()


def test_caller_supplied_queries(lib):
    m, d, p, k, n = 500, 900, 60, 48, 10
    F = _factors(m, d, p, k, False, seed=31)
    ctx = _context(lib, F)
    rows = np.array([5, 499, 0, 77, 77, 128])
    for link in ("linear", "logit"):
        a_idx, a_val = ctx.topk(U_, V_, n, link=link, rows=rows)
        q_idx, q_val = ctx.topk(U_, V_, n, link=link, queries=ctx.get_factor(U_)[rows])
        assert a_idx.tobytes() == q_idx.tobytes() and a_val.tobytes() == q_val.tobytes()
    # strided (transposed) query storage is honoured
    QT = np.asfortranarray(ctx.get_factor(U_)[rows])
    q2_idx, _ = ctx.topk(U_, V_, n, queries=QT)
    assert q2_idx.tobytes() == ctx.topk(U_, V_, n, rows=rows)[0].tobytes()
    # the k unit vectors: the top rows of a factor's COLUMNS (what print_topic_terms lists), any candidate factor
    idx, val = ctx.topk(U_, U_, 10, queries=np.eye(k))
    U32 = F[0].astype(np.float32)
    checked = 0
    for t in range(k):
        order = np.argsort(U32[:, t])
        top11 = U32[order[-11:], t]
        if len(set(top11.tolist())) == 11:
            assert idx[t].tolist() == order[-10:][::-1].tolist()
            assert val[t].tobytes() == U32[order[-10:][::-1], t].tobytes()
            checked += 1
    assert checked >= k // 2
    ctx.close()


def test_topk_leaves_the_context_as_it_was(lib):
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
    for qf, cf in PAIRS:
        a.topk(qf, cf, 7, link="logit")
    a.topk(U_, V_, 3, queries=rng.randn(5, k))
    after = [a.get_factor(w) for w in range(3)]
    for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    a.mu_step(0.0, 0.0, 7)
    b.mu_step(0.0, 0.0, 7)
    for w in range(3):
        assert a.get_factor(w).tobytes() == b.get_factor(w).tobytes()
    a.close()
    b.close()
    # no data at all: problem + factors suffice
    c = _context(lib, F)
    idx, val = c.topk(Z_, V_, 4)
    Y.check_top_n(idx, val, F[2], F[1], 4, label="no data")
    c.close()


def test_refusals_are_einval_with_a_message_and_leave_the_context_usable(lib):
    m, d, p, k = 40, 60, 30, 6
    F = _factors(m, d, p, k, True, seed=51)
    ctx = _context(lib, F)
    L = ctx._lib
    n = 3
    idx = np.empty((m, 200), dtype=np.int32)
    val = np.empty((m, 200), dtype=np.float32)
    pi, pv = idx.ctypes.data_as(C.POINTER(C.c_int32)), val.ctypes.data_as(C.POINTER(C.c_float))

    def refused(rc):
        assert rc == 1, "expected CMF_EINVAL, got %d" % rc                 # CMF_EINVAL
        assert len(L.cmf_last_error()) > 10

    def raw(query=U_, cand=V_, link=0, rows=None, nq=0, n_=n, xp=None, xi=None, oi=pi, ov=pv):
        r = None if rows is None else np.asarray(rows, dtype=np.int64)
        a = None if xp is None else np.asarray(xp, dtype=np.int64)
        b = None if xi is None else np.asarray(xi, dtype=np.int32)
        return L.cmf_topk(ctx._h, query, cand, link, None if r is None else r.ctypes.data_as(C.POINTER(C.c_int64)), nq, n_,
                          None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64)),
                          None if b is None else b.ctypes.data_as(C.POINTER(C.c_int32)), oi, ov)

    for pair in [(U_, U_), (U_, Z_), (Z_, U_), (Z_, Z_), (V_, V_), (3, V_), (U_, -1)]:
        refused(raw(query=pair[0], cand=pair[1]))
    refused(raw(n_=0))
    refused(raw(n_=129))
    refused(raw(n_=61))                                                    # above the 60 candidates
    refused(raw(cand=V_, query=Z_, n_=61))
    refused(raw(link=2))
    refused(raw(rows=[0, 40], nq=2))
    refused(raw(rows=[-1], nq=1))
    refused(raw(rows=[0], nq=-1))
    refused(raw(oi=None))
    refused(raw(rows=[0, 1], nq=2, xp=[0, 2, 3], xi=None))                 # one pointer of the pair
    refused(raw(rows=[0, 1], nq=2, xp=[0, 2, 3], xi=[5, 4, 1]))            # not sorted
    refused(raw(rows=[0, 1], nq=2, xp=[0, 2, 3], xi=[4, 4, 1]))            # repeated
    refused(raw(rows=[0, 1], nq=2, xp=[0, 2, 3], xi=[4, 60, 1]))           # out of range
    refused(raw(rows=[0, 1], nq=2, xp=[0, 2, 1], xi=[4, 5, 1]))            # indptr decreases
    refused(raw(rows=[0, 1], nq=2, xp=[1, 2, 3], xi=[4, 5, 1]))            # indptr[0] != 0
    Q = np.zeros((2, k))
    pq = Q.ctypes.data_as(C.POINTER(C.c_double))
    refused(L.cmf_topk_queries(ctx._h, pq, k, 1, 2, 3, 0, n, None, None, pi, pv))
    refused(L.cmf_topk_queries(ctx._h, pq, k, 1, 2, V_, 0, 0, None, None, pi, pv))
    refused(L.cmf_topk_queries(ctx._h, None, k, 1, 2, V_, 0, n, None, None, pi, pv))
    with pytest.raises(ValueError, match="top-n"):
        ctx.topk(U_, Z_, n)
    fresh = lib.Context(0)
    refused(L.cmf_topk(fresh._h, U_, V_, 0, None, 0, n, None, None, pi, pv))   # no problem set
    fresh.close()
    got, gv = ctx.topk(U_, V_, n)
    Y.check_top_n(got, gv, F[0], F[1], n, label="after the refusals")
    ctx.close()


def test_estimator_top_n_and_top_n_products(lib):
    import pycmf_amd
    from pycmf_amd import CMF
    rng = np.random.RandomState(61)
    m, d, p, k = 90, 70, 33, 6
    X = np.abs(rng.randn(m, d)) * (rng.rand(m, d) < 0.3)
    Yd = np.abs(rng.randn(d, p))
    model = CMF(n_components=k, solver="mu", max_iter=30, random_state=0).fit(X, Yd)
    U, V, Z = model.x_weights, model.components, model.y_weights
    for relation, axis, A, B in (("x", 0, U, V), ("x", 1, V, U), ("y", 0, V, Z), ("y", 1, Z, V)):
        idx, val = model.top_n(relation=relation, axis=axis, n=5)
        Y.check_top_n(idx, val, A, B, 5, "linear", label="%s axis %d" % (relation, axis))
    rows = np.array([3, 80, 3])
    idx, val = model.top_n(rows=rows, n=4)
    Y.check_top_n(idx, val, U[rows], V, 4, "linear", label="rows")
    Xs = sp.csr_matrix(X)
    idx, val = model.top_n(n=5, exclude=Xs)
    assert not (X[np.repeat(np.arange(m), 5), idx.ravel()] != 0).any()
    Y.check_top_n(idx, val, U, V, 5, "linear", (Xs.indptr.astype(np.int64), Xs.indices.astype(np.int32)), label="exclude=X")
    idx, val = model.top_n(axis=1, n=5, exclude=Xs)
    XT = sp.csr_matrix(Xs.T)
    XT.sort_indices()
    Y.check_top_n(idx, val, V, U, 5, "linear", (XT.indptr.astype(np.int64), XT.indices.astype(np.int32)), label="exclude=X, axis 1")
    Xnew = np.abs(rng.randn(11, d))
    Unew = model.transform(Xnew, None)[0]
    idx, val = model.top_n(queries=Unew, n=5)
    Y.check_top_n(idx, val, Unew, V, 5, "linear", label="queries from transform")
    # a logit side: the estimator's own link is applied to the values
    Yl = 1.0 / (1.0 + np.exp(-rng.randn(d, p)))
    lm = CMF(n_components=k, solver="newton", max_iter=3, random_state=0, y_link="logit", U_non_negative=False,
             V_non_negative=False, Z_non_negative=False).fit(X, Yl)
    idx, val = lm.top_n(relation="y", axis=1, n=6)
    Y.check_top_n(idx, val, lm.y_weights, lm.components, 6, "logit", label="logit y")
    assert (val > 0).all() and (val < 1).all()
    # plain arrays
    A, B = rng.randn(37, 9), rng.randn(410, 9)
    idx, val = pycmf_amd.top_n_products(A, B, 8, link="logit")
    Y.check_top_n(idx, val, A, B, 8, "logit", label="top_n_products")
    msk = sp.random(37, 410, density=0.2, random_state=3, format="csr")
    idx, val = pycmf_amd.top_n_products(A, B, 8, exclude=msk)
    msk.sort_indices()
    Y.check_top_n(idx, val, A, B, 8, "linear", (msk.indptr.astype(np.int64), msk.indices.astype(np.int32)), label="top_n_products exclude")


def test_full_size_all_rows_in_one_call(lib):
    """m = d = 65536, k = 256, n = 10: the product would be 17 GB; the call's scratch is n * 8 * (S + 1) bytes per query."""
    m = d = 65536
    k, n = 256, 10
    ctx = lib.Context(0)
    ctx.set_problem(m, d, 256, k)
    scale = (0.7979 / k) ** 0.5
    ctx.fill_factor_synthetic(U_, 101, 0, scale)
    ctx.fill_factor_synthetic(V_, 102, 0, scale)
    qb, S, chunk, scratch = ctx.topk_layout(m, V_, n)
    assert chunk == m and scratch == m * n * 8 * (S + 1)
    assert scratch < 0.005 * 4.0 * m * d                     # a small fraction of a percent of the dense product
    ctx.kernel_timing(True)
    idx, val = ctx.topk(U_, V_, n)
    ms, launches, flops = ctx.kernel_time("topk")
    ctx.kernel_timing(False)
    assert launches == 1 and flops == 2.0 * m * d * k
    print("full size top-%d: %.2f ms kernel time, %.1f TF/s algorithmic, split %d, scratch %.1f MB" % (n, ms, flops / ms * 1e-9, S, scratch / 2 ** 20))
    U, V = ctx.get_factor(U_), ctx.get_factor(V_)
    ctx.close()
    rows = np.random.RandomState(71).choice(m, 512, replace=False)
    worst = Y.check_top_n(idx[rows], val[rows], U[rows], V, n, label="full size")
    print("full size: max |r_t - s_t| / tau over 512 sampled rows = %.4f" % worst)
    assert (idx >= 0).all() and (idx < d).all()
