"""The native CSR kernels one product at a time against float64 (sparse_yardstick.py): the row-gather SpMM at every operand width, the
column-blocked SpMM with split rows and with more than one stretch, the SDDMM of the error metric at every k_pad under both links, a
split row written as a Newton update, and the per-row sweeps on native sides above k_pad 32.  Signed inputs; an exact family
compared with ==, a random family held to (L + 16) 2^-24 sum|terms| per element.  Every test prints its worst |err| / bound."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparse_yardstick as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _context(lib, shape, X=None, Y=None, F=None, **options):
    """Options first, then the problem, then the data: the layout is built when the data is set."""
    ctx = lib.Context(0)
    ctx.set_option("sparse_mode", 2)
    for name, value in options.items():
        ctx.set_option(name, value)
    ctx.set_problem(*shape)
    for which, A in enumerate((X, Y)):
        if A is not None:
            ctx.set_data(which, A)
            assert ctx.data_layout(which) == (False, True)
    for w, f in enumerate(F or ()):
        ctx.set_factor(w, f)
    return ctx


def _check_product(got, A, B, trans, family, what):
    """== in the exact family, inside product_bound in the random one; returns |err| / bound."""
    assert got.shape == ((A.shape[1] if trans else A.shape[0]), B.shape[1]), what
    if family == "exact":
        assert (got == S.product(A, B, trans)).all(), what
        return 0.0
    r = S.worst_ratio(got, A, B, trans)
    assert r <= 1.0, (what, r)
    return r


# ------------------------------------------------------------------ a. the row kernel, every width
@pytest.mark.parametrize("family", ["exact", "random"])
def test_row_kernel_at_every_width(lib, family):
    """spmm_csr_kernel<8|16|32|64, 1> and <64, 2|3|4> (operand widths padded to 32 .. 1024), A B and A^T B of X (77 x 300: rows
    of 0, 1, 3, 4, 5, 7, 8, 33, 70 and 300 entries, seven empty rows at the end) through cmf_data_matmul_f64 on a context of k = 40
    with the blocked form off; Y (300 x 45, an empty column, empty rows at the end) at one width."""
    X, Y = S.row_case(family)
    ctx = _context(lib, S.ROW_SHAPE + (40,), X, Y, spmm_blocked=0)
    assert ctx.sparse_layout(0) == ((0, 0, 0, 0), (0, 0, 0, 0))
    worst = 0.0
    for width in S.ROW_WIDTHS:
        for trans in (False, True):
            B = S.row_operand(0, trans, width, family)
            worst = max(worst, _check_product(ctx.data_matmul(0, trans, B), X, B, trans, family, "X, width %d, trans %d" % (width, trans)))
    for trans in (False, True):
        B = S.row_operand(1, trans, 40, family)
        worst = max(worst, _check_product(ctx.data_matmul(1, trans, B), Y, B, trans, family, "Y, trans %d" % trans))
    ctx.close()
    print("row kernel, %s family, widths %s: worst |err| / bound %.4f" % (family, S.ROW_WIDTHS, worst))


@pytest.mark.parametrize("blocked", [0, 2])
def test_a_matrix_without_entries_gives_exact_zeros(lib, blocked):
    m, d, p = S.ROW_SHAPE
    ctx = _context(lib, (m, d, p, 40), sp.csr_matrix((m, d)), spmm_blocked=blocked, spmm_block_cols=64)
    assert (ctx.sparse_layout(0)[0][0] > 0) == (blocked == 2)
    for width in (40, 300):                                           # 40: the blocked form where there is one
        for trans in (False, True):
            got = ctx.data_matmul(0, trans, S.row_operand(0, trans, width, "random"))
            assert got.shape == ((d if trans else m), width) and (got == 0).all() and not np.signbit(got).any()
    ctx.close()
    print("nnz = 0, spmm_blocked = %d: worst |err| / bound 0 (exact zeros)" % blocked)


def test_an_operand_wider_than_1024_is_refused_and_the_context_lives_on(lib):
    X, Y = S.row_case("exact")
    ctx = _context(lib, S.ROW_SHAPE + (40,), X, Y, spmm_blocked=0)
    with pytest.raises(NotImplementedError, match=r"operand widths 32\.\.1024 \(got 1280\)"):
        ctx.data_matmul(0, False, S.row_operand(0, False, 1100, "exact"))
    B = S.row_operand(0, True, 1000, "exact")
    _check_product(ctx.data_matmul(0, True, B), X, B, True, "exact", "after the refusal")
    ctx.close()
    print("1100 columns refused, 1000 exact afterwards: worst |err| / bound 0")


# ------------------------------------------------------------------ b. the blocked kernel
@pytest.mark.parametrize("stretch", [0, 1])
@pytest.mark.parametrize("k", [40, 100, 200])
def test_blocked_kernel_with_split_rows_and_stretches(lib, k, stretch):
    """spmm_blocked_kernel<1|2|4> + spmm_partial_sum_kernel through cmf_data_matmul_f64 with exactly k operand columns (padded to
    k_pad: the blocked form).  M is 100 x 3072 in 48 column blocks of 64 (one of them empty), rows of 0 .. 129 entries and of 1280
    (whole), 1281 (two pieces), 2049 and 3000 (three pieces each).  "spmm_stretch" = 1 puts one column block in a stretch:
    48 stretches with a rendezvous in front of each, against one stretch by default.  M as X, and M^T as X (the hot rows in the
    transposed image)."""
    rows, cols = S.BLOCK_SHAPE
    worst = 0.0
    for family in ("exact", "random"):
        M = S.blocked_case(family)
        Mt = M.T.tocsr()
        lengths = np.diff(M.indptr)
        opts = dict(spmm_blocked=2, spmm_block_cols=S.BLOCK_COLS, spmm_stretch=stretch)
        ctx = _context(lib, (rows, cols, 1, k), M, **opts)
        a, at = ctx.sparse_layout(0)
        assert a[0] > 0 and at[0] > 0, (a, at)
        nsplit, npieces, share = S.split_layout(lengths, a[3])
        assert share == 1024 and (nsplit, npieces) == (3, 8) and a[1:3] == (nsplit, npieces), (a, share)
        assert at[1:3] == S.split_layout(np.diff(Mt.indptr), at[3])[:2] == (0, 0), at
        tctx = _context(lib, (cols, rows, 1, k), Mt, **opts)
        ta, tat = tctx.sparse_layout(0)
        assert ta[0] > 0 and ta[1:3] == (0, 0) and tat[0] > 0 and tat[1:3] == S.split_layout(lengths, tat[3])[:2] == (3, 8), (ta, tat)
        others = {}
        if family == "exact":
            others["row kernel"] = _context(lib, (rows, cols, 1, k), M, spmm_blocked=0)
            others["no pieces"] = _context(lib, (rows, cols, 1, k), M, spmm_split=0, **opts)
            assert others["row kernel"].sparse_layout(0)[0][0] == 0
            lay = others["no pieces"].sparse_layout(0)
            assert lay[0][0] > 0 and lay[0][1:3] == (0, 0) and lay[1][1:3] == (0, 0), lay
        for trans in (False, True):
            B = S.blocked_operand(rows if trans else cols, k, family)
            what = "k %d stretch %d %s trans %d" % (k, stretch, family, trans)
            got = ctx.data_matmul(0, trans, B)
            worst = max(worst, _check_product(got, M, B, trans, family, what))
            assert ctx.data_matmul(0, trans, B).tobytes() == got.tobytes(), what               # a pure function of its inputs
            tgot = tctx.data_matmul(0, not trans, B)                                           # the same product from the other binding
            worst = max(worst, _check_product(tgot, M, B, trans, family, what + ", M^T bound"))
            assert tctx.data_matmul(0, not trans, B).tobytes() == tgot.tobytes(), what
            for name, o in others.items():
                assert (o.data_matmul(0, trans, B) == got).all(), (what, name)
            # any other operand width on the blocked context: the one-wave-per-row kernel
            Bw = S.blocked_operand(rows if trans else cols, 300, family)
            worst = max(worst, _check_product(ctx.data_matmul(0, trans, Bw), M, Bw, trans, family, what + ", width 300"))
        for c in [ctx, tctx] + list(others.values()):
            c.close()
    print("blocked kernel, k %d, spmm_stretch %d: worst |err| / bound %.4f" % (k, stretch, worst))


# ------------------------------------------------------------------ c. the SDDMM
@pytest.mark.parametrize("k", S.SDDMM_KS)
def test_sddmm_linear(lib, k):
    """sddmm_cross_kernel<8|16|32|64, 1> and <64, 2|3|4>, linear branch, through cmf_residual_sq on native sides with signed
    factors set and no step taken: == float64 in the exact family, inside residual_bound in the random one.  Both sides: the
    Y side (170 x 40) runs the same kernel over V and Z."""
    worst = 0.0
    for family in ("exact", "random"):
        X, Y, F = S.sddmm_case(k, family)
        ctx = _context(lib, S.SDDMM_SHAPE + (k,), X, Y, F)
        got = ctx.residual_sq("linear", "linear")
        assert ctx.data_layout(0) == (False, True) and ctx.data_layout(1) == (False, True)
        ctx.close()
        for side, (A, L, R) in enumerate(((X, F[0], F[1]), (Y, F[1], F[2]))):
            ref = S.residual_sq(A, L, R)
            if family == "exact":
                assert got[side] == ref, (k, side, got[side], ref)
                continue
            bound = S.residual_bound(A, L, R)
            ratio = abs(got[side] - ref) / bound
            print("k %d side %d: r2 %.9g, float64 %.9g, |err| / bound %.4f" % (k, side, got[side], ref, ratio))
            worst = max(worst, ratio)
            assert abs(got[side] - ref) <= bound, (k, side)
    print("SDDMM linear, k %d: exact family ==, random family worst |err| / bound %.4f" % (k, worst))


@pytest.mark.parametrize("k", S.SDDMM_KS)
def test_sddmm_logit(lib, k):
    """The logit branch (a cross-lane reduction of the dot product inside the loop over a row's entries, rows of different
    lengths in one wave below k_pad 256): targets in (0, 1), signed factors, the root of the squared residual within the
    project's parity of 1e-4 of float64."""
    X, Y, F = S.sddmm_case(k, "random", "logit")
    ctx = _context(lib, S.SDDMM_SHAPE + (k,), X, Y, F)
    got = ctx.residual_sq("logit", "logit")
    assert ctx.data_layout(0) == (False, True) and ctx.data_layout(1) == (False, True)
    ctx.close()
    worst = 0.0
    for side, (A, L, R) in enumerate(((X, F[0], F[1]), (Y, F[1], F[2]))):
        ref = np.sqrt(S.residual_sq(A, L, R, "logit"))
        dist = abs(np.sqrt(got[side]) - ref) / ref
        numpy32 = abs(np.sqrt(S.residual_sq_logit_f32(A, L, R)) - ref) / ref
        print("k %d side %d: relative distance of the root %.3e (float32 NumPy evaluation of the expansion: %.3e)" % (k, side, dist, numpy32))
        worst = max(worst, dist / 1e-4)
        np.testing.assert_allclose(np.sqrt(got[side]), ref, rtol=1e-4)
    print("SDDMM logit, k %d: worst |err| / bound %.4f" % (k, worst))


# ------------------------------------------------------------------ d. split rows written as a Newton update
def _split_update_case(k, nn):
    m, d, p = 300, 1536, 60
    rng = np.random.RandomState(71 + k)
    xlen = rng.randint(10, 60, m)
    xlen[[7, 150, 299]] = (1300, 1400, 1536)
    ytlen = rng.randint(40, 120, p)
    ytlen[[0, 33, 59]] = (1301, 1450, 1536)
    X = S.matrix(xlen, d, "exact", rng)
    Y = S.matrix(ytlen, d, "exact", rng).T.tocsr()
    F = [0.3 * np.abs(rng.randn(n, k)) for n in (m, d, p)]
    if not nn:
        F = [f - f.mean() for f in F]
    return X, Y, F, xlen, ytlen


@pytest.mark.parametrize("nn", [False, True])
@pytest.mark.parametrize("k", [100, 256])
def test_split_rows_written_as_a_newton_update(lib, k, nn):
    """The configuration of test_blocked_spmm_writes_the_newton_update_itself (l1 = 0, linear links: the SpMM's epilogue writes the
    factor) with rows that are cut into pieces, so that the epilogue which zeroes the columns >= k and clamps is that of
    spmm_partial_sum_kernel: three rows of X (U sweep) and three columns of Y (rows of Y^T, Z sweep) of 1300 .. 1536 entries.
    k = 100: kvalid < k_pad; k = 256: kvalid = k_pad."""
    from oracle import cmf_oracle as O
    X, Y, F, xlen, ytlen = _split_update_case(k, nn)
    shape = (300, 1536, 60, k)
    got, counts = {}, {}
    for name, opts in (("blocked", dict(spmm_blocked=2)), ("row kernel", dict(spmm_blocked=0)), ("no pieces", dict(spmm_blocked=2, spmm_split=0))):
        ctx = _context(lib, shape, X, Y, F, spmm_block_cols=64, **opts)
        (xa, xat), (ya, yat) = ctx.sparse_layout(0), ctx.sparse_layout(1)
        if name == "blocked":
            assert xa[0] > 0 and xa[1:3] == S.split_layout(xlen, xa[3])[:2] == (3, 6), xa
            assert yat[0] > 0 and yat[1:3] == S.split_layout(ytlen, yat[3])[:2] == (3, 6), yat
            assert xat[1] == 0 and ya[1] == 0
        else:
            assert xa[1] == 0 and yat[1] == 0 and (xa[0] > 0) == (name == "no pieces")
        ctx.kernel_timing(1)
        for _ in range(2):
            ctx.newton_step(0.4, 0.0, 0.6, "linear", "linear", 7 if nn else 0, 7, 0.2, 1.0)
        counts[name] = (ctx.kernel_time("spmm")[1], ctx.kernel_time("elementwise")[1])
        ctx.kernel_timing(False)
        got[name] = [ctx.get_factor(w) for w in range(3)]
        assert ctx.data_layout(0) == (False, True) and ctx.data_layout(1) == (False, True)
        ctx.close()
    # the route: the same four products per iteration everywhere, and the U and Z sweeps of the blocked images without the
    # combine pass that follows the row kernel's product (one elementwise launch per sweep and iteration)
    print("k %d nn %s: (spmm, elementwise) launches %s" % (k, nn, counts))
    assert counts["blocked"][0] == counts["row kernel"][0] == counts["no pieces"][0] == 8
    assert counts["blocked"][1] == counts["no pieces"][1] == counts["row kernel"][1] - 4
    U, V, Z = (f.copy() for f in F)
    for _ in range(2):
        O.newton_update_step(X, Y, U, V, Z, 0.4, 0.0, 0.6, "linear", "linear", nn, nn, nn, 1.0, 0.2)
    worst = 0.0
    for w, o in enumerate((U, V, Z)):
        a = got["blocked"][w]
        for other in ("row kernel", "no pieces"):
            b = got[other][w]
            worst = max(worst, np.abs(a - b).max() / (2e-5 * np.abs(b).max()))
            np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * np.abs(b).max())
        worst = max(worst, np.abs(a - o).max() / (5e-5 * np.abs(o).max()))
        np.testing.assert_allclose(a, o, rtol=0, atol=5e-5 * np.abs(o).max())
        if nn:
            assert (a >= 0).all() and (a == 0).any()
        else:
            assert (a < 0).any()
    # the split rows themselves, not only the largest element of the factor
    for w, hot in ((0, [7, 150, 299]), (2, [0, 33, 59])):
        o = (U, V, Z)[w]
        assert np.abs(got["blocked"][w][hot] - o[hot]).max() <= 5e-5 * np.abs(o).max()
    print("split rows as a Newton update, k %d nn %s: worst |err| / bound %.4f" % (k, nn, worst))


# ------------------------------------------------------------------ e. per-row sweeps on native sides above k_pad 32
@pytest.mark.parametrize("xl,yl,ratio", [("linear", "logit", 0.6), ("logit", "linear", 1.0)])
@pytest.mark.parametrize("k", [40, 100, 200])
def test_per_row_sweeps_on_native_sides(lib, k, xl, yl, ratio):
    """test_native_csr_per_row_sweeps_never_expand of test_gpu_sparse.py (its NumPy-sampler route, the oracle's masks) at
    k_pad 64, 128 and 256: csr_sampled_sub_kernel<16|32|64, 1> subtracts the stored targets of a row's sample from the gradient
    the per-row kernel accumulated with zero targets.  Against the float64 oracle and against the dense expansion on the same
    lists; no dense image afterwards."""
    from oracle import cmf_oracle as O
    rng = np.random.RandomState(5 + k)
    m, d, p = 400, 600, 90
    X = sp.random(m, d, density=0.06, random_state=rng, format="csr", data_rvs=lambda n: rng.rand(n) if xl == "logit" else np.abs(rng.randn(n)) + 0.1)
    Yd = rng.rand(d, p) if yl == "logit" else np.abs(rng.randn(d, p))
    Y = sp.csr_matrix(Yd * (rng.rand(d, p) < 0.3))
    F = [0.3 * rng.randn(n, k) for n in (m, d, p)]
    alpha, l1, l2 = 0.4, 0.01, 0.3
    np.random.seed(9)
    masks = {"U": [], "Z": [], "V": []}
    U, V, Z = (f.copy() for f in F)
    O.newton_update_step(X, Y, U, V, Z, alpha, l1, l2, xl, yl, False, False, False, ratio=ratio, pert=0.2, masks=masks)
    lists = ()
    if ratio < 1:
        lists = (np.array(masks["U"]), np.array(masks["Z"]), np.array([a for a, _ in masks["V"]]), np.array([b for _, b in masks["V"]]))
    got = {}
    for mode in (2, 1):
        ctx = lib.Context(0)
        ctx.set_option("sparse_mode", mode)
        ctx.set_problem(m, d, p, k)
        ctx.set_data(0, X); ctx.set_data(1, Y)
        for w, f in enumerate(F):
            ctx.set_factor(w, f)
        ctx.newton_step(alpha, l1, l2, xl, yl, 0, 7, 0.2, ratio, *lists)
        got[mode] = [ctx.get_factor(w) for w in range(3)]
        if mode == 2:
            assert ctx.data_layout(0) == (False, True) and ctx.data_layout(1) == (False, True)
        ctx.close()
    worst = 0.0
    for a, dense, o in zip(got[2], got[1], (U, V, Z)):
        worst = max(worst, np.abs(a - o).max() / (2e-4 * np.abs(o).max()), np.abs(a - dense).max() / (2e-4 * np.abs(dense).max()))
        np.testing.assert_allclose(a, o, rtol=0, atol=2e-4 * np.abs(o).max())
        np.testing.assert_allclose(a, dense, rtol=0, atol=2e-4 * np.abs(dense).max())
    print("per-row sweeps on native sides, k %d %s/%s ratio %.1f: worst |err| / bound %.4f" % (k, xl, yl, ratio, worst))
