"""The float64 yardstick of the native CSR kernels (sparse_yardstick.py) before any kernel meets it: the exact family is exact in
float32 in any order, the random family stays inside its bounds in float32, and in every case of test_gpu_sparse_products.py a
single dropped or doubled entry moves the result by more than four times the bound it is held to.  No device."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparse_yardstick as S

ORDERS = ("forward", "reverse", "interleaved")
BLOCK_KS = (40, 100, 200)
BLOCK_FALLBACK = 300


def _spmm_cases(family):
    """(name, A, trans, B) of every product the GPU tests form."""
    X, Y = S.row_case(family)
    for width in S.ROW_WIDTHS:
        for trans in (False, True):
            yield "rows X w%d t%d" % (width, trans), X, trans, S.row_operand(0, trans, width, family)
    for trans in (False, True):
        yield "rows Y w40 t%d" % trans, Y, trans, S.row_operand(1, trans, 40, family)
    M = S.blocked_case(family)
    for k in BLOCK_KS + (BLOCK_FALLBACK,):
        for trans in (False, True):
            yield "blocked M w%d t%d" % (k, trans), M, trans, S.blocked_operand(M.shape[0] if trans else M.shape[1], k, family)


def test_case_matrices_are_what_the_kernels_need():
    X, Y = S.row_case("random")
    assert X.shape == (77, 300) and sorted(set(np.diff(X.indptr))) == sorted(S.ROW_LENGTHS)
    assert (np.diff(X.indptr)[-7:] == 0).all() and np.diff(X.indptr)[69] == 300
    assert np.bincount(Y.indices, minlength=Y.shape[1])[17] == 0 and (np.diff(Y.indptr)[-9:] == 0).all()
    M = S.blocked_case("random")
    L = np.diff(M.indptr)
    assert M.shape == (100, 3072) and set(S.BLOCK_LENGTHS + S.BLOCK_HOT) == set(L) and L.mean() < 128
    per_block = np.bincount(M.indices // S.BLOCK_COLS, minlength=48)
    assert per_block[S.BLOCK_EMPTY] == 0 and (np.delete(per_block, S.BLOCK_EMPTY) > 0).all()
    assert S.split_layout(L, 8) == (3, 8, 1024) and S.split_layout(L, 256) == (3, 8, 1024)
    for A in (X, Y, M):
        assert A.has_canonical_format and (A.data != 0).all()
    Xe = S.row_case("exact")[0]
    assert set(np.unique(Xe.data)) <= set(S.EXACT_VALUES) and (S.f32(S.row_case("random")[0].data) == S.row_case("random")[0].data).all()
    for k in S.SDDMM_KS:
        X, Y, F = S.sddmm_case(k, "random")
        assert 0.05 < X.nnz / (130 * 170) < 0.07 and np.diff(X.indptr)[-1] == 0 and (np.diff(X.indptr)[[5, 64, 65]] == 0).all()
        assert all((f < 0).any() and (f > 0).any() for f in F)
        Xl = S.sddmm_case(k, "exact", "logit")[0]
        assert (Xl.data > 0).all() and (Xl.data < 1).all()


def test_exact_family_is_exact_in_float32_in_any_order():
    for name, A, trans, B in _spmm_cases("exact"):
        ref = S.product(A, B, trans)
        assert np.abs(B).max() <= 8 and (B == np.round(B)).all()
        for order in ORDERS:
            assert (S.product_f32(A, B, trans, order) == ref).all(), (name, order)
        assert S.worst_ratio(ref, A, B, trans) == 0.0


def test_random_family_stays_inside_the_product_bound_in_float32():
    worst = 0.0
    for name, A, trans, B in _spmm_cases("random"):
        assert (S.f32(B) == B).all() and (B < 0).any() and (B > 0).any()
        for order in ORDERS:
            r = S.worst_ratio(S.product_f32(A, B, trans, order), A, B, trans)
            worst = max(worst, r)
            assert r <= 1.0, (name, order, r)
    print("float32 NumPy products, three orders: worst |err| / bound %.4f" % worst)
    assert worst > 0.0                                     # the random family does round


def test_a_single_entry_stands_out_of_the_product_bound():
    """Removing (or doubling) any one stored entry moves at least one output element by more than 4 bounds, in every random case."""
    least = np.inf
    for name, A, trans, B in _spmm_cases("random"):
        v = S.single_entry_visibility(A, B, trans)
        least = min(least, v)
        assert v > 4.0, (name, v)
    print("least visible entry: %.1f bounds" % least)
    # and the yardstick does see one: drop the middle entry of the longest row
    M = S.blocked_case("random")
    B = S.blocked_operand(M.shape[1], 40, "random")
    D = M.copy()
    i = int(np.argmax(np.diff(M.indptr)))
    D.data[(M.indptr[i] + M.indptr[i + 1]) // 2] = 0.0
    assert S.worst_ratio(S.product(D, B), M, B) > 4.0
    assert S.worst_ratio(S.product(M, B) + 1e-3 * (np.arange(100)[:, None] == 0), M, B) == np.inf   # an empty row must stay zero


@pytest.mark.parametrize("k", S.SDDMM_KS)
def test_residual_expansion_in_float32(k):
    for family in ("exact", "random"):
        X, Y, (U, V, Z) = S.sddmm_case(k, family)
        for A, L, R in ((X, U, V), (Y, V, Z)):
            ref = S.residual_sq(A, L, R)
            got = S.residual_sq_f32(A, L, R)
            if family == "exact":
                assert got == ref, (k, got, ref)
                continue
            bound = S.residual_bound(A, L, R)
            print("k %d: float32 expansion |err| / bound %.4f" % (k, abs(got - ref) / bound))
            assert abs(got - ref) <= bound
            terms = np.abs(S.cross_terms(A, L, R)[0])
            assert np.median(terms) > 4.0 * bound, (k, np.median(terms) / bound)


def test_exact_factors_meet_in_every_pair_of_rows():
    """At every k the median stored entry of the exact SDDMM case has a non-zero dot product: a dropped entry changes the sum."""
    for k in S.SDDMM_KS:
        X, Y, (U, V, Z) = S.sddmm_case(k, "exact")
        for A, L, R in ((X, U, V), (Y, V, Z)):
            terms = S.cross_terms(A, L, R)[0]
            assert (terms != 0).mean() > 0.5, k
            assert (np.abs(L[L != 0]) >= 0.5).all() and (np.abs(L) <= 2).all()


@pytest.mark.parametrize("k", S.SDDMM_KS)
def test_logit_residual_against_its_expansion(k):
    """The float32 expansion lands within a tenth of the 1e-4 the kernel is held to; and an exchange step of the cross-lane sum
    that went missing would move the root by more than four times that 1e-4, on either side."""
    X, Y, (U, V, Z) = S.sddmm_case(k, "random", "logit")
    least = np.inf
    for A, L, R in ((X, U, V), (Y, V, Z)):
        ref = S.residual_sq(A, L, R, "logit")
        assert abs(np.sqrt(S.residual_sq_logit_f32(A, L, R)) - np.sqrt(ref)) <= 1e-5 * np.sqrt(ref)
        P = 1.0 / (1.0 + np.exp(-(L @ R.T)))
        assert abs(ref - ((A.toarray() - P) ** 2).sum()) <= 1e-12 * ref and np.abs(P - 0.5).mean() > 0.1
        assert all((f < 0).any() and (f > 0).any() for f in (L, R))
        least = min(least, S.logit_lane_visibility(A, L, R))
    print("k %d: a lost exchange step moves the root by at least %.2e" % (k, least))
    assert least > 4e-4
