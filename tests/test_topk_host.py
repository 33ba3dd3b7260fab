"""Host side of top-n prediction (no GPU): argument validation that must raise before any device is touched, the exclusion-list
builder against a dense mask, and the float64 yardstick helper of the GPU tests against a brute-force loop."""
import numpy as np
import pytest
import scipy.sparse as sp

import topk_yardstick as Y


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _model(m=12, d=9, p=5, k=3):
    from pycmf_amd import CMF
    rng = np.random.RandomState(0)
    model = CMF(n_components=k)
    model.x_weights, model.components, model.y_weights = rng.rand(m, k), rng.rand(d, k), rng.rand(p, k)
    return model


@pytest.mark.parametrize("kwargs, match", [
    (dict(relation="z"), "relation"),
    (dict(axis=2), "axis"),
    (dict(rows=[0, 1], queries=np.zeros((2, 3))), "exclude each other"),
    (dict(n=0), "at least 1"),
    (dict(n=-3), "at least 1"),
    (dict(n=129), "maximum"),
    (dict(n=10), "exceeds the 9 candidates"),
    (dict(n=2.5), "integer"),
    (dict(n=2, exclude=sp.csr_matrix((9, 12))), "exclude must have shape"),
    (dict(n=2, axis=1, exclude=sp.csr_matrix((9, 12))), "exclude must have shape"),
    (dict(n=2, rows=[0, 12]), "rows must lie"),
    (dict(n=2, rows=[-1]), "rows must lie"),
    (dict(n=2, rows=[0.5]), "integer index"),
    (dict(n=2, queries=np.zeros((4, 2))), "queries must be"),
    (dict(n=2, queries=np.zeros((4, 3)), exclude=sp.csr_matrix((12, 9))), "exclude must have shape"),
])
def test_top_n_rejects_bad_arguments_before_any_device(no_device, kwargs, match):
    with pytest.raises(ValueError, match=match):
        _model().top_n(**kwargs)


def test_top_n_before_fit_is_the_transform_contract(no_device):
    from pycmf_amd import CMF
    with pytest.raises(AssertionError):
        CMF(n_components=3).top_n()


@pytest.mark.parametrize("kwargs, match", [
    (dict(n=0), "at least 1"),
    (dict(n=200), "maximum"),
    (dict(n=8), "exceeds the 7 candidates"),
    (dict(n=2, link="probit"), "No such link"),
    (dict(n=2, exclude=np.zeros((5, 8))), "exclude must have shape"),
])
def test_top_n_products_rejects_bad_arguments_before_any_device(no_device, kwargs, match):
    import pycmf_amd
    A, B = np.ones((5, 4)), np.ones((7, 4))
    with pytest.raises(ValueError, match=match):
        pycmf_amd.top_n_products(A, B, **kwargs)
    with pytest.raises(ValueError, match="queries must be"):
        pycmf_amd.top_n_products(np.ones((5, 3)), B, 2)


def test_exclusion_lists_match_a_dense_mask():
    from pycmf_amd.prediction import exclusion_lists
    rng = np.random.RandomState(3)
    mask = rng.rand(11, 23) < 0.3
    mask[4] = False          # an empty row
    mask[7] = True           # a full row
    # a CSR whose rows are NOT sorted and that repeats an entry: the builder sorts and merges
    rows, cols = np.nonzero(mask)
    perm = rng.permutation(rows.size)
    M = sp.coo_matrix((np.ones(rows.size + 1), (np.r_[rows[perm], rows[0]], np.r_[cols[perm], cols[0]])), shape=mask.shape)
    csr = sp.csr_matrix((M.data, (M.row, M.col)), shape=mask.shape)
    for src in (csr, sp.csc_matrix(csr), mask.astype(float)):
        indptr, indices = exclusion_lists(src, mask.shape)
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and indptr[0] == 0
        for i in range(mask.shape[0]):
            assert indices[indptr[i]:indptr[i + 1]].tolist() == np.nonzero(mask[i])[0].tolist()
    # a row subset, shuffled, with a repeated row
    pick = np.array([7, 0, 4, 0, 10])
    indptr, indices = exclusion_lists(csr, mask.shape, rows=pick)
    assert indptr.size == pick.size + 1
    for i, r in enumerate(pick):
        assert indices[indptr[i]:indptr[i + 1]].tolist() == np.nonzero(mask[r])[0].tolist()
    # the relation queried along axis 1: the lists of the transpose
    indptr, indices = exclusion_lists(sp.csr_matrix(mask.T.astype(float)), mask.shape, transpose=True)
    for i in range(mask.shape[0]):
        assert indices[indptr[i]:indptr[i + 1]].tolist() == np.nonzero(mask[i])[0].tolist()
    # the caller's matrix is left as it was (unsorted indices stay unsorted)
    before = csr.indices.copy()
    exclusion_lists(csr, mask.shape)
    assert (csr.indices == before).all()
    # stored zeros count: what is stored was seen
    z = sp.csr_matrix((np.zeros(2), (np.array([1, 1]), np.array([5, 2]))), shape=(3, 6))
    indptr, indices = exclusion_lists(z, (3, 6))
    assert indptr.tolist() == [0, 0, 2, 2] and indices.tolist() == [2, 5]


def test_yardstick_matches_brute_force_on_7_by_9():
    rng = np.random.RandomState(5)
    Q = rng.randint(-2, 3, size=(7, 4)).astype(float) + 0.1 * rng.randn(7, 4)
    B = rng.randint(-2, 3, size=(9, 4)).astype(float)
    B[5] = B[2]                                   # a tie in every row
    excl_rows = {1: [0, 3, 8], 4: list(range(9)), 6: [2, 3, 4, 5, 6, 7, 8]}
    indptr = np.zeros(8, dtype=np.int64)
    indices = []
    for i in range(7):
        indices += excl_rows.get(i, [])
        indptr[i + 1] = len(indices)
    excl = (indptr, np.array(indices, dtype=np.int32))
    n = 4
    S = Y.exact_scores(Q, B, excl)
    idx, sc = Y.exact_top_n(S, n)
    Q32, B32 = Q.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)
    for i in range(7):
        cands = []
        for j in range(9):
            if j in excl_rows.get(i, []):
                continue
            s = 0.0
            for t in range(4):
                s += Q32[i, t] * B32[j, t]
            cands.append((-s, j))
        cands.sort()                              # larger score first, then smaller index
        want = [j for _, j in cands[:n]] + [-1] * (n - min(n, len(cands)))
        assert idx[i].tolist() == want
        for t in range(min(n, len(cands))):
            assert abs(sc[i, t] + cands[t][0]) <= 1e-12
        assert np.isneginf(sc[i, len(cands):]).all()
    # the tolerance is the stated formula
    t = Y.tau(Q, B)
    assert np.allclose(t, 1.01 * 32 * 2.0 ** -24 * np.linalg.norm(Q32, axis=1) * np.linalg.norm(B32, axis=1).max(), rtol=1e-12)
    assert [Y.pad_k(k) for k in (1, 7, 32, 33, 64, 100, 128, 129, 256)] == [32, 32, 32, 64, 64, 128, 128, 256, 256]
    # and check_top_n accepts the exact answer, with and without the sigmoid
    val = np.where(idx >= 0, sc, -np.inf).astype(np.float32)
    Y.check_top_n(idx.astype(np.int32), val, Q, B, n, "linear", excl)
    vs = np.where(idx >= 0, Y.sigmoid(sc), -np.inf).astype(np.float32)
    Y.check_top_n(idx.astype(np.int32), vs, Q, B, n, "logit", excl)
    # ... and refuses a wrong one: an excluded candidate, a repeated one, a clearly worse one
    bad = idx.astype(np.int32).copy()
    bad[1, 0] = 3
    with pytest.raises(AssertionError):
        Y.check_top_n(bad, val, Q, B, n, "linear", excl)
    bad = idx.astype(np.int32).copy()
    bad[0, 1] = bad[0, 0]
    with pytest.raises(AssertionError):
        Y.check_top_n(bad, val, Q, B, n, "linear", excl)
    bad = idx.astype(np.int32).copy()
    bad[0, 0] = np.argmin(S[0])
    with pytest.raises(AssertionError):
        Y.check_top_n(bad, val, Q, B, n, "linear", excl)


def test_header_constant_and_kernel_class_agree_with_python():
    import os
    import re
    from pycmf_amd import _lib, prediction
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmfhip.h")).read()
    assert int(re.search(r"#define\s+CMF_TOPK_MAX_N\s+(\d+)", text).group(1)) == prediction.TOPK_MAX_N >= 128
    assert int(re.search(r"CMF_K_TOPK\s*=\s*(\d+)", text).group(1)) == _lib.KERNEL_CLASSES["topk"]
    assert int(re.search(r"CMF_K_COUNT\s*=\s*(\d+)", text).group(1)) == len(_lib.KERNEL_CLASSES)
