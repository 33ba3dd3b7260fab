"""Host side of held-out ranking evaluation (no GPU): ``ranking_metrics`` against brute force and scikit-learn, the held-out list
builder, the argument validation that must raise before any device is touched, and the declarations of the three entry points."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a context fails the test."""
    from pycmf_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened before the arguments were validated")
    monkeypatch.setattr(_lib, "Context", boom)


def _ranks_from_scores(S, held, excl=None):
    """Brute force: CSR pair and 0-based ranks of the held-out entries of a dense score matrix (argsort, excluded removed)."""
    indptr, rank, eligible = [0], [], []
    for i in range(S.shape[0]):
        out = set(np.flatnonzero(excl[i]).tolist()) if excl is not None else set()
        order = [c for c in np.argsort(-S[i], kind="stable").tolist() if c not in out]
        pos = {c: t for t, c in enumerate(order)}
        for j in np.flatnonzero(held[i]).tolist():
            rank.append(pos[j])
        indptr.append(len(rank))
        eligible.append(len(order))
    return np.array(indptr), np.array(rank), np.array(eligible)


def _textbook(indptr, rank, eligible, ns):
    """The definitions, row by row, in plain Python."""
    per = {"mrr": [], "map": [], "auc": []}
    for c in ns:
        for name in ("hit_rate", "recall", "precision", "ndcg"):
            per["%s@%d" % (name, c)] = []
    for i in range(len(indptr) - 1):
        r = sorted(int(x) for x in rank[indptr[i]:indptr[i + 1]] if x >= 0)
        h, E = len(r), int(eligible[i])
        if h == 0:
            continue
        for c in ns:
            inside = [x for x in r if x < c]
            per["hit_rate@%d" % c].append(1.0 if inside else 0.0)
            per["recall@%d" % c].append(len(inside) / h)
            per["precision@%d" % c].append(len(inside) / c)
            per["ndcg@%d" % c].append(sum(1.0 / np.log2(x + 2.0) for x in inside) / sum(1.0 / np.log2(t + 2.0) for t in range(min(h, c))))
        per["mrr"].append(1.0 / (r[0] + 1))
        per["map"].append(sum((t + 1.0) / (x + 1.0) for t, x in enumerate(r)) / h)
        if E > h:
            per["auc"].append(1.0 - (sum(r) - h * (h - 1) / 2.0) / (h * (E - h)))
    return {k: (float(np.mean(v)) if v else float("nan")) for k, v in per.items()}, len(per["mrr"])


@pytest.mark.parametrize("seed, with_excl", [(0, False), (1, True), (2, True)])
def test_ranking_metrics_match_brute_force_on_dense_scores(seed, with_excl):
    from pycmf_amd import ranking_metrics
    rng = np.random.RandomState(seed)
    nq, C = 40, 57
    S = rng.randn(nq, C)
    held = rng.rand(nq, C) < 0.08
    held[3] = False                                  # a row without held-out entries
    excl = None
    if with_excl:
        excl = (rng.rand(nq, C) < 0.3) & ~held
    indptr, rank, eligible = _ranks_from_scores(S, held, excl)
    ns = (1, 5, 10, 60)
    got = ranking_metrics(indptr, rank, eligible, n=ns)
    want, rows = _textbook(indptr, rank, eligible, ns)
    assert got["rows_evaluated"] == rows == int((held.sum(axis=1) > 0).sum()) and got["dropped"] == 0
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, k


def test_ranking_metrics_match_scikit_learn_per_row():
    from sklearn.metrics import ndcg_score, roc_auc_score
    from pycmf_amd import ranking_metrics
    rng = np.random.RandomState(7)
    nq, C = 25, 80
    S = rng.randn(nq, C)                              # tie-free
    held = rng.rand(nq, C) < 0.1
    held[:, 0] |= ~held.any(axis=1)                   # every row has one
    indptr, rank, eligible = _ranks_from_scores(S, held)
    for i in range(nq):
        one = ranking_metrics(indptr[i:i + 2] - indptr[i], rank[indptr[i]:indptr[i + 1]], eligible[i:i + 1], n=(5, 10))
        assert abs(one["auc"] - roc_auc_score(held[i], S[i])) <= 1e-12
        for c in (5, 10):
            assert abs(one["ndcg@%d" % c] - ndcg_score(held[i:i + 1].astype(float), S[i:i + 1], k=c)) <= 1e-12
    allrows = ranking_metrics(indptr, rank, eligible, n=10)
    assert abs(allrows["auc"] - np.mean([roc_auc_score(held[i], S[i]) for i in range(nq)])) <= 1e-12
    assert abs(allrows["ndcg@10"] - np.mean([ndcg_score(held[i:i + 1].astype(float), S[i:i + 1], k=10) for i in range(nq)])) <= 1e-12


def test_ranking_metrics_edge_rows():
    from pycmf_amd import ranking_metrics
    # h = 0 rows are skipped
    m = ranking_metrics([0, 0, 2, 2], [0, 1], [9, 9, 9], n=(1, 2))
    assert m["rows_evaluated"] == 1 and m["recall@2"] == 1.0 and m["recall@1"] == 0.5 and m["precision@1"] == 1.0
    # a perfect ranking: every metric 1 (precision at n = h)
    m = ranking_metrics([0, 3], [2, 0, 1], [50], n=3)
    for k in ("hit_rate@3", "recall@3", "precision@3", "ndcg@3", "mrr", "map", "auc"):
        assert m[k] == 1.0, k
    # the worst ranking: the held-out entries are the last three of 50
    m = ranking_metrics([0, 3], [47, 49, 48], [50], n=(10, 50))
    assert m["hit_rate@10"] == 0.0 and m["recall@10"] == 0.0 and m["ndcg@10"] == 0.0 and m["auc"] == 0.0
    assert m["recall@50"] == 1.0 and abs(m["mrr"] - 1.0 / 48) <= 1e-15
    assert abs(m["map"] - (1 / 48 + 2 / 49 + 3 / 50) / 3) <= 1e-15
    # E = h: no pair to order, the row is left out of the AUC mean only
    m = ranking_metrics([0, 2, 3], [1, 0, 4], [2, 10], n=2)
    assert m["rows_evaluated"] == 2 and m["auc_rows"] == 1 and abs(m["auc"] - (1 - 4 / 9)) <= 1e-15
    assert m["recall@2"] == 0.5 and m["mrr"] == (1.0 + 1 / 5) / 2
    m = ranking_metrics([0, 2], [1, 0], [2])
    assert np.isnan(m["auc"]) and m["auc_rows"] == 0 and m["recall@10"] == 1.0
    # rank -1 entries are dropped and counted; a row left with none is not evaluated
    m = ranking_metrics([0, 2, 3], [-1, 3, -1], [20, 20], n=4)
    assert m["dropped"] == 2 and m["rows_evaluated"] == 1 and m["recall@4"] == 1.0 and m["mrr"] == 0.25
    # nothing to evaluate
    m = ranking_metrics([0, 0], [], [5])
    assert m["rows_evaluated"] == 0 and np.isnan(m["mrr"]) and np.isnan(m["recall@10"])
    # an integer cut-off and several at once give the same numbers
    a = ranking_metrics([0, 2, 5], [0, 7, 3, 1, 30], [40, 40], n=5)
    b = ranking_metrics([0, 2, 5], [0, 7, 3, 1, 30], [40, 40], n=(2, 5, 9))
    assert a["ndcg@5"] == b["ndcg@5"] and a["map"] == b["map"] and set(b) >= {"recall@2", "recall@5", "recall@9"}
    for bad in (0, (), (3, 0), 2.5, (True,)):
        with pytest.raises(ValueError):
            ranking_metrics([0, 1], [0], [3], n=bad)
    with pytest.raises(ValueError):
        ranking_metrics([0, 1], [3], [3])             # a rank needs that many candidates before it
    with pytest.raises(ValueError):
        ranking_metrics([0, 2], [0], [3])


def test_held_out_lists_sort_merge_subset_and_transpose():
    from pycmf_amd.prediction import held_out_lists
    rng = np.random.RandomState(3)
    mask = rng.rand(11, 23) < 0.3
    mask[4] = False
    rows, cols = np.nonzero(mask)
    perm = rng.permutation(rows.size)
    # unsorted, with a repeated entry
    M = sp.coo_matrix((np.ones(rows.size + 1), (np.r_[rows[perm], rows[0]], np.r_[cols[perm], cols[0]])), shape=mask.shape)
    csr = sp.csr_matrix((M.data, (M.row, M.col)), shape=mask.shape)
    for src in (csr, sp.csc_matrix(csr), mask.astype(float)):
        indptr, indices = held_out_lists(src, mask.shape)
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and indptr[0] == 0 and indptr[-1] == mask.sum()
        for i in range(mask.shape[0]):
            assert indices[indptr[i]:indptr[i + 1]].tolist() == np.nonzero(mask[i])[0].tolist()
    pick = np.array([7, 0, 4, 0, 10])
    indptr, indices = held_out_lists(csr, mask.shape, rows=pick)
    assert indptr.size == pick.size + 1
    for i, r in enumerate(pick):
        assert indices[indptr[i]:indptr[i + 1]].tolist() == np.nonzero(mask[r])[0].tolist()
    indptr, indices = held_out_lists(sp.csr_matrix(mask.T.astype(float)), mask.shape, transpose=True)
    for i in range(mask.shape[0]):
        assert indices[indptr[i]:indptr[i + 1]].tolist() == np.nonzero(mask[i])[0].tolist()
    with pytest.raises(ValueError, match="held_out must have shape"):
        held_out_lists(csr, (23, 11))


def _model(m=12, d=9, p=5, k=3):
    from pycmf_amd import CMF
    rng = np.random.RandomState(0)
    model = CMF(n_components=k)
    model.x_weights, model.components, model.y_weights = rng.rand(m, k), rng.rand(d, k), rng.rand(p, k)
    return model


def _one(shape, i, j):
    return sp.csr_matrix((np.ones(1), (np.array([i]), np.array([j]))), shape=shape)


@pytest.mark.parametrize("kwargs, match", [
    (dict(held_out=_one((12, 9), 0, 0), relation="z"), "relation"),
    (dict(held_out=_one((12, 9), 0, 0), axis=2), "axis"),
    (dict(held_out=_one((2, 9), 0, 0), rows=[0, 1], queries=np.zeros((2, 3))), "exclude each other"),
    (dict(held_out=_one((9, 12), 0, 0)), "held_out must have shape"),
    (dict(held_out=_one((9, 12), 0, 0), axis=1), "held_out must have shape"),
    (dict(held_out=_one((12, 9), 0, 0), relation="y"), "held_out must have shape"),
    (dict(held_out=np.zeros(9)), "held_out must be a 2-d matrix"),
    (dict(held_out=_one((12, 9), 0, 0), exclude=sp.csr_matrix((9, 12))), "exclude must have shape"),
    (dict(held_out=_one((12, 9), 0, 0), rows=[0, 12]), "rows must lie"),
    (dict(held_out=_one((12, 9), 0, 0), rows=[0.5]), "integer index"),
    (dict(held_out=_one((4, 9), 0, 0), queries=np.zeros((4, 2))), "queries must be"),
    (dict(held_out=_one((12, 9), 0, 0), queries=np.zeros((4, 3))), "held_out must have shape"),
    (dict(held_out=_one((12, 9), 5, 2), exclude=_one((12, 9), 5, 2)), "leak"),
    (dict(held_out=_one((12, 9), 5, 2), exclude=_one((12, 9), 5, 2), rows=[5, 5]), "leak"),
    (dict(held_out=_one((12, 9), 5, 2), exclude=_one((12, 9), 5, 2), axis=1), "leak"),
])
def test_ranks_and_evaluate_reject_bad_arguments_before_any_device(no_device, kwargs, match):
    with pytest.raises(ValueError, match=match):
        _model().ranks(**kwargs)
    with pytest.raises(ValueError, match=match):
        _model().evaluate(**kwargs)


def test_evaluate_rejects_bad_cutoffs_and_unfitted_models_before_any_device(no_device):
    from pycmf_amd import CMF
    for bad in (0, (), (5, -1), 1.5):
        with pytest.raises(ValueError, match="cut-off"):
            _model().evaluate(_one((12, 9), 0, 0), n=bad)
    with pytest.raises(AssertionError):
        CMF(n_components=3).ranks(_one((12, 9), 0, 0))
    with pytest.raises(AssertionError):
        CMF(n_components=3).evaluate(_one((12, 9), 0, 0))


@pytest.mark.parametrize("kwargs, match", [
    (dict(held_out=_one((5, 8), 0, 0)), "held_out must have shape"),
    (dict(held_out=_one((5, 7), 0, 0), exclude=np.zeros((5, 8))), "exclude must have shape"),
    (dict(held_out=_one((5, 7), 1, 6), exclude=_one((5, 7), 1, 6)), "leak"),
])
def test_rank_products_rejects_bad_arguments_before_any_device(no_device, kwargs, match):
    import pycmf_amd
    A, B = np.ones((5, 4)), np.ones((7, 4))
    with pytest.raises(ValueError, match=match):
        pycmf_amd.rank_products(A, B, **kwargs)
    with pytest.raises(ValueError, match="queries must be"):
        pycmf_amd.rank_products(np.ones((5, 3)), B, _one((5, 7), 0, 0))
    with pytest.raises(ValueError, match="non-empty"):
        pycmf_amd.rank_products(A, np.ones(4), _one((5, 7), 0, 0))


def test_context_rank_checks_list_lengths_before_the_library_call():
    """``Context.rank`` sizes its outputs from the lists: a list that does not fit the queries must not reach the C side."""
    from pycmf_amd import _lib

    class Fake(_lib.Context):
        def __init__(self):                            # no device, no library
            self.shape = (4, 6, 3, 2)
            self._lib = None
            self._h = None

        def __del__(self):
            pass
    ctx = Fake()
    with pytest.raises(ValueError, match="held: indptr must have nq \\+ 1 = 5"):
        ctx.rank(0, 1, (np.zeros(4, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    with pytest.raises(ValueError, match="held: indptr points beyond"):
        ctx.rank(0, 1, (np.array([0, 1, 1, 1, 2]), np.zeros(1, dtype=np.int32)))
    with pytest.raises(ValueError, match="exclude: indptr must have"):
        ctx.rank(0, 1, (np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32)), rows=[0, 1],
                 exclude=(np.zeros(2, dtype=np.int64), np.zeros(0, dtype=np.int32)))
    with pytest.raises(ValueError, match="exclude each other"):
        ctx.rank(0, 1, (np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32)), rows=[0, 1], queries=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="queries must be"):
        ctx.rank(0, 1, (np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32)), queries=np.zeros((2, 3)))


def test_header_prototypes_and_context_declare_the_three_entry_points():
    import pycmf_amd
    from pycmf_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmfhip.h")).read()
    for name, nargs in (("cmf_rank", 12), ("cmf_rank_queries", 13), ("cmf_rank_layout", 7)):
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name]), name
    assert callable(_lib.Context.rank) and callable(_lib.Context.rank_layout)
    assert int(re.search(r"CMF_K_COUNT\s*=\s*(\d+)", text).group(1)) == len(_lib.KERNEL_CLASSES) == 11
    assert "topk_split" in text and "cmf_rank / cmf_rank_queries" in text
    for name in ("rank_products", "ranking_metrics", "CMF"):
        assert name in pycmf_amd.__all__ and callable(getattr(pycmf_amd, name))
    assert callable(pycmf_amd.CMF.ranks) and callable(pycmf_amd.CMF.evaluate)


def test_built_library_exports_the_three_entry_points():
    from pycmf_amd import _lib
    lib = _lib.load()
    for name in ("cmf_rank", "cmf_rank_queries", "cmf_rank_layout"):
        assert getattr(lib, name) is not None
