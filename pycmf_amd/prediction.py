"""Top-n prediction from fitted factors: for every query row the n candidates with the largest f(q . b_j), computed on the device
without ever forming the product (csrc/cmf_topk.hip.h through ``Context.topk``) -- and the exact rank of held-out entries under
the same order (csrc/cmf_rank.hip.h through ``Context.rank``; the metrics over those ranks: evaluation.py).

The reference has no counterpart: it returns the three factor arrays and its only consumer of them is the host argsort of
pycmf/analysis.py:3-16.  Everything here that can fail on its arguments fails BEFORE a device is touched.
"""
import numpy as np

from . import _lib

TOPK_MAX_N = 128   # CMF_TOPK_MAX_N of include/cmfhip.h

# relation, axis -> (query factor, candidate factor): X ~ f(U V^T), Y ~ f(V Z^T)
_PAIRS = {("x", 0): (_lib.CMF_U, _lib.CMF_V), ("x", 1): (_lib.CMF_V, _lib.CMF_U),
          ("y", 0): (_lib.CMF_V, _lib.CMF_Z), ("y", 1): (_lib.CMF_Z, _lib.CMF_V)}


def exclusion_lists(exclude, shape, rows=None, transpose=False, name="exclude"):
    """CSR pair ``(indptr int64[nq + 1], indices int32)`` of the entries to skip: row i lists, strictly ascending, the columns that
    ``exclude`` stores in row ``rows[i]`` (``rows=None``: every row).  ``exclude`` is a SciPy sparse matrix or a dense array (its
    non-zeros count) of shape ``shape`` -- of ``shape[::-1]`` when ``transpose`` (a relation queried along axis 1).  Explicitly
    stored zeros of a sparse matrix are skipped entries too: what is stored was seen."""
    import scipy.sparse as sp
    want = tuple(shape[::-1]) if transpose else tuple(shape)
    if not sp.issparse(exclude):
        exclude = np.asarray(exclude)
        if exclude.ndim != 2:
            raise ValueError("%s must be a 2-d matrix of shape %r, got %d dimension(s)" % (name, want, exclude.ndim))
    if tuple(exclude.shape) != want:
        raise ValueError("%s must have shape %r, got %r" % (name, want, tuple(exclude.shape)))
    if shape[1] > np.iinfo(np.int32).max:
        raise ValueError("%s: %d candidates do not fit int32 indices" % (name, shape[1]))
    M = sp.csr_matrix(exclude.T if transpose else exclude)
    M = M[np.asarray(rows, dtype=np.int64)] if rows is not None else M.copy()   # never the caller's own arrays
    M.sum_duplicates()        # sorts the column indices of every row and merges repeated ones
    return np.asarray(M.indptr, dtype=np.int64), np.asarray(M.indices, dtype=np.int32)


def _check_n(n, ncand):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise ValueError("n must be an integer, got %r" % (n,))
    if n < 1:
        raise ValueError("n must be at least 1, got %d" % n)
    if n > TOPK_MAX_N:
        raise ValueError("n = %d exceeds the supported maximum %d" % (n, TOPK_MAX_N))
    if n > ncand:
        raise ValueError("n = %d exceeds the %d candidates" % (n, ncand))
    return int(n)


def _check_link(link):
    if link not in _lib.LINKS:
        raise ValueError("No such link %s" % (link,))
    return link


def _check_queries(queries, k):
    Q = np.asarray(queries, dtype=np.float64)
    if Q.ndim != 2 or Q.shape[1] != k:
        raise ValueError("queries must be an (nq, %d) array, got shape %r" % (k, Q.shape))
    return Q


def _check_rows(rows, nrows):
    r = np.asarray(rows)
    if r.ndim != 1 or (r.size and not np.issubdtype(r.dtype, np.integer)):
        raise ValueError("rows must be a 1-d integer index array")
    r = r.astype(np.int64)
    if r.size and (r.min() < 0 or r.max() >= nrows):
        raise ValueError("rows must lie in [0, %d)" % nrows)
    return r


def _augmented(factors, qf, cf, bias, axis, rows, queries, query_bias):
    """(queries, candidates) of a biased relation for the top-n and rank kernels, which know dot products only:
    query rows [f | 1 | offset + own bias], candidate rows [f | candidate bias | 1] -- so that q . c is the prediction itself and
    the order includes the candidate's bias.  ``bias``: (offset, rows, cols) of the relation; ``axis`` 1 swaps their roles."""
    offset, rb, cb = bias
    qb, kb = (rb, cb) if axis == 0 else (cb, rb)
    C = np.asarray(factors[cf], dtype=np.float64)
    k = C.shape[1]
    if k + 2 > 256:
        raise NotImplementedError("top_n / ranks on a model with biases need n_components + 2 <= 256, got n_components = %d" % k)
    if queries is not None:
        Q = queries
        own = np.zeros(Q.shape[0]) if query_bias is None else np.asarray(query_bias, dtype=np.float64).ravel()
        if own.shape != (Q.shape[0],):
            raise ValueError("query_bias must hold one value per query (%d), got shape %r" % (Q.shape[0], np.shape(query_bias)))
    else:
        if query_bias is not None:
            raise ValueError("query_bias goes with queries: the fitted rows have their fitted biases")
        Q = np.asarray(factors[qf], dtype=np.float64)
        own = np.asarray(qb, dtype=np.float64)
        if rows is not None:
            Q, own = Q[rows], own[rows]
    Qa = np.concatenate([Q, np.ones((Q.shape[0], 1)), (float(offset) + own)[:, None]], axis=1)
    Ca = np.concatenate([C, np.asarray(kb, dtype=np.float64)[:, None], np.ones((C.shape[0], 1))], axis=1)
    return Qa, Ca


def _problem_rows(cf, ncand):
    """Row counts of a problem whose candidate factor has ``ncand`` rows (the others are placeholders of one row)."""
    rows = [1, 1, 1]
    rows[cf] = ncand
    return rows


def predict_products(A, B, rows, cols, link="linear", row_bias=None, col_bias=None, offset=0.0, device=0):
    """float32[n]: ``f(offset + row_bias[i] + col_bias[j] + a_i . b_j)`` for the pairs ``(i, j) = (rows[q], cols[q])`` of rows of
    ``A`` (m x k) and ``B`` (d x k).  ``link``: 'linear' | 'logit' (sigmoid); ``row_bias`` / ``col_bias``: vectors of m / d values or
    None (zeros).  Float32 arithmetic on GPU ``device`` (csrc/cmf_als_bias.hip.h, one lane group per pair); the m x d product is
    never formed.  Everything that can fail on its arguments fails before a device is touched."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or A.shape[1] < 1 or A.shape[0] < 1 or B.shape[0] < 1:
        raise ValueError("A and B must be non-empty (m, k) and (d, k) arrays, got shapes %r and %r" % (A.shape, B.shape))
    if A.shape[1] > 256:
        raise NotImplementedError("predict_products is built for at most 256 components, got %d" % A.shape[1])
    _check_link(link)
    rows, cols = np.asarray(rows), np.asarray(cols)
    if rows.ndim != 1 or cols.ndim != 1 or rows.shape != cols.shape:
        raise ValueError("rows and cols must be 1-d index arrays of one length, got shapes %r and %r" % (rows.shape, cols.shape))
    if rows.size and not (np.issubdtype(rows.dtype, np.integer) and np.issubdtype(cols.dtype, np.integer)):
        raise ValueError("rows and cols must be integer index arrays")
    rows, cols = rows.astype(np.int64), cols.astype(np.int64)
    if rows.size and (rows.min() < 0 or rows.max() >= A.shape[0] or cols.min() < 0 or cols.max() >= B.shape[0]):
        raise ValueError("rows must lie in [0, %d) and cols in [0, %d)" % (A.shape[0], B.shape[0]))
    offset = float(offset)
    if not np.isfinite(offset):
        raise ValueError("offset must be finite, got %r" % (offset,))
    biased = row_bias is not None or col_bias is not None or offset != 0.0
    vecs = []
    for v, n, nm in ((row_bias, A.shape[0], "row_bias"), (col_bias, B.shape[0], "col_bias")):
        v = np.zeros(n) if v is None else np.asarray(v, dtype=np.float64).ravel()
        if v.shape != (n,) or not np.isfinite(v).all():
            raise ValueError("%s must hold %d finite values" % (nm, n))
        vecs.append(v)
    if rows.size == 0:
        return np.zeros(0, dtype=np.float32)
    ctx = _lib.Context(device)
    try:
        ctx.set_problem(A.shape[0], B.shape[0], 1, A.shape[1])
        ctx.set_factor(_lib.CMF_U, A)
        ctx.set_factor(_lib.CMF_V, B)
        if biased:   # the bias terms live on a relation with CSR weights: an empty pattern carries them
            ctx.set_weighted_csr(0, np.zeros(A.shape[0] + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0), np.zeros(0))
            ctx.set_biases(0, True, offset, 0.0)
            ctx.set_bias(0, 0, vecs[0])
            ctx.set_bias(0, 1, vecs[1])
        return ctx.predict_pairs(0, rows, cols, link=link)
    finally:
        ctx.close()


def top_n_products(A, B, n, link="linear", exclude=None, device=0):
    """For every row a_i of ``A`` (nq x k) the ``n`` rows b_j of ``B`` (C x k) with the largest ``f(a_i . b_j)``:
    ``(idx int32[nq, n], val float32[nq, n])``, best first, equal scores by smaller j.  ``link``: 'linear' | 'logit' (sigmoid).
    ``exclude``: (nq x C) sparse or dense matrix whose stored / non-zero entries are skipped; a row with fewer than n candidates
    left has ``-1 / -inf`` in the remaining places.  Float32 arithmetic on GPU ``device``; the nq x C product is never formed."""
    B = np.asarray(B, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] < 1 or B.shape[1] < 1:
        raise ValueError("B must be a non-empty (C, k) array, got shape %r" % (B.shape,))
    A = _check_queries(A, B.shape[1])
    n = _check_n(n, B.shape[0])
    _check_link(link)
    excl = None if exclude is None else exclusion_lists(exclude, (A.shape[0], B.shape[0]))
    ctx = _lib.Context(device)
    try:
        ctx.set_problem(1, B.shape[0], 1, B.shape[1])
        ctx.set_factor(_lib.CMF_V, B)
        return ctx.topk(_lib.CMF_U, _lib.CMF_V, n, link=link, exclude=excl, queries=A)
    finally:
        ctx.close()


def model_top_n(U, V, Z, x_link, y_link, device, relation="x", axis=0, rows=None, n=10, exclude=None, queries=None, bias=None,
                query_bias=None):
    """``CMF.top_n`` on explicit factors (see there).  ``bias``: (offset, rows, cols) of a relation fitted with biases -- the
    kernels then run on augmented factors (``_augmented``), ``query_bias`` the biases of ``queries`` (default 0)."""
    if relation not in ("x", "y"):
        raise ValueError("relation must be 'x' or 'y', got %r" % (relation,))
    if axis not in (0, 1):
        raise ValueError("axis must be 0 or 1, got %r" % (axis,))
    if rows is not None and queries is not None:
        raise ValueError("rows and queries exclude each other: queries replace the fitted rows")
    factors = (U, V, Z)
    qf, cf = _PAIRS[(relation, axis)]
    ncand, k = factors[cf].shape
    n = _check_n(n, ncand)
    link = _check_link(x_link if relation == "x" else y_link)
    if queries is not None:
        queries = _check_queries(queries, k)
        nrows = queries.shape[0]
    else:
        nrows = factors[qf].shape[0]
        if rows is not None:
            rows = _check_rows(rows, nrows)
    excl = None
    if exclude is not None:
        excl = exclusion_lists(exclude, (nrows, ncand), rows=rows, transpose=(axis == 1))
    if bias is None and query_bias is not None:
        raise ValueError("query_bias needs a model fitted with biases on relation %r" % (relation,))
    if bias is not None:
        Qa, Ca = _augmented(factors, qf, cf, bias, axis, rows, queries, query_bias)
    ctx = _lib.Context(device)
    try:
        if bias is not None:
            ctx.set_problem(*_problem_rows(cf, ncand), k + 2)
            ctx.set_factor(cf, Ca)
            return ctx.topk(qf, cf, n, link=link, exclude=excl, queries=Qa)
        ctx.set_problem(U.shape[0], V.shape[0], Z.shape[0], k)
        ctx.set_factor(cf, factors[cf])
        if queries is None:
            ctx.set_factor(qf, factors[qf])
        return ctx.topk(qf, cf, n, link=link, rows=rows, exclude=excl, queries=queries)
    finally:
        ctx.close()


def held_out_lists(held_out, shape, rows=None, transpose=False):
    """CSR pair ``(indptr int64[nq + 1], indices int32)`` of the held-out entries: ``exclusion_lists`` under another name -- row i
    lists, strictly ascending, the columns that ``held_out`` stores in row ``rows[i]`` (``rows=None``: every row; ``transpose``:
    ``held_out`` has ``shape[::-1]``, a relation queried along axis 1).  Repeated entries are merged, stored zeros count."""
    return exclusion_lists(held_out, shape, rows=rows, transpose=transpose, name="held_out")


def _check_no_leak(held, excl, ncand):
    """A held-out entry that the exclusion lists store too is a test entry among the training entries."""
    if excl is None or not held[1].size or not excl[1].size:
        return
    def keys(pair):
        return np.repeat(np.arange(pair[0].size - 1, dtype=np.int64), np.diff(pair[0])) * ncand + pair[1]
    hk = keys(held)
    both = np.isin(hk, keys(excl), assume_unique=True)
    if both.any():
        e = int(np.flatnonzero(both)[0])
        raise ValueError("%d held-out entries are also stored in exclude (the first: query %d, candidate %d): a test entry among "
                         "the training entries is a leak" % (int(both.sum()), hk[e] // ncand, hk[e] % ncand))


def rank_products(A, B, held_out, exclude=None, device=0):
    """Exact ranks of the entries ``held_out`` stores (nq x C sparse or dense matrix) among the scores ``a_i . b_j`` of row i of
    ``A`` (nq x k) against the rows of ``B`` (C x k): ``(indptr, indices, rank, eligible)`` -- the canonical CSR order of
    ``held_out``, ``rank[e]`` = how many candidates outside row i's ``exclude`` list score higher than entry e (equal scores: a
    smaller index goes first; 0-based), ``eligible[i]`` = C - the length of that list.  A held-out entry that ``exclude`` stores as
    well is a ``ValueError``.  Float32 arithmetic on GPU ``device``, the order of ``top_n_products``; the product is never formed."""
    B = np.asarray(B, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] < 1 or B.shape[1] < 1:
        raise ValueError("B must be a non-empty (C, k) array, got shape %r" % (B.shape,))
    A = _check_queries(A, B.shape[1])
    held = held_out_lists(held_out, (A.shape[0], B.shape[0]))
    excl = None if exclude is None else exclusion_lists(exclude, (A.shape[0], B.shape[0]))
    _check_no_leak(held, excl, B.shape[0])
    ctx = _lib.Context(device)
    try:
        ctx.set_problem(1, B.shape[0], 1, B.shape[1])
        ctx.set_factor(_lib.CMF_V, B)
        rank, _, eligible = ctx.rank(_lib.CMF_U, _lib.CMF_V, held, exclude=excl, queries=A)
    finally:
        ctx.close()
    return held[0], held[1], rank, eligible


def model_ranks(U, V, Z, device, held_out, relation="x", axis=0, exclude=None, rows=None, queries=None, bias=None, query_bias=None):
    """``CMF.ranks`` on explicit factors (see there); ``bias`` / ``query_bias`` as in ``model_top_n``."""
    if relation not in ("x", "y"):
        raise ValueError("relation must be 'x' or 'y', got %r" % (relation,))
    if axis not in (0, 1):
        raise ValueError("axis must be 0 or 1, got %r" % (axis,))
    if rows is not None and queries is not None:
        raise ValueError("rows and queries exclude each other: queries replace the fitted rows")
    factors = (U, V, Z)
    qf, cf = _PAIRS[(relation, axis)]
    ncand, k = factors[cf].shape
    if queries is not None:
        queries = _check_queries(queries, k)
        nrows = queries.shape[0]
    else:
        nrows = factors[qf].shape[0]
        if rows is not None:
            rows = _check_rows(rows, nrows)
    held = held_out_lists(held_out, (nrows, ncand), rows=rows, transpose=(axis == 1))
    excl = None
    if exclude is not None:
        excl = exclusion_lists(exclude, (nrows, ncand), rows=rows, transpose=(axis == 1))
    _check_no_leak(held, excl, ncand)
    if bias is None and query_bias is not None:
        raise ValueError("query_bias needs a model fitted with biases on relation %r" % (relation,))
    if bias is not None:
        Qa, Ca = _augmented(factors, qf, cf, bias, axis, rows, queries, query_bias)
    ctx = _lib.Context(device)
    try:
        if bias is not None:
            ctx.set_problem(*_problem_rows(cf, ncand), k + 2)
            ctx.set_factor(cf, Ca)
            rank, _, eligible = ctx.rank(qf, cf, held, exclude=excl, queries=Qa)
            return held[0], held[1], rank, eligible
        ctx.set_problem(U.shape[0], V.shape[0], Z.shape[0], k)
        ctx.set_factor(cf, factors[cf])
        if queries is None:
            ctx.set_factor(qf, factors[qf])
        rank, _, eligible = ctx.rank(qf, cf, held, rows=rows, exclude=excl, queries=queries)
    finally:
        ctx.close()
    return held[0], held[1], rank, eligible
