"""Ranking metrics over the exact ranks of held-out entries (``CMF.ranks`` / ``rank_products``): plain NumPy, binary relevance.

Every metric is a function of one integer per held-out entry -- how many eligible candidates of its row the model places before
it -- and of two per row: the number h of held-out entries and the number E of eligible candidates.  The reference has no
counterpart."""
import numpy as np


def _check_cutoffs(n):
    try:
        ns = list(n)
    except TypeError:
        ns = [n]
    if not ns:
        raise ValueError("n must name at least one cut-off")
    for v in ns:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("every cut-off n must be an integer of at least 1, got %r" % (v,))
    return [int(v) for v in ns]


def ranking_metrics(indptr, rank, eligible, n=(10,)):
    """Means over the rows that have held-out entries of, per cut-off ``n`` (an integer or several):

    ``hit_rate@n``   any rank < n
    ``recall@n``     #{rank < n} / h
    ``precision@n``  #{rank < n} / n
    ``ndcg@n``       sum over rank < n of 1 / log2(rank + 2), divided by the same sum of the ideal ranks 0 .. min(h, n) - 1

    and of ``mrr`` = 1 / (smallest rank + 1), ``map`` = (1 / h) sum_t (t + 1) / (r_(t) + 1) over the row's ranks in ascending
    order, ``auc`` = 1 - (sum of ranks - h (h - 1) / 2) / (h (E - h)): the fraction of (held-out, other eligible) pairs the model
    orders correctly.  Rows whose eligible candidates are all held out (E = h) have no such pair and are left out of the AUC mean
    (``auc_rows`` counts the others).

    ``indptr`` int[nq + 1] delimits the rows' entries in ``rank`` (0-based ranks among the row's ``eligible[i]`` candidates).
    Entries of rank -1 (their own score was NaN) are dropped and counted in ``dropped``; h is what remains.  ``rows_evaluated`` is
    the number of rows with h >= 1; without any, the means are NaN.  Returns a dict."""
    ns = _check_cutoffs(n)
    indptr = np.asarray(indptr, dtype=np.int64)
    rank = np.asarray(rank, dtype=np.int64)
    eligible = np.asarray(eligible, dtype=np.int64)
    nq = indptr.size - 1
    if indptr.ndim != 1 or nq < 0 or rank.ndim != 1 or eligible.shape != (nq,):
        raise ValueError("indptr must be int[nq + 1], rank 1-d and eligible int[nq]")
    if nq and (indptr[0] != 0 or indptr[-1] != rank.size or (np.diff(indptr) < 0).any()):
        raise ValueError("indptr must rise from 0 to len(rank) = %d" % rank.size)
    row = np.repeat(np.arange(nq, dtype=np.int64), np.diff(indptr))
    keep = rank >= 0
    dropped = int(rank.size - keep.sum())
    row, r = row[keep], rank[keep]
    h = np.bincount(row, minlength=nq).astype(np.float64)
    has = h >= 1
    rows_evaluated = int(has.sum())
    out = {"rows_evaluated": rows_evaluated, "dropped": dropped}
    if (r >= eligible[row]).any():
        raise ValueError("a rank is not below its row's number of eligible candidates")

    def mean(per_row, rows=has):
        return float(per_row[rows].mean()) if rows.any() else float("nan")

    hs = np.where(has, h, 1.0)
    for c in ns:
        inside = r < c
        hits = np.bincount(row[inside], minlength=nq).astype(np.float64)
        dcg = np.bincount(row[inside], weights=1.0 / np.log2(r[inside] + 2.0), minlength=nq)
        ideal = np.concatenate(([0.0], np.cumsum(1.0 / np.log2(np.arange(c) + 2.0))))[np.minimum(h, c).astype(np.int64)]
        out["hit_rate@%d" % c] = mean((hits > 0).astype(np.float64))
        out["recall@%d" % c] = mean(hits / hs)
        out["precision@%d" % c] = mean(hits / c)
        out["ndcg@%d" % c] = mean(dcg / np.where(has, ideal, 1.0))
    order = np.lexsort((r, row))                       # by row, ranks ascending inside a row
    rs, rows_s = r[order], row[order]
    start = np.concatenate(([0], np.cumsum(h.astype(np.int64))))[:-1]
    t = np.arange(rs.size, dtype=np.int64) - start[rows_s]    # place of the entry among its row's sorted ranks
    first = np.full(nq, 0.0)
    first[rows_s[t == 0]] = 1.0 / (rs[t == 0] + 1.0)
    out["mrr"] = mean(first)
    out["map"] = mean(np.bincount(rows_s, weights=(t + 1.0) / (rs + 1.0), minlength=nq) / hs)
    pairs = h * (eligible - h)
    with_pairs = has & (pairs > 0)
    wrong = np.bincount(row, weights=r.astype(np.float64), minlength=nq) - h * (h - 1.0) / 2.0
    out["auc"] = mean(1.0 - wrong / np.where(with_pairs, pairs, 1.0), with_pairs)
    out["auc_rows"] = int(with_pairs.sum())
    return out
