"""NumPy yardstick of the dual form of the exact ALS rows (helper of test_als_dual_host.py / test_gpu_als_dual.py; not collected).

A sweep without a shared term (every relation it reads observed, no background weight) gives row i, with its stored entries
e = 1 .. n (side 0 then side 1, stored order), weights w_e >= 0, p_e = w_e t_e and gathered factor rows b_e,

    a_e = sqrt(w_e) b_e   (A: n x k),     y_e = p_e / sqrt(w_e)   (0 where w_e = 0),
    primal:  (A^T A + l2 I_k) f = A^T y           (als_yardstick.sweep, route "rows exact")
    dual:    K = A A^T + l2 I_n,   K z = y,   f = A^T z

and  A^T (A A^T + l2 I_n)^-1 = (A^T A + l2 I_k)^-1 A^T  makes the two the same f.  ``plan`` mirrors the device's planner: a row goes
dual when 1 <= n <= dual_max and its class width NP(n) -- the smallest of 32, 64, 128 that is >= n -- is below k_pad; a row without
a stored entry is zeros; every other row takes the formed route.  ``dtype=np.float32`` runs the same formulas on float32 arrays and
exists only to size the tolerances of the device tests (als_yardstick.tolerance); ``order`` re-associates its sums (the envelope
of DESIGN section 23: the largest tolerance over four summation orders)."""
import numpy as np

import als_yardstick as A

ZERO, FORMED = "zero", "formed"
ORDERS = ("forward", "reverse", "pairs", "halves")


def k_pad(k):
    return 32 if k <= 32 else 64 if k <= 64 else 128 if k <= 128 else 256 * ((k + 255) // 256)


def class_width(n):
    """NP(n): the smallest of 32, 64, 128 that is >= n (n <= 128)."""
    assert 1 <= n <= 128
    return 32 if n <= 32 else 64 if n <= 64 else 128


def route(n, k, dual_max):
    """What the planner does with a row of n stored entries of an eligible sweep: ZERO, FORMED, or the class width 32 | 64 | 128."""
    if n == 0:
        return ZERO
    if n <= min(dual_max, 128) and class_width(n) < k_pad(k):
        return class_width(n)
    return FORMED


def lengths(Rx, Ry, which):
    """Stored entries per row of the sweep of factor ``which`` (every side observed)."""
    sides = A._sides(Rx, Ry, None, None, None, which)
    assert all(rel.observed for rel, _, _, _ in sides)
    return sum(rel.row_lengths(trans) for rel, trans, _, _ in sides)


def plan(Rx, Ry, which, k, dual_max):
    return [route(int(n), k, dual_max) for n in lengths(Rx, Ry, which)]


def counts(routes):
    """(rows in class 32, 64, 128, formed rows, zero rows): what cmf_als_dual_last reports."""
    return tuple(sum(1 for r in routes if r == what) for what in (32, 64, 128, FORMED, ZERO))


def _sum(terms, order, dtype):
    """sum of the rows of ``terms`` [n, ...] in float ``dtype`` in the given association."""
    terms = [np.asarray(t, dtype=dtype) for t in terms]
    if not terms:
        return None
    if order == "reverse":
        terms = terms[::-1]
    if order in ("forward", "reverse"):
        out = terms[0]
        for t in terms[1:]:
            out = (out + t).astype(dtype)
        return out
    if order == "pairs":
        while len(terms) > 1:
            terms = [(terms[i] + terms[i + 1]).astype(dtype) if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        return terms[0]
    h = (len(terms) + 1) // 2                    # halves
    a, b = _sum(terms[:h], "forward", dtype), _sum(terms[h:], "forward", dtype)
    return a if b is None else (a + b).astype(dtype)


def dual_row(Bs, ws, pvs, l2, dtype=np.float64, order=None):
    """(K, z, f) of one row.  Bs / ws / pvs: per observed side the gathered rows [n_s, k], the weights and p = w t.  ``order`` None:
    NumPy's products; otherwise the sums over k (the Gram) and over the entries (the back-product) in that association."""
    B = np.concatenate([np.asarray(b, dtype=dtype) for b in Bs])
    w = np.concatenate([np.asarray(x, dtype=dtype) for x in ws])
    p = np.concatenate([np.asarray(x, dtype=dtype) for x in pvs])
    sq = np.sqrt(w).astype(dtype)
    Am = (B * sq[:, None]).astype(dtype)
    y = np.zeros_like(p)
    y[w > 0] = (p[w > 0] / sq[w > 0]).astype(dtype)
    n = len(w)
    if order is None:
        K = (Am @ Am.T).astype(dtype)
    else:
        K = _sum([np.outer(Am[:, j], Am[:, j]) for j in range(Am.shape[1])], order, dtype)
    K = (K + dtype(l2) * np.eye(n, dtype=dtype)).astype(dtype)
    z = np.linalg.solve(K, y).astype(dtype)
    if order is None:
        f = (Am.T @ z).astype(dtype)
    else:
        f = _sum([(sq[e] * z[e]).astype(dtype) * B[e] for e in range(n)], order, dtype)
    return K, z, f


def dual_rows(Rx, Ry, U, V, Z, which, l2, dual_max, *, rows=None, dtype=np.float64, order=None, non_negative=False):
    """The rows ``rows`` (None: all) of an eligible sweep of factor ``which`` as the planner routes them: dual rows by ``dual_row``,
    rows without a stored entry zeros, every other row by ``als_yardstick.sweep`` (the formed route)."""
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], dtype=dtype)
    k = F.shape[1]
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    routes = plan(Rx, Ry, which, k, dual_max)
    obs = A._observed_sides(Rx, Ry, U, V, Z, which, 0.0, 0.0, dtype)
    out = np.zeros((len(rows), k), dtype=dtype)
    formed = [n for n, i in enumerate(rows) if routes[i] == FORMED]
    if formed:
        out[formed] = A.sweep(Rx, Ry, U, V, Z, which, l2, rows=rows[formed], dtype=dtype)
    for n, i in enumerate(rows):
        if routes[i] in (ZERO, FORMED):
            continue
        Bs, ws, pvs = [], [], []
        for B, indptr, idx, pv, e in obs:
            a, b = indptr[i], indptr[i + 1]
            Bs.append(B[idx[a:b]])
            ws.append(e[a:b])
            pvs.append(pv[a:b])
        out[n] = dual_row(Bs, ws, pvs, l2, dtype, order)[2]
    return np.maximum(out, dtype(0)) if non_negative else out


def envelope(Rx, Ry, U, V, Z, which, l2, dual_max, y64, k):
    """The largest als_yardstick.tolerance over the float32 yardstick under NumPy's products and the four summation orders."""
    tols = [A.tolerance(dual_rows(Rx, Ry, U, V, Z, which, l2, dual_max, dtype=np.float32, order=o), y64, k) for o in (None,) + ORDERS]
    return max(tols)
