"""NumPy yardstick of ALS with a background weight, the implicit-feedback model (helper of test_als_implicit_host.py /
test_gpu_als_implicit.py; not collected).  Built on als_yardstick.py, als_nnls_yardstick.py and als_cg_yardstick.py.

An OBSERVED relation (weights w on a stored pattern O) may carry a background weight c0 >= 0 (``cx`` for X, ``cy`` for Y), w >= c0
on every stored entry.  Its term of the objective is

    1/2 sum_O w (t - a.b)^2  +  1/2 c0 sum_{not O} (a.b)^2

-- the dense weighted objective with W = c0 and target 0 off the pattern (``dense_equivalent``).  This file never forms that dense
matrix.  With the excess weights e = w - c0 the system of a row is

    H_i = sum_{c in O_i} e_ic b_c b_c^T + S + l2 I,      g_i = sum_{c in O_i} w_ic t_ic b_c + N_i,
    S   = sum_sides coef B_side^T B_side     (coef: c0 of a side with a background, 1 of a full side; the X side first),
    N   = T B of a full side,

and the error of the relation  E = sum_O w (t - s)^2 + c0 (<A^T A, B^T B>_F - sum_O s^2).  A row without stored entries on a side
with a background is an ordinary row: S gives it a system.  The routes of a sweep are the ones of the device: a factor whose
relations are all full goes to the yardsticks this file is built on; otherwise a factor in ``nn_mask`` is projected
(``nn_sweeps = 0``) or swept by coordinate descent (``als_nnls_yardstick.cd_rows``), a signed one is solved exactly or
(``cg_steps > 0``) runs conjugate gradients (``als_cg_yardstick.cg_row`` with S and the excess weights).

``dtype=np.float64`` is the yardstick; ``dtype=np.float32`` runs the same formulas on float32 arrays (each coef * Gram and their
sum rounded once, as the device rounds them) and exists only to size the tolerances of the device tests
(``als_yardstick.tolerance``)."""
import numpy as np
import scipy.sparse as sp

import als_cg_yardstick as C
import als_nnls_yardstick as N
import als_yardstick as A

U_BIT, V_BIT, Z_BIT = A.U_BIT, A.V_BIT, A.Z_BIT
tolerance = A.tolerance


def _sides(Rx, Ry, U, V, Z, which, cx, cy):
    """[(relation, transposed?, gathered factor, background of the relation)] of the sweep of factor ``which``."""
    if which == "U":
        return [(Rx, False, V, cx)]
    if which == "Z":
        return [(Ry, True, V, cy)]
    return [(Rx, True, U, cx), (Ry, False, Z, cy)]


def shared(Rx, Ry, U, V, Z, which, cx, cy, rows=None, dtype=np.float64):
    """(S [k, k] or None, N [len(rows), k] or None) of the sweep of factor ``which``."""
    S = Nf = None
    for rel, trans, B, c0 in _sides(Rx, Ry, U, V, Z, which, cx, cy):
        B = np.asarray(B, dtype=dtype)
        if rel.observed and not c0:
            continue
        G = (dtype(c0 if rel.observed else 1.0) * (B.T @ B).astype(dtype)).astype(dtype)
        S = G if S is None else (S + G).astype(dtype)
        if not rel.observed:
            T = rel.T.T if trans else rel.T
            T = T.tocsr() if sp.issparse(T) else np.asarray(T)
            T = T if rows is None else T[rows]
            Nf = np.asarray(T.astype(dtype) @ B, dtype=dtype)
    return S, Nf


def _observed_sides(Rx, Ry, U, V, Z, which, cx, cy, dtype):
    """[(B, indptr, idx, pv = w t, e = w - c0)] of the observed sides of the sweep."""
    out = []
    for rel, trans, B, c0 in _sides(Rx, Ry, U, V, Z, which, cx, cy):
        if rel.observed:
            indptr, idx, t, w = rel.images[1 if trans else 0]
            w32 = w.astype(dtype)
            out.append((np.asarray(B, dtype=dtype), indptr, idx, (w32 * t.astype(dtype)).astype(dtype), (w32 - dtype(c0)).astype(dtype)))
    return out


def systems(Rx, Ry, U, V, Z, which, l2, cx=0.0, cy=0.0, rows=None, dtype=np.float64):
    """(H [n, k, k], g [n, k]) of the rows ``rows`` (an index array; None = all) of the sweep of factor ``which``."""
    F = {"U": U, "V": V, "Z": Z}[which]
    k = F.shape[1]
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    H = np.zeros((len(rows), k, k), dtype=dtype)
    g = np.zeros((len(rows), k), dtype=dtype)
    for B, indptr, idx, pv, e in _observed_sides(Rx, Ry, U, V, Z, which, cx, cy, dtype):
        for n, i in enumerate(rows):
            a, b = indptr[i], indptr[i + 1]
            if a == b:
                continue
            Bi = B[idx[a:b]]
            Bs = Bi * np.sqrt(e[a:b]).astype(dtype)[:, None]
            H[n] += Bs.T @ Bs
            g[n] += Bi.T @ pv[a:b]
    S, Nf = shared(Rx, Ry, U, V, Z, which, cx, cy, rows, dtype)
    if S is not None:
        H += S[None]
    if Nf is not None:
        g += Nf
    H[:, np.arange(k), np.arange(k)] += dtype(l2)
    return H, g


def observed(Rx, Ry, which):
    return C.observed(Rx, Ry, which)


def no_information(Rx, Ry, U, V, Z, which, cx, cy):
    """bool[rows]: the rows of factor ``which`` without a stored entry, when no side of the sweep is full or has a background."""
    sides = _sides(Rx, Ry, U, V, Z, which, cx, cy)
    n = {"U": U, "V": V, "Z": Z}[which].shape[0]
    if any((not rel.observed) or c0 for rel, _, _, c0 in sides):
        return np.zeros(n, dtype=bool)
    return sum(rel.row_lengths(trans) for rel, trans, _, _ in sides) == 0


def exact_sweep(Rx, Ry, U, V, Z, which, l2, cx=0.0, cy=0.0, non_negative=False, rows=None, dtype=np.float64, chunk=64):
    F = {"U": U, "V": V, "Z": Z}[which]
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    out = np.empty((len(rows), F.shape[1]), dtype=dtype)
    for r0 in range(0, len(rows), chunk):
        sel = slice(r0, min(r0 + chunk, len(rows)))
        H, g = systems(Rx, Ry, U, V, Z, which, l2, cx, cy, rows[sel], dtype)
        out[sel] = np.linalg.solve(H, g[:, :, None])[:, :, 0]
    return np.maximum(out, dtype(0)) if non_negative else out


def nnls_sweep(Rx, Ry, U, V, Z, which, l2, sweeps, cx=0.0, cy=0.0, dtype=np.float64, chunk=64):
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], dtype=dtype)
    out = np.empty(F.shape, dtype=dtype)
    for r0 in range(0, F.shape[0], chunk):
        rows = np.arange(r0, min(r0 + chunk, F.shape[0]))
        H, g = systems(Rx, Ry, U, V, Z, which, l2, cx, cy, rows, dtype)
        out[rows] = N.cd_rows(H, g, F[rows], sweeps, dtype)
    out[no_information(Rx, Ry, U, V, Z, which, cx, cy)] = 0
    return out


def cg_sweep(Rx, Ry, U, V, Z, which, l2, cg_steps, cx=0.0, cy=0.0, rows=None, dtype=np.float64):
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], dtype=dtype)
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    obs = _observed_sides(Rx, Ry, U, V, Z, which, cx, cy, dtype)
    S, Nf = shared(Rx, Ry, U, V, Z, which, cx, cy, rows, dtype)
    out = np.empty((len(rows), F.shape[1]), dtype=dtype)
    for n, i in enumerate(rows):
        Bs, es, pvs = [], [], []
        for B, indptr, idx, pv, e in obs:
            a, b = indptr[i], indptr[i + 1]
            Bs.append(B[idx[a:b]])
            es.append(e[a:b])
            pvs.append(pv[a:b])
        if S is None and sum(len(e) for e in es) == 0:
            out[n] = 0
            continue
        out[n] = C.cg_row(Bs, es, pvs, S, None if Nf is None else Nf[n], l2, F[i], cg_steps, dtype)
    return out


def sweep(Rx, Ry, U, V, Z, which, l2, cx=0.0, cy=0.0, non_negative=False, nn_sweeps=0, cg_steps=0, dtype=np.float64):
    """The swept copy of factor ``which`` by the route the device gives it."""
    if not observed(Rx, Ry, which):
        if non_negative and nn_sweeps:
            return N.sweep(Rx, Ry, U, V, Z, which, l2, nn_sweeps, True, dtype)
        return A.sweep(Rx, Ry, U, V, Z, which, l2, non_negative, dtype)
    if non_negative and nn_sweeps:
        return nnls_sweep(Rx, Ry, U, V, Z, which, l2, nn_sweeps, cx, cy, dtype)
    if not non_negative and cg_steps:
        return cg_sweep(Rx, Ry, U, V, Z, which, l2, cg_steps, cx, cy, None, dtype)
    return exact_sweep(Rx, Ry, U, V, Z, which, l2, cx, cy, non_negative, None, dtype)


def step(X, Y, Wx, Wy, U, V, Z, l2, cx=0.0, cy=0.0, mask=7, nn_mask=0, nn_sweeps=0, cg_steps=0, dtype=np.float64):
    """One iteration V, U, Z; returns new (U, V, Z), the inputs are left alone.  X / Y may be ``als_yardstick.Relation`` objects."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    U, V, Z = (np.array(F, dtype=dtype) for F in (U, V, Z))
    if mask & V_BIT:
        V = sweep(Rx, Ry, U, V, Z, "V", l2, cx, cy, bool(nn_mask & V_BIT), nn_sweeps, cg_steps, dtype)
    if mask & U_BIT:
        U = sweep(Rx, Ry, U, V, Z, "U", l2, cx, cy, bool(nn_mask & U_BIT), nn_sweeps, cg_steps, dtype)
    if mask & Z_BIT:
        Z = sweep(Rx, Ry, U, V, Z, "Z", l2, cx, cy, bool(nn_mask & Z_BIT), nn_sweeps, cg_steps, dtype)
    return U, V, Z


def residual_parts(rel, Af, Bf):
    """(sum_O w (t - s)^2, sum_O s^2, <A^T A, B^T B>_F) of an observed relation."""
    Af, Bf = np.asarray(Af, np.float64), np.asarray(Bf, np.float64)
    s = np.einsum("ij,ij->i", Af[rel.r], Bf[rel.c])
    e = rel.t - s
    return float((rel.w * e * e).sum()), float((s * s).sum()), float(((Af.T @ Af) * (Bf.T @ Bf)).sum())


def residual_sq(rel, Af, Bf, c0=0.0):
    """E of one relation: over the pattern, plus c0 times the squared scores off it."""
    if not rel.observed or not c0:
        return A.residual_sq(rel, Af, Bf)
    p, q, d = residual_parts(rel, Af, Bf)
    return max(0.0, p + c0 * (d - q))


def errors(X, Y, Wx, Wy, U, V, Z, cx=0.0, cy=0.0):
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    return np.sqrt(residual_sq(Rx, U, V, cx)), np.sqrt(residual_sq(Ry, V, Z, cy))


def objective(X, Y, Wx, Wy, U, V, Z, l2, cx=0.0, cy=0.0):
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    U, V, Z = (np.asarray(F, np.float64) for F in (U, V, Z))
    return 0.5 * residual_sq(Rx, U, V, cx) + 0.5 * residual_sq(Ry, V, Z, cy) + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum())


def fit(X, Y, Wx, Wy, U, V, Z, max_iter, tol, l2, cx=0.0, cy=0.0, alpha=0.5, mask=7, nn_mask=0, nn_sweeps=0, cg_steps=0, dtype=np.float64,
        trace=None):
    """The loop of ``als_yardstick.fit`` with this file's step and error.  Returns (U, V, Z, n_iter, ratios)."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    ex, ey = errors(Rx, Ry, None, None, U, V, Z, cx, cy)
    prev = init = alpha * ex + (1 - alpha) * ey
    ratios = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        U, V, Z = step(Rx, Ry, None, None, U, V, Z, l2, cx, cy, mask, nn_mask, nn_sweeps, cg_steps, dtype)
        if trace is not None:
            trace.append(objective(Rx, Ry, None, None, U, V, Z, l2, cx, cy))
        if tol > 0 and n_iter % 10 == 0:
            ex, ey = errors(Rx, Ry, None, None, U, V, Z, cx, cy)
            err = alpha * ex + (1 - alpha) * ey
            ratios.append((prev - err) / init)
            if ratios[-1] < tol:
                break
            prev = err
    return U, V, Z, n_iter, ratios


def dense_equivalent(T, W, c0):
    """(D, Wd) dense: the data with zeros off the pattern of the SciPy sparse ``W``, and the weights ``c0`` everywhere with ``W`` on
    its pattern -- the dense weighted problem the background model is equal to (c0 > 0: ``als_yardstick`` then counts every cell)."""
    P = sp.csr_matrix(W, dtype=np.float64, copy=True)
    P.sum_duplicates()
    P.sort_indices()
    r = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    c = P.indices
    Td = T.toarray() if sp.issparse(T) else np.asarray(T, np.float64)
    D = np.zeros(P.shape)
    D[r, c] = np.asarray(Td)[r, c]
    Wd = np.full(P.shape, float(c0))
    Wd[r, c] = P.data
    return D, Wd


# ------------------------------------------------------------------ the planted click problem
def clicks(seed, m=120, d=150, p=20, kt=3, dens=0.08, hold=0.25, k=8):
    r = np.random.RandomState(seed)
    Ut, Vt, Zt = r.randn(m, kt), r.randn(d, kt), r.randn(p, kt)
    pop = 0.8 * r.randn(d)
    S = Ut @ Vt.T + pop[None]
    thr = np.quantile(S + 0.5 * r.randn(m, d), 1 - dens)
    on = (S + 0.5 * r.randn(m, d)) > thr
    counts = on * (1 + r.poisson(np.maximum(0, 2 * (S - S.mean()))))
    _ = Vt @ Zt.T + 0.1 * r.randn(d, p)          # drawn and discarded: keeps the stream
    test = on & (r.rand(m, d) < hold); train = on & ~test
    Y = r.randn(d, p)                             # side information without signal
    U0, V0, Z0 = (0.1 * r.randn(n, k) for n in (m, d, p))
    return counts, train, test, Y, U0, V0, Z0


def recall_at(scores, train, test, n=10):
    """Mean over the rows with held-out clicks of (held-out clicks among the top n) / (held-out clicks); training cells are
    excluded, ties go to the smaller index."""
    sc = np.where(train, -np.inf, np.asarray(scores, np.float64))
    top = np.argsort(-sc, axis=1, kind="stable")[:, :n]
    hits = np.take_along_axis(test, top, axis=1).sum(axis=1)
    held = test.sum(axis=1)
    rows = held > 0
    return float((hits[rows] / held[rows]).mean())


def click_relations(counts, train):
    """(P, W): targets 1 and confidences 1 + count on the training clicks, SciPy CSR."""
    P = sp.csr_matrix(train.astype(np.float64))
    W = sp.csr_matrix(np.where(train, 1.0 + counts, 0.0))
    return P, W
