"""NumPy yardstick of the conjugate-gradient row solve of the ALS solver (helper of test_als_cg_host.py / test_gpu_als_cg.py; not
collected).  Built on als_yardstick.py: the same objective, the same systems H_i f_i = g_i, the same sweep order V, U, Z.

A swept factor that is SIGNED and has an OBSERVED relation is not solved: every row runs ``cg_steps`` steps of plain conjugate
gradients from the row it has, matrix-free (``cg_row``):

    H x = sum_{e in O_i} w_e b_e (b_e . x) + S x + l2 x,       g = sum_{e in O_i} w_e t_e b_e + N_i       (S = B^T B, N = T B: a full side)
    r = g - H f,   p = r
    per step:   q = H p;   alpha = (r.r) / (p.q);   f += alpha p;   r -= alpha q;   beta = (r'.r') / (r.r);   p = r' + beta p

A row stops when r.r or p.q is not a positive finite number and keeps what it has.  A row without information (no stored entry
and no full side) is set to exact zeros.  Every other swept factor takes the route it has without the keyword: a factor in
``nn_mask`` the projection (``nn_sweeps = 0``, als_yardstick) or coordinate descent (``nn_sweeps > 0``, als_nnls_yardstick), a
signed factor whose relations are all full the exact solve.

``dtype=np.float64`` is the yardstick; ``dtype=np.float32`` runs the same formulas on float32 arrays and exists only to size the
tolerances of the device tests (``als_yardstick.tolerance``)."""
import numpy as np
import scipy.sparse as sp

import als_nnls_yardstick as N
import als_yardstick as A

U_BIT, V_BIT, Z_BIT = A.U_BIT, A.V_BIT, A.Z_BIT


def _good(v):
    return bool(v > 0) and bool(np.isfinite(v))


def cg_row(Bs, ws, pvs, S, Nrow, l2, f, cg_steps, dtype=np.float64):
    """The row after ``cg_steps`` steps.  Bs / ws / pvs: per observed side the gathered rows [n, k], the weights and p = w t;
    S [k, k] and Nrow [k] of the full side, or None."""
    f = np.array(f, dtype=dtype)
    l2 = dtype(l2)

    def times(x):
        out = l2 * x
        for B, w in zip(Bs, ws):
            out = out + B.T @ (w * (B @ x))
        if S is not None:
            out = out + S @ x
        return out.astype(dtype)
    g = np.zeros_like(f)
    for B, pv in zip(Bs, pvs):
        g = g + B.T @ pv
    if Nrow is not None:
        g = g + Nrow
    r = (g - times(f)).astype(dtype)
    p = r.copy()
    rr = r @ r
    for _ in range(int(cg_steps)):
        if not _good(rr):
            break
        q = times(p)
        pq = p @ q
        if not _good(pq):
            break
        alpha = dtype(rr / pq)
        f = (f + alpha * p).astype(dtype)
        r = (r - alpha * q).astype(dtype)
        rn = r @ r
        p = (r + dtype(rn / rr) * p).astype(dtype)
        rr = rn
    return f


def observed(Rx, Ry, which):
    """Does the sweep of factor ``which`` read an observed relation?"""
    return any(rel.observed for rel, _, _ in A._sides(Rx, Ry, None, None, None, which))


def sweep_rows(Rx, Ry, U, V, Z, which, l2, cg_steps, rows=None, dtype=np.float64):
    """The rows ``rows`` (None = all) of factor ``which`` after ``cg_steps`` CG steps each."""
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], dtype=dtype)
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    sides = A._sides(Rx, Ry, U, V, Z, which)
    S = Nfull = None
    obs = []
    for rel, trans, B in sides:
        B = np.asarray(B, dtype=dtype)
        if rel.observed:
            indptr, idx, t, w = rel.images[1 if trans else 0]
            obs.append((B, indptr, idx, (w * t).astype(dtype), w.astype(dtype)))
            continue
        S = (B.T @ B).astype(dtype)
        T = rel.T.T if trans else rel.T
        Nfull = np.asarray((T.tocsr().astype(dtype) @ B) if sp.issparse(T) else np.asarray(T, dtype=dtype) @ B, dtype=dtype)
    out = np.empty((len(rows), F.shape[1]), dtype=dtype)
    for n, i in enumerate(rows):
        Bs, ws, pvs = [], [], []
        for B, indptr, idx, pv, w in obs:
            a, b = indptr[i], indptr[i + 1]
            Bs.append(B[idx[a:b]])
            ws.append(w[a:b])
            pvs.append(pv[a:b])
        if S is None and sum(len(w) for w in ws) == 0:
            out[n] = 0
            continue
        out[n] = cg_row(Bs, ws, pvs, S, None if Nfull is None else Nfull[i], l2, F[i], cg_steps, dtype)
    return out


def sweep(Rx, Ry, U, V, Z, which, l2, cg_steps, non_negative=False, nn_sweeps=0, dtype=np.float64):
    """The swept copy of factor ``which`` by the route ``cmf_als_cg_step`` gives it."""
    if non_negative:
        if nn_sweeps:
            return N.sweep(Rx, Ry, U, V, Z, which, l2, nn_sweeps, True, dtype)
        return A.sweep(Rx, Ry, U, V, Z, which, l2, True, dtype)
    if not cg_steps or not observed(Rx, Ry, which):
        return A.sweep(Rx, Ry, U, V, Z, which, l2, False, dtype)
    return sweep_rows(Rx, Ry, U, V, Z, which, l2, cg_steps, None, dtype)


def step(X, Y, Wx, Wy, U, V, Z, l2, cg_steps, mask=7, nn_mask=0, nn_sweeps=0, dtype=np.float64):
    """One iteration V, U, Z; returns new (U, V, Z), the inputs are left alone.  X / Y may be ``Relation`` objects."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    U, V, Z = (np.array(F, dtype=dtype) for F in (U, V, Z))
    if mask & V_BIT:
        V = sweep(Rx, Ry, U, V, Z, "V", l2, cg_steps, bool(nn_mask & V_BIT), nn_sweeps, dtype)
    if mask & U_BIT:
        U = sweep(Rx, Ry, U, V, Z, "U", l2, cg_steps, bool(nn_mask & U_BIT), nn_sweeps, dtype)
    if mask & Z_BIT:
        Z = sweep(Rx, Ry, U, V, Z, "Z", l2, cg_steps, bool(nn_mask & Z_BIT), nn_sweeps, dtype)
    return U, V, Z


def fit(X, Y, Wx, Wy, U, V, Z, max_iter, l2, cg_steps, mask=7, nn_mask=0, nn_sweeps=0, dtype=np.float64, trace=None):
    """``max_iter`` steps (the loop of als_yardstick.fit with tol = 0); ``trace`` (a list) receives the objective after each."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    for _ in range(max_iter):
        U, V, Z = step(Rx, Ry, None, None, U, V, Z, l2, cg_steps, mask, nn_mask, nn_sweeps, dtype)
        if trace is not None:
            trace.append(A.objective(Rx, Ry, None, None, U, V, Z, l2))
    return U, V, Z
