"""NumPy yardstick of the ALS solver, all of its routes (helper of test_als*_host.py / test_gpu_als*.py; not collected).

    minimise  1/2 sum_{Ox} wx_ij (x_ij - u_i.v_j)^2 + 1/2 sum_{Oy} wy_jc (y_jc - v_j.z_c)^2 + l2/2 (|U|^2 + |V|^2 + |Z|^2),   l2 > 0

in MU's sweep order V, U, Z (pycmf/cmf_solvers.py:248-263), the new V used for U and Z.  A relation with weights W is OBSERVED: a
SciPy sparse W counts on its stored pattern O (T read there, stored zeros of either included), a dense W on its non-zeros.  W = None
is FULL: every cell with weight 1, T dense or SciPy sparse.  An observed relation may carry a background weight c0 >= 0 (``cx`` for
X, ``cy`` for Y; w >= c0 on every stored entry), which adds  1/2 c0 sum_{not O} (a.b)^2  to its term: the dense weighted objective
with W = c0 and target 0 off the pattern (``dense_equivalent``), never formed here.  With the excess weights e = w - c0 every row
f_i of a swept factor has its own system

    H_i f_i = g_i,    H_i = sum_{c in O_i} e_ic b_c b_c^T + S + l2 I,      g_i = sum_{c in O_i} w_ic t_ic b_c + N_i,
    S = sum_sides coef B_side^T B_side     (coef: c0 of a side with a background, 1 of a full side; the X side first),
    N = T B of a full side

with U: the X side (b = rows of V), Z: the Y side (rows of V), V: both sides (rows of U and of Z).  The error of a relation with a
background:  E = sum_O w (t - s)^2 + c0 (<A^T A, B^T B>_F - sum_O s^2).  ``route`` names what a sweep does with its systems, as the
device's als_route does:

    exact (shared | rows)    np.linalg.solve; a factor in ``nn_mask`` is then projected, max(0, .) -- exact minimisation holds
                             without it only
    hals (shared) | nnls (rows)   ``nn_sweeps`` passes of cyclic coordinate descent from the row it has (``cd_rows``) on
                             min_{f >= 0} 1/2 f^T H_i f - g_i^T f:  r = g - H f anew at the start of every pass, then for j = 0 .. k - 1
                             new = max(0, f_j + r_j / H_jj);  delta = new - f_j;  f_j = new;  r -= delta H[j, :]
                             -- exact along coordinate j, so the row objective never rises
    cg (rows)                ``cg_steps`` steps of plain conjugate gradients from the row it has, matrix-free (``cg_row``):
                             H x = sum_e e_e b_e (b_e . x) + S x + l2 x;   r = g - H f, p = r;   per step q = H p,
                             alpha = (r.r) / (p.q), f += alpha p, r -= alpha q, beta = (r'.r') / (r.r), p = r' + beta p;
                             a row stops when r.r or p.q is not a positive finite number and keeps what it has

A row without information (no stored entry, and no side that is full or has a background: H = l2 I, g = 0) is exact zeros on every
route.

``dtype=np.float64`` is the yardstick.  ``dtype=np.float32`` runs the same formulas on float32 arrays (sums, Grams, each
coef * Gram and their sum rounded once, the solve); it exists only to size the tolerances of the device tests, by the HALS rule
(hals_yardstick.py):

    tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|)      per factor

float32 normal equations lose cond(H_i) eps, which only the case at hand can price; the factor 4 covers another association of the
same sums; the floor is k + 16 roundings of the largest entry."""
import numpy as np
import scipy.sparse as sp

U_BIT, V_BIT, Z_BIT = 1, 2, 4
SHARED_EXACT, SHARED_HALS, ROWS_EXACT, ROWS_NNLS, ROWS_CG = "shared exact", "shared hals", "rows exact", "rows nnls", "rows cg"
ROWS_NNCG, ROWS_DUAL = "rows nncg", "rows dual"


class Relation:
    """One relation in the form the sweeps read it: ``observed`` with the pattern in both orientations, or full."""

    def __init__(self, T, W):
        self.shape = T.shape
        self.observed = W is not None
        if not self.observed:
            self.T = T.tocsr().astype(np.float64) if sp.issparse(T) else np.asarray(T, np.float64)
            return
        if sp.issparse(W):
            P = sp.csr_matrix(W, dtype=np.float64, copy=True)
            P.sum_duplicates()
        else:
            P = sp.csr_matrix(np.asarray(W, np.float64))
            P.eliminate_zeros()
        P.sort_indices()
        r = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
        c = P.indices.astype(np.int64)
        t = np.asarray(T.tocsr()[r, c], np.float64).ravel() if sp.issparse(T) else np.asarray(T, np.float64)[r, c]
        w = np.asarray(P.data, np.float64)
        self.r, self.c, self.t, self.w = r, c, t, w
        order = np.lexsort((r, c))               # the transpose: by column, rows ascending inside one
        self.images = ((P.indptr.astype(np.int64), c, t, w),
                       (np.concatenate(([0], np.cumsum(np.bincount(c, minlength=P.shape[1])))).astype(np.int64), r[order], t[order], w[order]))

    def row_lengths(self, trans):
        return np.diff(self.images[1 if trans else 0][0])


def as_relation(T, W):
    return T if isinstance(T, Relation) else Relation(T, W)


def _sides(Rx, Ry, U, V, Z, which, cx=0.0, cy=0.0):
    """[(relation, transposed?, gathered factor, background of the relation)] of the sweep of factor ``which``."""
    if which == "U":
        return [(Rx, False, V, cx)]
    if which == "Z":
        return [(Ry, True, V, cy)]
    return [(Rx, True, U, cx), (Ry, False, Z, cy)]


def observed(Rx, Ry, which):
    """Does the sweep of factor ``which`` read an observed relation?"""
    return any(rel.observed for rel, _, _, _ in _sides(Rx, Ry, None, None, None, which))


def shared(Rx, Ry, U, V, Z, which, *, cx=0.0, cy=0.0, rows=None, dtype=np.float64):
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
            TB = np.asarray(T.astype(dtype) @ B, dtype=dtype)
            Nf = TB if Nf is None else Nf + TB
    return S, Nf


def _observed_sides(Rx, Ry, U, V, Z, which, cx, cy, dtype):
    """[(B, indptr, idx, pv = w t, e = w - c0)] of the observed sides of the sweep."""
    out = []
    for rel, trans, B, c0 in _sides(Rx, Ry, U, V, Z, which, cx, cy):
        if rel.observed:
            indptr, idx, t, w = rel.images[1 if trans else 0]
            w = w.astype(dtype)
            out.append((np.asarray(B, dtype=dtype), indptr, idx, (w * t.astype(dtype)).astype(dtype), (w - dtype(c0)).astype(dtype)))
    return out


def systems(Rx, Ry, U, V, Z, which, l2, *, cx=0.0, cy=0.0, rows=None, dtype=np.float64):
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
    S, Nf = shared(Rx, Ry, U, V, Z, which, cx=cx, cy=cy, rows=rows, dtype=dtype)
    if S is not None:
        H += S[None]
    if Nf is not None:
        g += Nf
    H[:, np.arange(k), np.arange(k)] += dtype(l2)
    return H, g


def no_information(Rx, Ry, U, V, Z, which, *, cx=0.0, cy=0.0):
    """bool[rows]: the rows of factor ``which`` without a stored entry, when no side of the sweep is full or has a background."""
    sides = _sides(Rx, Ry, U, V, Z, which, cx, cy)
    n = {"U": U, "V": V, "Z": Z}[which].shape[0]
    if any((not rel.observed) or c0 for rel, _, _, c0 in sides):
        return np.zeros(n, dtype=bool)
    return sum(rel.row_lengths(trans) for rel, trans, _, _ in sides) == 0


def cd_rows(H, g, F, sweeps, dtype=np.float64):
    """The swept copy of F [n, k] under the systems H [n, k, k], g [n, k]: ``sweeps`` passes, all rows at once."""
    H, g = np.asarray(H, dtype=dtype), np.asarray(g, dtype=dtype)
    F = np.array(F, dtype=dtype)
    k = F.shape[1]
    for _ in range(int(sweeps)):
        r = g - np.einsum("nij,nj->ni", H, F).astype(dtype)
        moved = False
        for j in range(k):
            new = np.maximum(dtype(0), F[:, j] + r[:, j] / H[:, j, j])
            delta = new - F[:, j]
            F[:, j] = new
            r -= delta[:, None] * H[:, j, :]
            moved = moved or bool(np.any(delta != 0))
        if not moved:
            break
    return F


def _good(v):
    return bool(v > 0) and bool(np.isfinite(v))


def cg_row(Bs, ws, pvs, S, Nrow, l2, f, cg_steps, dtype=np.float64):
    """The row after ``cg_steps`` steps.  Bs / ws / pvs: per observed side the gathered rows [n, k], the (excess) weights and
    p = w t; S [k, k] and Nrow [k] of the shared part, or None."""
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


def route(is_observed, non_negative, nn_sweeps, cg_steps, nn_cg_steps=0, dual_max=0, shared_term=False, logistic=False, k_pad=64):
    """What the sweep of one factor does (the device's als_route, the same precedence): without an observed relation all rows share
    one matrix.  The facts behind the options: the sweep has a shared term (a full relation or a background weight), reads a
    logistic relation, and k_pad -- the dual rows need an exact row sweep without either, and a class width below k_pad."""
    if is_observed and non_negative and nn_cg_steps:
        return ROWS_NNCG
    if non_negative and nn_sweeps:
        return ROWS_NNLS if is_observed else SHARED_HALS
    if not is_observed:
        return SHARED_EXACT
    if cg_steps and not non_negative:
        return ROWS_CG
    return ROWS_DUAL if dual_max > 0 and not shared_term and not logistic and k_pad > 32 else ROWS_EXACT


def sweep(Rx, Ry, U, V, Z, which, l2, *, non_negative=False, nn_sweeps=0, cg_steps=0, cx=0.0, cy=0.0, rows=None, dtype=np.float64,
          chunk=64):
    """The rows ``rows`` (an index array; None = all) of the swept factor ``which``, by the route the device gives it.  The shared
    routes are computed from the per-row systems too: the same equations."""
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], dtype=dtype)
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    how = route(observed(Rx, Ry, which), non_negative, nn_sweeps, cg_steps)
    out = np.empty((len(rows), F.shape[1]), dtype=dtype)
    if how == ROWS_CG:
        obs = _observed_sides(Rx, Ry, U, V, Z, which, cx, cy, dtype)
        S, Nf = shared(Rx, Ry, U, V, Z, which, cx=cx, cy=cy, rows=rows, dtype=dtype)
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
            out[n] = cg_row(Bs, es, pvs, S, None if Nf is None else Nf[n], l2, F[i], cg_steps, dtype)
        return out
    descend = how in (SHARED_HALS, ROWS_NNLS)
    for r0 in range(0, len(rows), chunk):
        sel = slice(r0, min(r0 + chunk, len(rows)))
        H, g = systems(Rx, Ry, U, V, Z, which, l2, cx=cx, cy=cy, rows=rows[sel], dtype=dtype)
        out[sel] = cd_rows(H, g, F[rows[sel]], nn_sweeps, dtype) if descend else np.linalg.solve(H, g[:, :, None])[:, :, 0]
    if descend:
        out[no_information(Rx, Ry, U, V, Z, which, cx=cx, cy=cy)[rows]] = 0
    return np.maximum(out, dtype(0)) if non_negative and not descend else out


def step(X, Y, Wx, Wy, U, V, Z, l2, *, mask=7, nn_mask=0, nn_sweeps=0, cg_steps=0, cx=0.0, cy=0.0, dtype=np.float64):
    """One iteration V, U, Z; returns new (U, V, Z), the inputs are left alone.  X / Y may be ``Relation`` objects (Wx / Wy ignored)."""
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    F = {w: np.array(M, dtype=dtype) for w, M in zip("UVZ", (U, V, Z))}
    for w, bit in (("V", V_BIT), ("U", U_BIT), ("Z", Z_BIT)):
        if mask & bit:
            F[w] = sweep(Rx, Ry, F["U"], F["V"], F["Z"], w, l2, non_negative=bool(nn_mask & bit), nn_sweeps=nn_sweeps, cg_steps=cg_steps,
                         cx=cx, cy=cy, dtype=dtype)
    return F["U"], F["V"], F["Z"]


def residual_sq(rel, A, B, c0=0.0):
    """E of one relation: sum w (t - a.b)^2 over it (weight 1 in every cell of a full one), plus c0 times the squared scores off the
    pattern of an observed one."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if not rel.observed:
        T = rel.T.toarray() if sp.issparse(rel.T) else rel.T
        return float(((T - A @ B.T) ** 2).sum())
    s = np.einsum("ij,ij->i", A[rel.r], B[rel.c])
    e = rel.t - s
    p = float((rel.w * e * e).sum())
    if not c0:
        return p
    return max(0.0, p + c0 * (float(((A.T @ A) * (B.T @ B)).sum()) - float((s * s).sum())))


def errors(X, Y, Wx, Wy, U, V, Z, *, cx=0.0, cy=0.0):
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    return np.sqrt(residual_sq(Rx, U, V, cx)), np.sqrt(residual_sq(Ry, V, Z, cy))


def objective(X, Y, Wx, Wy, U, V, Z, l2, *, cx=0.0, cy=0.0):
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    U, V, Z = (np.asarray(F, np.float64) for F in (U, V, Z))
    return 0.5 * residual_sq(Rx, U, V, cx) + 0.5 * residual_sq(Ry, V, Z, cy) + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum())


def gradient(X, Y, Wx, Wy, U, V, Z, l2, which, *, cx=0.0, cy=0.0):
    """The gradient of the objective with respect to factor ``which`` (rows x k)."""
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], np.float64)
    G = l2 * F
    for n in range(F.shape[0]):
        H, g = systems(Rx, Ry, U, V, Z, which, 0.0, cx=cx, cy=cy, rows=[n])
        G[n] += H[0] @ F[n] - g[0]
    return G


def fit(X, Y, Wx, Wy, U, V, Z, max_iter, l2, *, tol=0.0, alpha=0.5, mask=7, nn_mask=0, nn_sweeps=0, cg_steps=0, cx=0.0, cy=0.0,
        dtype=np.float64, trace=None):
    """The reference's loop (cmf_solvers.py:132-195) with the weighted error: error at init, a step per iteration, every 10th
    iteration when tol > 0 the stopping test (previous - error) / error_at_init < tol.  Returns (U, V, Z, n_iter, ratios) -- ratios:
    the left side of the test at every check; ``trace`` (a list) receives the objective after every iteration."""
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    ex, ey = errors(Rx, Ry, None, None, U, V, Z, cx=cx, cy=cy)
    prev = init = alpha * ex + (1 - alpha) * ey
    ratios = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        U, V, Z = step(Rx, Ry, None, None, U, V, Z, l2, mask=mask, nn_mask=nn_mask, nn_sweeps=nn_sweeps, cg_steps=cg_steps, cx=cx, cy=cy,
                       dtype=dtype)
        if trace is not None:
            trace.append(objective(Rx, Ry, None, None, U, V, Z, l2, cx=cx, cy=cy))
        if tol > 0 and n_iter % 10 == 0:
            ex, ey = errors(Rx, Ry, None, None, U, V, Z, cx=cx, cy=cy)
            err = alpha * ex + (1 - alpha) * ey
            ratios.append((prev - err) / init)
            if ratios[-1] < tol:
                break
            prev = err
    return U, V, Z, n_iter, ratios


def tolerance(y32, y64, k):
    """tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|) of one comparison (module docstring)."""
    y32, y64 = np.asarray(y32, dtype=np.float64), np.asarray(y64, dtype=np.float64)
    return max(4.0 * float(np.max(np.abs(y32 - y64))), (k + 16) * 2.0 ** -24 * float(np.max(np.abs(y64))))


def dense_equivalent(T, W, c0):
    """(D, Wd) dense: the data with zeros off the pattern of the SciPy sparse ``W``, and the weights ``c0`` everywhere with ``W`` on
    its pattern -- the dense weighted problem the background model is equal to (c0 > 0: every cell then counts as observed)."""
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
