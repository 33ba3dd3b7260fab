"""NumPy yardstick of the ALS solver (helper of test_als_host.py / test_gpu_als.py; not collected).

    minimise  1/2 sum_{Ox} wx_ij (x_ij - u_i.v_j)^2 + 1/2 sum_{Oy} wy_jc (y_jc - v_j.z_c)^2 + l2/2 (|U|^2 + |V|^2 + |Z|^2),   l2 > 0

in MU's sweep order V, U, Z (pycmf/cmf_solvers.py:248-263), the new V used for U and Z.  A relation with weights W is OBSERVED: a
SciPy sparse W counts on its stored pattern (T read there, stored zeros of either included), a dense W on its non-zeros.  W = None
is FULL: every cell with weight 1, T dense or SciPy sparse.  Every row f_i of a swept factor solves its own system

    H_i f_i = g_i,    H_i = sum_{c in O_i} w_ic b_c b_c^T  +  B^T B (full side)  +  l2 I,    g_i = sum_{c in O_i} w_ic t_ic b_c + (T B)_i

with U: the X side (b = rows of V), Z: the Y side (rows of V), V: both sides (rows of U and of Z).  ``nn_mask`` projects the solved
rows, max(0, .), as the Newton solver honours ``*_non_negative`` -- exact minimisation holds without it only.

``dtype=np.float64`` is the yardstick.  ``dtype=np.float32`` runs the same formulas on float32 arrays (sums, Grams and the solve);
it exists only to size the tolerances of the device tests, by the HALS rule (hals_yardstick.py):

    tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|)      per factor

float32 normal equations lose cond(H_i) eps, which only the case at hand can price; the factor 4 covers another association of the
same sums; the floor is k + 16 roundings of the largest entry."""
import numpy as np
import scipy.sparse as sp

U_BIT, V_BIT, Z_BIT = 1, 2, 4


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


def _sides(Rx, Ry, U, V, Z, which):
    """[(relation, transposed?, gathered factor)] of the sweep of factor ``which``."""
    if which == "U":
        return [(Rx, False, V)]
    if which == "Z":
        return [(Ry, True, V)]
    return [(Rx, True, U), (Ry, False, Z)]


def systems(Rx, Ry, U, V, Z, which, l2, rows=None, dtype=np.float64):
    """(H [n, k, k], g [n, k]) of the rows ``rows`` (an index array; None = all) of the sweep of factor ``which``."""
    F = {"U": U, "V": V, "Z": Z}[which]
    k = F.shape[1]
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    H = np.zeros((len(rows), k, k), dtype=dtype)
    g = np.zeros((len(rows), k), dtype=dtype)
    for rel, trans, B in _sides(Rx, Ry, U, V, Z, which):
        B = np.asarray(B, dtype=dtype)
        if not rel.observed:
            H += (B.T @ B)[None]
            T = rel.T.T if trans else rel.T
            TB = (T.tocsr()[rows].astype(dtype) @ B) if sp.issparse(T) else np.asarray(T[rows], dtype=dtype) @ B
            g += np.asarray(TB, dtype=dtype)
            continue
        indptr, idx, t, w = rel.images[1 if trans else 0]
        for n, i in enumerate(rows):
            a, b = indptr[i], indptr[i + 1]
            if a == b:
                continue
            Bi = B[idx[a:b]]
            Bs = Bi * np.sqrt(w[a:b]).astype(dtype)[:, None]
            H[n] += Bs.T @ Bs
            g[n] += Bi.T @ (w[a:b] * t[a:b]).astype(dtype)
    H[:, np.arange(k), np.arange(k)] += dtype(l2)
    return H, g


def sweep(Rx, Ry, U, V, Z, which, l2, non_negative=False, dtype=np.float64, chunk=64):
    """The swept copy of factor ``which``."""
    F = {"U": U, "V": V, "Z": Z}[which]
    out = np.empty(F.shape, dtype=dtype)
    for r0 in range(0, F.shape[0], chunk):
        rows = np.arange(r0, min(r0 + chunk, F.shape[0]))
        H, g = systems(Rx, Ry, U, V, Z, which, l2, rows, dtype)
        out[rows] = np.linalg.solve(H, g[:, :, None])[:, :, 0]
    if non_negative:
        out = np.maximum(out, dtype(0))
    return out


def step(X, Y, Wx, Wy, U, V, Z, l2, mask=7, nn_mask=0, dtype=np.float64):
    """One iteration V, U, Z; returns new (U, V, Z), the inputs are left alone.  X / Y may be ``Relation`` objects (Wx / Wy ignored)."""
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    U, V, Z = (np.array(F, dtype=dtype) for F in (U, V, Z))
    if mask & V_BIT:
        V = sweep(Rx, Ry, U, V, Z, "V", l2, bool(nn_mask & V_BIT), dtype)
    if mask & U_BIT:
        U = sweep(Rx, Ry, U, V, Z, "U", l2, bool(nn_mask & U_BIT), dtype)
    if mask & Z_BIT:
        Z = sweep(Rx, Ry, U, V, Z, "Z", l2, bool(nn_mask & Z_BIT), dtype)
    return U, V, Z


def residual_sq(rel, A, B):
    """sum w (t - a.b)^2 over the relation (weight 1 in every cell of a full one)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if rel.observed:
        e = rel.t - np.einsum("ij,ij->i", A[rel.r], B[rel.c])
        return float((rel.w * e * e).sum())
    T = rel.T.toarray() if sp.issparse(rel.T) else rel.T
    return float(((T - A @ B.T) ** 2).sum())


def errors(X, Y, Wx, Wy, U, V, Z):
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    return np.sqrt(residual_sq(Rx, U, V)), np.sqrt(residual_sq(Ry, V, Z))


def objective(X, Y, Wx, Wy, U, V, Z, l2):
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    U, V, Z = (np.asarray(F, np.float64) for F in (U, V, Z))
    return 0.5 * residual_sq(Rx, U, V) + 0.5 * residual_sq(Ry, V, Z) + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum())


def gradient(X, Y, Wx, Wy, U, V, Z, l2, which):
    """The gradient of the objective with respect to factor ``which`` (rows x k)."""
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], np.float64)
    G = l2 * F
    for n in range(F.shape[0]):
        H, g = systems(Rx, Ry, U, V, Z, which, 0.0, [n])
        G[n] += H[0] @ F[n] - g[0]
    return G


def fit(X, Y, Wx, Wy, U, V, Z, max_iter, tol, l2, alpha=0.5, mask=7, nn_mask=0, dtype=np.float64, trace=None):
    """The reference's loop (cmf_solvers.py:132-195) with the weighted error: error at init, a step per iteration, every 10th
    iteration when tol > 0 the stopping test (previous - error) / error_at_init < tol.  Returns (U, V, Z, n_iter, ratios) -- ratios:
    the left side of the test at every check; ``trace`` (a list) receives the objective after every iteration."""
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    ex, ey = errors(Rx, Ry, None, None, U, V, Z)
    prev = init = alpha * ex + (1 - alpha) * ey
    ratios = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        U, V, Z = step(Rx, Ry, None, None, U, V, Z, l2, mask, nn_mask, dtype)
        if trace is not None:
            trace.append(objective(Rx, Ry, None, None, U, V, Z, l2))
        if tol > 0 and n_iter % 10 == 0:
            ex, ey = errors(Rx, Ry, None, None, U, V, Z)
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
