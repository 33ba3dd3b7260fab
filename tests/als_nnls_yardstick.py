"""NumPy yardstick of the non-negative row solve of the ALS solver (helper of test_als_nnls_host.py / test_gpu_als_nnls.py; not
collected).  Built on als_yardstick.py: the same objective, the same systems H_i f_i = g_i, the same sweep order V, U, Z.

A swept factor in ``nn_mask`` is not solved and projected: every row runs ``sweeps`` passes of cyclic coordinate descent on

    min_{f >= 0}  1/2 f^T H_i f - g_i^T f

from the row it has.  One pass (``cd_rows``):

    r = g - H f                                  (formed anew at the start of every pass)
    for j = 0 .. k - 1:   new = max(0, f_j + r_j / H_jj);   delta = new - f_j;   f_j = new;   r -= delta H[j, :]

Each step minimises the row objective exactly along coordinate j, so the objective never rises.  A row without information (no
observed entry and no full side: H = l2 I, g = 0) is set to exact zeros, as the ALS sweep leaves it.  A swept factor outside
``nn_mask`` is solved with ``np.linalg.solve``, signed, as in als_yardstick.

``dtype=np.float64`` is the yardstick; ``dtype=np.float32`` runs the same formulas on float32 arrays and exists only to size the
tolerances of the device tests (``als_yardstick.tolerance``)."""
import numpy as np

import als_yardstick as A

U_BIT, V_BIT, Z_BIT = A.U_BIT, A.V_BIT, A.Z_BIT


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


def no_information(Rx, Ry, U, V, Z, which):
    """bool[rows]: the rows of factor ``which`` with no observed entry, when no side of the sweep is full (else all False)."""
    sides = A._sides(Rx, Ry, U, V, Z, which)
    n = {"U": U, "V": V, "Z": Z}[which].shape[0]
    if any(not rel.observed for rel, _, _ in sides):
        return np.zeros(n, dtype=bool)
    return sum(rel.row_lengths(trans) for rel, trans, _ in sides) == 0


def sweep(Rx, Ry, U, V, Z, which, l2, sweeps, non_negative=True, dtype=np.float64, chunk=64):
    """The swept copy of factor ``which``: coordinate descent from its current rows (``non_negative``) or the signed solve."""
    if not non_negative:
        return A.sweep(Rx, Ry, U, V, Z, which, l2, False, dtype, chunk)
    F = {"U": U, "V": V, "Z": Z}[which]
    out = np.empty(F.shape, dtype=dtype)
    for r0 in range(0, F.shape[0], chunk):
        rows = np.arange(r0, min(r0 + chunk, F.shape[0]))
        H, g = A.systems(Rx, Ry, U, V, Z, which, l2, rows, dtype)
        out[rows] = cd_rows(H, g, np.asarray(F, dtype=dtype)[rows], sweeps, dtype)
    out[no_information(Rx, Ry, U, V, Z, which)] = 0
    return out


def step(X, Y, Wx, Wy, U, V, Z, l2, sweeps, mask=7, nn_mask=7, dtype=np.float64):
    """One iteration V, U, Z; returns new (U, V, Z), the inputs are left alone.  X / Y may be ``Relation`` objects."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    U, V, Z = (np.array(F, dtype=dtype) for F in (U, V, Z))
    if mask & V_BIT:
        V = sweep(Rx, Ry, U, V, Z, "V", l2, sweeps, bool(nn_mask & V_BIT), dtype)
    if mask & U_BIT:
        U = sweep(Rx, Ry, U, V, Z, "U", l2, sweeps, bool(nn_mask & U_BIT), dtype)
    if mask & Z_BIT:
        Z = sweep(Rx, Ry, U, V, Z, "Z", l2, sweeps, bool(nn_mask & Z_BIT), dtype)
    return U, V, Z


def fit(X, Y, Wx, Wy, U, V, Z, max_iter, l2, sweeps, mask=7, nn_mask=7, dtype=np.float64, trace=None):
    """``max_iter`` steps (the loop of als_yardstick.fit with tol = 0); ``trace`` (a list) receives the objective after each."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    for _ in range(max_iter):
        U, V, Z = step(Rx, Ry, None, None, U, V, Z, l2, sweeps, mask, nn_mask, dtype)
        if trace is not None:
            trace.append(A.objective(Rx, Ry, None, None, U, V, Z, l2))
    return U, V, Z
