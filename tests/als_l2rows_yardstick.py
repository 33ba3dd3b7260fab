"""NumPy yardstick of the ALS solver under per-row l2 multipliers (helper of test_als_l2rows_host.py / test_gpu_als_l2rows.py; not
collected).

    minimise  (the data terms of als_yardstick.py) + l2 / 2 sum_F sum_i m_F[i] |f_i|^2,      F in {U, V, Z},  m_F > 0

Row i of a sweep of F solves the system of als_yardstick.py under lambda_i = l2 m_F[i] in place of l2.  There is no arithmetic of
its own here: for every distinct value v among a factor's multipliers, ``sweep`` calls ``als_yardstick.sweep(..., l2 = l2 v,
rows = the rows with that multiplier)`` and assembles the factor.  ``mults`` is a triple (m_U, m_V, m_Z); None for a factor means
ones.  In float32 mode lambda is the ONE float32 product float32(l2) * float32(v), as on the device."""
import numpy as np

import als_yardstick as A

NAMES = "UVZ"


def _lam(l2, v, dtype):
    return float(np.float32(l2) * np.float32(v)) if dtype is np.float32 else float(l2) * float(v)


def sweep(Rx, Ry, U, V, Z, which, l2, mult, *, rows=None, dtype=np.float64, **kw):
    """The rows ``rows`` (None = all) of the swept factor ``which`` under the multipliers ``mult`` of that factor (None: ones)."""
    F = {"U": U, "V": V, "Z": Z}[which]
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    if mult is None:
        return A.sweep(Rx, Ry, U, V, Z, which, l2, rows=rows, dtype=dtype, **kw)
    mult = np.asarray(mult, dtype=np.float64)
    assert mult.shape == (F.shape[0],) and (mult > 0).all() and np.isfinite(mult).all()
    out = np.empty((len(rows), F.shape[1]), dtype=dtype)
    for v in np.unique(mult[rows]):
        sel = np.flatnonzero(mult[rows] == v)
        out[sel] = A.sweep(Rx, Ry, U, V, Z, which, _lam(l2, v, dtype), rows=rows[sel], dtype=dtype, **kw)
    return out


def step(X, Y, Wx, Wy, U, V, Z, l2, mults, *, mask=7, nn_mask=0, nn_sweeps=0, cg_steps=0, cx=0.0, cy=0.0, dtype=np.float64):
    """One iteration V, U, Z (als_yardstick.step's order and arguments) under ``mults`` = (m_U, m_V, m_Z)."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    F = {w: np.array(M, dtype=dtype) for w, M in zip(NAMES, (U, V, Z))}
    for w, bit in (("V", A.V_BIT), ("U", A.U_BIT), ("Z", A.Z_BIT)):
        if mask & bit:
            F[w] = sweep(Rx, Ry, F["U"], F["V"], F["Z"], w, l2, mults[NAMES.index(w)], non_negative=bool(nn_mask & bit), nn_sweeps=nn_sweeps,
                         cg_steps=cg_steps, cx=cx, cy=cy, dtype=dtype)
    return F["U"], F["V"], F["Z"]


def objective(X, Y, Wx, Wy, U, V, Z, l2, mults, *, cx=0.0, cy=0.0):
    """The full objective: als_yardstick's data terms plus l2 / 2 sum_F sum_i m_F[i] |f_i|^2."""
    reg = 0.0
    for F, m in zip((U, V, Z), mults):
        sq = (np.asarray(F, np.float64) ** 2).sum(axis=1)
        reg += float(sq.sum() if m is None else (np.asarray(m, np.float64) * sq).sum())
    return A.objective(X, Y, Wx, Wy, U, V, Z, 0.0, cx=cx, cy=cy) + 0.5 * l2 * reg
