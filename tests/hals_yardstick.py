"""NumPy yardstick of the HALS solver (helper of test_hals_host.py / test_gpu_hals.py; not collected).

One sweep of a factor F (rows x k) with numerator N and Gram G, every row f on its own:

    for j = 0 .. k - 1:   h = G[j, j] + l2;   h == 0: f[j] stays
                          f[j] <- max(0, f[j] - (sum_l f[l] G[l, j] + l2 f[j] - N[j] + l1) / h)      (l < j: already updated)

-- sklearn's ``_update_coordinate_descent`` without shuffling.  A step runs the sweeps in the reference's MU order V, U, Z
(pycmf/cmf_solvers.py:248-263) with  V: N = X^T U + Y Z, G = U^T U + Z^T Z;  U: N = X V, G = V^T V;  Z: N = Y^T V, G = V^T V.

``dtype=np.float64`` is the yardstick.  ``dtype=np.float32`` runs the same formulas on float32 arrays (N and G formed in float32
too); it exists only to size the tolerances of the device tests:

    tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|)

the float32 yardstick shows what float32 arithmetic costs on the case at hand (the recurrence amplifies rounding with cond(G)); the
factor 4 covers another association of the same sums; the floor is k + 16 roundings of the largest entry."""
import numpy as np

U_BIT, V_BIT, Z_BIT = 1, 2, 4


def hals_sweep(F, N, G, l1=0.0, l2=0.0, dtype=np.float64, jacobi=False, unclipped=None):
    """The swept copy of F.  ``jacobi``: every coordinate from the OLD f (the wrong order; the tests show they can tell).
    ``unclipped`` (array like F, optional): receives the value of every coordinate before its max(0, .)."""
    F = np.array(F, dtype=dtype)
    N, G = np.asarray(N, dtype=dtype), np.asarray(G, dtype=dtype)
    l1, l2 = dtype(l1), dtype(l2)
    old = F.copy()
    for j in range(F.shape[1]):
        h = G[j, j] + l2
        if h == 0:
            if unclipped is not None:
                unclipped[:, j] = F[:, j]
            continue
        src = old if jacobi else F
        grad = src @ G[:, j] + l2 * src[:, j] - N[:, j] + l1
        raw = src[:, j] - grad / h
        if unclipped is not None:
            unclipped[:, j] = raw
        F[:, j] = np.maximum(dtype(0), raw)
    return F


def _mm(A, B, dtype):
    """A @ B in ``dtype`` (A may be SciPy sparse)."""
    if hasattr(A, "tocsr"):
        return np.asarray(A.astype(dtype) @ np.asarray(B, dtype=dtype), dtype=dtype)
    return np.asarray(A, dtype=dtype) @ np.asarray(B, dtype=dtype)


def products(X, Y, U, V, Z, which, dtype=np.float64):
    """(N, G) of the sweep of factor ``which`` ('U' | 'V' | 'Z')."""
    U, V, Z = (np.asarray(F, dtype=dtype) for F in (U, V, Z))
    if which == "V":
        return _mm(X.T, U, dtype) + _mm(Y, Z, dtype), U.T @ U + Z.T @ Z
    if which == "U":
        return _mm(X, V, dtype), V.T @ V
    return _mm(Y.T, V, dtype), V.T @ V


def hals_step(X, Y, U, V, Z, l1=0.0, l2=0.0, mask=7, dtype=np.float64, unclipped=None):
    """One iteration V, U, Z; returns new (U, V, Z), the inputs are left alone.  ``unclipped`` (a dict, optional): receives under
    'U' / 'V' / 'Z' the value of every coordinate of a swept factor before its max(0, .), as ``hals_sweep`` reports it."""
    U, V, Z = (np.array(F, dtype=dtype) for F in (U, V, Z))

    def raw(name, F):
        if unclipped is None:
            return None
        unclipped[name] = np.empty(F.shape, dtype=dtype)
        return unclipped[name]
    if mask & V_BIT:
        V = hals_sweep(V, *products(X, Y, U, V, Z, "V", dtype), l1, l2, dtype, unclipped=raw("V", V))
    if mask & U_BIT:
        U = hals_sweep(U, *products(X, Y, U, V, Z, "U", dtype), l1, l2, dtype, unclipped=raw("U", U))
    if mask & Z_BIT:
        Z = hals_sweep(Z, *products(X, Y, U, V, Z, "Z", dtype), l1, l2, dtype, unclipped=raw("Z", Z))
    return U, V, Z


def error(X, Y, U, V, Z, alpha=0.5):
    """alpha |X - U V^T|_F + (1 - alpha) |Y - V Z^T|_F (pycmf/cmf_solvers.py:128-130, linear links)."""
    X = X.toarray() if hasattr(X, "toarray") else np.asarray(X, dtype=np.float64)
    Y = Y.toarray() if hasattr(Y, "toarray") else np.asarray(Y, dtype=np.float64)
    return alpha * np.linalg.norm(X - U @ V.T) + (1 - alpha) * np.linalg.norm(Y - V @ Z.T)


def objective(X, Y, U, V, Z, l1=0.0, l2=0.0):
    return (0.5 * np.linalg.norm(X - U @ V.T) ** 2 + 0.5 * np.linalg.norm(Y - V @ Z.T) ** 2 + l1 * (U.sum() + V.sum() + Z.sum())
            + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum()))


def hals_fit(X, Y, U, V, Z, l1=0.0, l2=0.0, mask=7, max_iter=200, tol=1e-4, alpha=0.5, dtype=np.float64, trace=None):
    """The reference loop (pycmf/cmf_solvers.py:132-195) around hals_step: the error at init, a check every 10th iteration when
    tol > 0, stop when (previous - error) / error_at_init < tol.  Returns (U, V, Z, n_iter); ``trace`` (a list) receives
    (n_iter, error, (previous - error) / error_at_init) of every check."""
    previous = at_init = error(X, Y, U, V, Z, alpha)
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        U, V, Z = hals_step(X, Y, U, V, Z, l1, l2, mask, dtype)
        if tol > 0 and n_iter % 10 == 0:
            e = error(X, Y, *(np.asarray(F, dtype=np.float64) for F in (U, V, Z)), alpha)
            if trace is not None:
                trace.append((n_iter, e, (previous - e) / at_init))
            if (previous - e) / at_init < tol:
                break
            previous = e
    return U, V, Z, n_iter


def tolerance(y32, y64, k):
    """tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|) of one comparison (module docstring)."""
    y32, y64 = np.asarray(y32, dtype=np.float64), np.asarray(y64, dtype=np.float64)
    return max(4.0 * float(np.max(np.abs(y32 - y64))), (k + 16) * 2.0 ** -24 * float(np.max(np.abs(y64))))


def planted(m=300, d=240, p=40, rank=12, noise=0.05, seed=0, k=None, start_seed=1):
    """The planted non-negative problem of DESIGN section 14: X = Ut Vt^T + noise |N|, Y = Vt Zt^T + noise |N|, starts |N(0,1)|."""
    r = np.random.RandomState(seed)
    Ut, Vt, Zt = (np.abs(r.randn(n, rank)) for n in (m, d, p))
    X = Ut @ Vt.T + noise * np.abs(r.randn(m, d))
    Y = Vt @ Zt.T + noise * np.abs(r.randn(d, p))
    r = np.random.RandomState(start_seed)
    k = rank if k is None else k
    U, V, Z = (np.abs(r.randn(n, k)) for n in (m, d, p))
    return X, Y, U, V, Z
