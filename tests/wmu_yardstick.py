"""Float64 restatement of the multiplicative updates of the collective model with per-entry weights on the Frobenius objective
(plain NumPy; T and W dense or SciPy sparse).  It evaluates the formulas and nothing else:

    minimise  1/2 |sqrt(Wx) .* (X - U V^T)|^2 + 1/2 |sqrt(Wy) .* (Y - V Z^T)|^2 + l1 sum(U, V, Z) + l2 / 2 (|U|^2 + |V|^2 + |Z|^2)

    V <- V .* [(Wx.*X)^T U + (Wy.*Y) Z] ./ reg((Wx.*(U V^T))^T U + (Wy.*(V Z^T)) Z, V)
    U <- U .* [(Wx.*X) V]  ./ reg((Wx.*(U V^T)) V, U)          (new V)
    Z <- Z .* [(Wy.*Y)^T V] ./ reg((Wy.*(V Z^T))^T V, Z)
    reg(den, F) = den + l1 + l2 F, then den == 0 -> EPS = 2^-23     (pycmf/cmf_solvers.py:212-228 with gamma = 1)
    E_x = sum Wx .* (X - U V^T)^2, E_y likewise;  error = alpha sqrt(E_x) + (1 - alpha) sqrt(E_y)

W = None stands for W == 1.  A SciPy sparse W restricts the sums to its stored pattern (T is read on that pattern, stored zeros of
either matrix included); a dense W of the same values gives the same sums.  With both weights None this is the reference's MU step
(pycmf/cmf_solvers.py:248-263) in another association; tests/test_wmu_host.py holds it against oracle.cmf_oracle.mu_update_step.

Tolerances of the float32 device against this yardstick (tests/test_gpu_wmu.py)
-------------------------------------------------------------------------------
``tau(k, L) = (k + 2 L + 16) 2^-24``: first-order forward bound, relative, of one updated element, for non-negative data, weights
and factors.  Every sum in the update then has non-negative terms, so no summation order can cancel and the bound holds for any
order: gamma_k for the dot product A_r . B_c under the weight, gamma_L for each of the two outer sums over the streamed dimension
(numerator and denominator; L = the longest sum of the sweep: d for U and Z, m + p for V), and at most 16 single roundings for
the rest (float32 inputs are exact; w t, w s, the products of the outer sums, the regulariser's product and two sums, the
quotient and the final product).  A full step gives U and Z ``tau_U + 3 tau_V``: the new V enters their numerator once and their
denominator twice (in s and in the outer product).

``resid_tol(k, sum_wes, E) = 2^-24 (2 (k + 2) sum w |t - s| s + 8 sum w (t - s)^2)``: the DIRECT form w (t - s)^2 with every term
in float32 and float64 accumulation.  With u = 2^-24: the device's s carries gamma_k s, the difference one rounding, so the error
of (t - s) is at most (k + 1) u s + u |t - s| to first order; squaring doubles the relative error, the square and the product
with w add a rounding each: per term at most w (2 (k + 1) u |t - s| s + 4 u (t - s)^2).  The constants above leave the second-order
terms and the float64 sum (2^-53 per addition) ample room.  The expanded form |T|^2 - 2 tr + tr would cancel and is not used.
"""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -23
U_BIT, V_BIT, Z_BIT = 1, 2, 4


def tau(k, L):
    return (k + 2 * L + 16) * 2.0 ** -24


def resid_tol(k, sum_wes, E):
    return 2.0 ** -24 * (2 * (k + 2) * sum_wes + 8 * E)


def _dense(T):
    return T.toarray().astype(np.float64) if sp.issparse(T) else np.asarray(T, np.float64)


def _pattern(T, W):
    """(rows, cols, t, w) of a SciPy sparse W: its stored pattern (duplicates summed, zeros kept) with T read on it."""
    P = sp.csr_matrix(W, dtype=np.float64, copy=True)
    P.sum_duplicates()
    r = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    c = P.indices
    t = np.asarray(T.tocsr()[r, c], np.float64).ravel() if sp.issparse(T) else np.asarray(T, np.float64)[r, c]
    return r, c, t, np.asarray(P.data, np.float64)


def products(T, W, A, B, trans=False):
    """((W.*T) B, (W.*(A B^T)) B) -- rows of A; trans: ((W.*T)^T A, (W.*(A B^T))^T A) -- rows of B."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if sp.issparse(W):
        r, c, t, w = _pattern(T, W)
        s = np.einsum("ij,ij->i", A[r], B[c])
        N = sp.csr_matrix((w * t, (r, c)), shape=W.shape)
        D = sp.csr_matrix((w * s, (r, c)), shape=W.shape)
        if trans:
            return np.asarray(N.T @ A), np.asarray(D.T @ A)
        return np.asarray(N @ B), np.asarray(D @ B)
    T = _dense(T)
    S = A @ B.T
    if W is not None:
        W = np.asarray(W, np.float64)
        T, S = W * T, W * S
    if trans:
        return T.T @ A, S.T @ A
    return T @ B, S @ B


def reg(den, F, l1, l2):
    den = np.array(den, dtype=np.float64)
    if l1 > 0:
        den = den + l1
    if l2 > 0:
        den = den + l2 * F
    den[den == 0] = EPS
    return den


def step(X, Y, Wx, Wy, U, V, Z, l1=0.0, l2=0.0, mask=7):
    """One sweep V, U, Z; returns new arrays (inputs untouched)."""
    U, V, Z = (np.array(F, dtype=np.float64) for F in (U, V, Z))
    if mask & V_BIT:
        nx, dx = products(X, Wx, U, V, trans=True)
        ny, dy = products(Y, Wy, V, Z)
        V = V * ((nx + ny) / reg(dx + dy, V, l1, l2))
    if mask & U_BIT:
        n, d = products(X, Wx, U, V)
        U = U * (n / reg(d, U, l1, l2))
    if mask & Z_BIT:
        n, d = products(Y, Wy, V, Z, trans=True)
        Z = Z * (n / reg(d, Z, l1, l2))
    return U, V, Z


def residual_terms(T, W, A, B):
    """(E = sum w (t - s)^2, sum w |t - s| s)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if sp.issparse(W):
        r, c, t, w = _pattern(T, W)
        s = np.einsum("ij,ij->i", A[r], B[c])
    else:
        t, s = _dense(T), A @ B.T
        w = np.ones_like(t) if W is None else np.asarray(W, np.float64)
    e = t - s
    return float((w * e * e).sum()), float((w * np.abs(e) * np.abs(s)).sum())


def errors(X, Y, Wx, Wy, U, V, Z):
    return np.sqrt(residual_terms(X, Wx, U, V)[0]), np.sqrt(residual_terms(Y, Wy, V, Z)[0])


def objective(X, Y, Wx, Wy, U, V, Z, l1=0.0, l2=0.0):
    return (0.5 * residual_terms(X, Wx, U, V)[0] + 0.5 * residual_terms(Y, Wy, V, Z)[0] + l1 * (U.sum() + V.sum() + Z.sum())
            + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum()))


def fit(X, Y, Wx, Wy, U, V, Z, max_iter, tol, alpha=0.5, l1=0.0, l2=0.0, mask=7):
    """The reference's loop (cmf_solvers.py:132-195): error at init, a step per iteration, every 10th iteration when tol > 0 the
    stopping test (previous - error) / error_at_init < tol.  Returns (U, V, Z, n_iter, ratios) -- ratios: the left side of the
    test at every check."""
    ex, ey = errors(X, Y, Wx, Wy, U, V, Z)
    prev = init = alpha * ex + (1 - alpha) * ey
    ratios = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        U, V, Z = step(X, Y, Wx, Wy, U, V, Z, l1, l2, mask)
        if tol > 0 and n_iter % 10 == 0:
            ex, ey = errors(X, Y, Wx, Wy, U, V, Z)
            err = alpha * ex + (1 - alpha) * ey
            ratios.append((prev - err) / init)
            if ratios[-1] < tol:
                break
            prev = err
    return U, V, Z, n_iter, ratios
