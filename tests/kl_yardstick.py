"""Float64 restatement of the Kullback-Leibler multiplicative updates of the collective model (plain NumPy; T dense or SciPy
sparse).  It evaluates the formulas and nothing else:

    EPS = 2^-23,  Q(T, A, B) = T ./ max(A B^T, EPS)      (a zero of T gives an exact 0; nothing is divided by 0)
    V <- V .* [Q(X,U,V)^T U + Q(Y,V,Z) Z] ./ reg(colsum U + colsum Z, V)
    U <- U .* [Q(X,U,V) V]   ./ reg(colsum V, U)          (new V)
    Z <- Z .* [Q(Y,V,Z)^T V] ./ reg(colsum V, Z)
    reg(den, F) = den + l1 + l2 F, then den == 0 -> EPS
    D(T || S) = sum_{t > 0} t log(t / s) - sum t + sum s  (s = 0 under a positive t counts as EPS, as in sklearn's _beta_divergence)
    error = alpha sqrt(2 D_x) + (1 - alpha) sqrt(2 D_y)

This is sklearn's ``_multiplicative_update_w`` / ``_h`` with beta_loss = 1 applied to each block, in the reference's sweep
order V, U, Z (pycmf/cmf_solvers.py:248-263); tests/test_kl_host.py holds it against sklearn.

Tolerances of the float32 device against this yardstick (tests/test_gpu_kl.py)
------------------------------------------------------------------------------
``tau(k, L) = (k + 2 L + 16) 2^-24``: first-order forward bound, relative, of one updated element.  Every sum in the update has
non-negative terms, so no summation order can cancel and the bound holds for any order: gamma_k for the dot product under the
quotient, gamma_L for the outer sum over the streamed dimension, gamma_L for the column sum in the denominator (L = the longest
sum of the sweep: d for U and Z, m + p for V), and 16 single roundings for the rest (float32 inputs are exact; the products,
the max, two 1-ulp reciprocals counted twice, the regulariser, the final quotient and product).
A full step gives U and Z ``tau_U + 3 tau_V``: the error of the new V enters their S, their outer product and their column sum.
``div_tol(k, st, ss, sl) = (k + 16) 2^-24 (sum t + sum s + sum t |log(t / s)|)``: float32 per element (gamma_k on s, a handful
of roundings on the three terms), float64 accumulation.
"""
import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -23
U_BIT, V_BIT, Z_BIT = 1, 2, 4


def tau(k, L):
    return (k + 2 * L + 16) * 2.0 ** -24


def div_tol(k, sum_t, sum_s, sum_tlog):
    return (k + 16) * 2.0 ** -24 * (sum_t + sum_s + sum_tlog)


def _stored(T):
    T = sp.coo_matrix(T)
    return T.row, T.col, np.asarray(T.data, dtype=np.float64)


def numerator(T, A, B):
    """Q(T, A, B) B  (rows of A)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if sp.issparse(T):
        r, c, t = _stored(T)
        s = np.maximum(np.einsum("ij,ij->i", A[r], B[c]), EPS)
        Q = sp.csr_matrix((t / s, (r, c)), shape=T.shape)
        return np.asarray(Q @ B)
    T = np.asarray(T, np.float64)
    return (T / np.maximum(A @ B.T, EPS)) @ B


def numerator_t(T, A, B):
    """Q(T, A, B)^T A  (rows of B)."""
    return numerator(T.T.tocsr() if sp.issparse(T) else np.asarray(T).T, B, A)


def reg(den, F, l1, l2):
    den = np.broadcast_to(den, F.shape).astype(np.float64)
    if l1 > 0:
        den = den + l1
    if l2 > 0:
        den = den + l2 * F
    den = np.array(den)
    den[den == 0] = EPS
    return den


def step(X, Y, U, V, Z, l1=0.0, l2=0.0, mask=7):
    """One sweep V, U, Z; returns new arrays (inputs untouched)."""
    U, V, Z = (np.array(F, dtype=np.float64) for F in (U, V, Z))
    if mask & V_BIT:
        num = numerator_t(X, U, V) + numerator(Y, V, Z)
        V = V * (num / reg(U.sum(axis=0) + Z.sum(axis=0), V, l1, l2))
    if mask & U_BIT:
        U = U * (numerator(X, U, V) / reg(V.sum(axis=0), U, l1, l2))
    if mask & Z_BIT:
        Z = Z * (numerator_t(Y, V, Z) / reg(V.sum(axis=0), Z, l1, l2))
    return U, V, Z


def divergence_terms(T, A, B):
    """(sum t, sum s, sum t log(t / s) over t > 0, sum t |log(t / s)|)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if sp.issparse(T):
        r, c, t = _stored(T)
        s_nz = np.einsum("ij,ij->i", A[r], B[c])
        sum_s = float(A.sum(axis=0) @ B.sum(axis=0))
    else:
        T = np.asarray(T, np.float64)
        S = A @ B.T
        t, s_nz = T.ravel(), S.ravel()
        sum_s = float(S.sum())
    pos = t > 0
    t, s_nz = t[pos], np.array(s_nz[pos])
    s_nz[s_nz <= 0] = EPS
    lg = t * np.log(t / s_nz)
    return float(t.sum()), sum_s, float(lg.sum()), float(np.abs(lg).sum())


def divergence(T, A, B):
    st, ss, sl, _ = divergence_terms(T, A, B)
    return sl - st + ss


def errors(X, Y, U, V, Z):
    return np.sqrt(2 * max(divergence(X, U, V), 0.0)), np.sqrt(2 * max(divergence(Y, V, Z), 0.0))


def objective(X, Y, U, V, Z, l1=0.0, l2=0.0):
    return (divergence(X, U, V) + divergence(Y, V, Z) + l1 * (U.sum() + V.sum() + Z.sum())
            + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum()))


def fit(X, Y, U, V, Z, max_iter, tol, alpha=0.5, l1=0.0, l2=0.0, mask=7):
    """The reference's loop (cmf_solvers.py:132-195): error at init, a step per iteration, every 10th iteration when tol > 0 the
    stopping test (previous - error) / error_at_init < tol.  Returns (U, V, Z, n_iter, ratios) -- ratios: the left side of the
    test at every check."""
    ex, ey = errors(X, Y, U, V, Z)
    prev = init = alpha * ex + (1 - alpha) * ey
    ratios = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        U, V, Z = step(X, Y, U, V, Z, l1, l2, mask)
        if tol > 0 and n_iter % 10 == 0:
            ex, ey = errors(X, Y, U, V, Z)
            err = alpha * ex + (1 - alpha) * ey
            ratios.append((prev - err) / init)
            if ratios[-1] < tol:
                break
            prev = err
    return U, V, Z, n_iter, ratios
