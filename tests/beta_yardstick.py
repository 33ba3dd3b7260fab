"""Float64 restatement of the beta-divergence multiplicative updates of the collective model (plain NumPy, dense T), 0 <= beta <= 2.
It evaluates the formulas and nothing else:

    EPS = 2^-23,  S = A B^T,  P = max(S, EPS)^(beta - 2)
    num = (T .* P) B        den = (S .* P) B              (den takes the UNCLAMPED S: a zero row of A gives an exact 0)
    F <- F .* (num / reg(den, F))^gamma,    gamma = 1 / (2 - beta) for beta < 1,  1 for 1 <= beta <= 2
    reg(den, F) = den + l1 + l2 F, then den == 0 -> EPS
    V from the old U, Z with both relations' products added; then U and Z from the new V  (pycmf/cmf_solvers.py:248-263)
    d_beta(t | s) = (t^beta + (beta - 1) s^beta - beta t s^(beta - 1)) / (beta (beta - 1)),  s = max(S, EPS)
        beta = 0: t / s - log(t / s) - 1        beta = 1: t log(t / s) - t + s        t = 0 (beta > 0): s^beta / beta
    error = alpha sqrt(2 D_x) + (1 - alpha) sqrt(2 D_y)

This is sklearn's ``_multiplicative_update_w`` / ``_h`` and ``_beta_divergence`` applied to each block wherever S >= EPS;
tests/test_beta_host.py holds it against sklearn.

Tolerances of the float32 device against this yardstick (tests/test_gpu_beta.py)
--------------------------------------------------------------------------------
First-order forward bounds with u = 2^-24.  Every sum has non-negative terms, so no order of summation can cancel and the bounds
hold for any order.  ``lmax`` = max |log2 max(s, EPS)| over the products of the case (from this yardstick's own S).

``pow_err(e, l)``: relative error of  exp2(e log2 x)  with |log2 x| <= l on the device's raw v_log_f32 / v_exp_f32, each documented
with 1 ULP (= 2 u relative): the logarithm carries 2 u l absolute, the product with e one more rounding, u |e| l, and 2 u |e| l
after scaling -- an absolute error 3 u |e| l of the exponent, which exp2 turns into that much relative (ln 2 < 1), plus its own
2 u:  (3 |e| l + 2) u.  The Itakura-Saito policy takes p = r r from a 1-ULP reciprocal instead: 2 * 2 u + u = 5 u.

``tau_products(k, L, beta, lmax)``: one element of num or den.  gamma_k = k u on s, amplified by |beta - 2| through the power and
entering den once more through s itself: k (|beta - 2| + 1) u; the power's own error; one rounding for t p or s p; gamma_L = L u on
the outer sum (L: the streamed extent, m + p for V); 8 single roundings for the rest (the sums over at most a few slabs of shares).

``tau_step(tn, beta, lq)``: one updated element from products with bound ``tn`` each.  The quotient carries 2 tn, two roundings of
the regulariser and one of the division; the final power contracts that by gamma <= 1 and adds its own error -- 2 u for the
correctly rounded sqrtf at gamma = 1/2, pow_err(gamma, lq) otherwise with lq = max |log2 q| over the non-zero quotients of the
case -- and the product with F one rounding.  In a full step U and Z read the new V, whose bound tV enters their s (amplified by
|beta - 2| in num, |beta - 2| + 1 in den) and the streamed factor of both outer products: gamma (2 |beta - 2| + 3) tV more.

``div_tol``: the three terms of the closed form are evaluated in float32 and summed in float64, so the bound is the per-term
relative error (gamma_k on s amplified by at most 2, two powers, a handful of roundings) times the sum of the ABSOLUTE values of
the three terms; divergence_terms returns that sum.

``fit_rtol(n, t_full)`` bounds the fitted factors after n iterations, relative to the largest element: n times the full-step bound
of the fit's shape, times 2 for the growth of an error that the following sweeps read again.
"""
import numpy as np

EPS = 2.0 ** -23
U_BIT, V_BIT, Z_BIT = 1, 2, 4
_u = 2.0 ** -24


def gamma_of(beta):
    return 1.0 / (2.0 - beta) if beta < 1 else 1.0


def pow_err(e, l):
    return (3.0 * abs(e) * l + 2.0) * _u


def lmax_of(A, B):
    """max |log2 max(s, EPS)| over S = A B^T."""
    S = np.maximum(np.asarray(A, np.float64) @ np.asarray(B, np.float64).T, EPS)
    return float(np.abs(np.log2(S)).max())


def tau_products(k, L, beta, lmax):
    power = 5.0 * _u if beta == 0 else pow_err(beta - 2.0, lmax)
    return (k * (abs(beta - 2.0) + 1.0) + L + 9.0) * _u + power


def tau_step(tn, beta, lq, t_v=0.0):
    g = gamma_of(beta)
    own = 0.0 if g == 1.0 else (2.0 * _u if g == 0.5 else pow_err(g, lq))
    return g * (2.0 * tn + 3.0 * _u + (2.0 * abs(beta - 2.0) + 3.0) * t_v) + own + _u


def fit_rtol(n_iter, t_full):
    return 2.0 * n_iter * t_full


def pair(T, A, B, beta):
    """(num, den) = ((T .* P) B, (S .* P) B) with the rows of A."""
    T, A, B = (np.asarray(M, np.float64) for M in (T, A, B))
    S = A @ B.T
    P = np.maximum(S, EPS) ** (beta - 2.0)
    return (T * P) @ B, (S * P) @ B


def pair_t(T, A, B, beta):
    """The same for the rows of B: T^T against B A^T."""
    return pair(np.asarray(T).T, B, A, beta)


def sweep_products(X, Y, U, V, Z, beta, sweep):
    """(num, den) of sweep 0 = U, 1 = V, 2 = Z from the given factors."""
    if sweep == 0:
        return pair(X, U, V, beta)
    if sweep == 2:
        return pair_t(Y, V, Z, beta)
    n1, d1 = pair_t(X, U, V, beta)
    n2, d2 = pair(Y, V, Z, beta)
    return n1 + n2, d1 + d2


def reg(den, F, l1, l2):
    den = np.array(den, dtype=np.float64)
    if l1 > 0:
        den = den + l1
    if l2 > 0:
        den = den + l2 * F
    den[den == 0] = EPS
    return den


def quotient(num, den, F, l1, l2):
    return num / reg(den, F, l1, l2)


def step(X, Y, U, V, Z, beta, l1=0.0, l2=0.0, mask=7):
    """One sweep V, U, Z; returns new arrays (inputs untouched)."""
    U, V, Z = (np.array(F, dtype=np.float64) for F in (U, V, Z))
    g = gamma_of(beta)
    for bit, sweep in ((V_BIT, 1), (U_BIT, 0), (Z_BIT, 2)):
        if not mask & bit:
            continue
        F = (U, V, Z)[sweep]
        num, den = sweep_products(X, Y, U, V, Z, beta, sweep)
        F = F * quotient(num, den, F, l1, l2) ** g
        if sweep == 0:
            U = F
        elif sweep == 1:
            V = F
        else:
            Z = F
    return U, V, Z


def divergence_terms(T, A, B, beta):
    """(D_beta, the sum of the absolute values of the closed form's terms) over every cell."""
    T, A, B = (np.asarray(M, np.float64) for M in (T, A, B))
    S = np.maximum(A @ B.T, EPS)
    pos = T > 0
    t, s = T[pos], S[pos]
    if beta == 0:
        if not pos.all():
            return np.inf, np.inf
        q = t / s
        return float((q - np.log(q) - 1.0).sum()), float((q + np.abs(np.log(q)) + 1.0).sum())
    s0 = S[~pos] ** beta / beta
    if beta == 1:
        a, b, c = t * np.log(t / s), -t, s
    else:
        den = beta * (beta - 1.0)
        a, b, c = t ** beta / den, (beta - 1.0) * s ** beta / den, -beta * t * s ** (beta - 1.0) / den
    return float((a + b + c).sum() + s0.sum()), float((np.abs(a) + np.abs(b) + np.abs(c)).sum() + s0.sum())


def divergence(T, A, B, beta):
    return divergence_terms(T, A, B, beta)[0]


def div_tol(k, beta, lmax, sum_abs):
    return (2.0 * k * _u + 2.0 * pow_err(2.0, lmax) + 8.0 * _u) * sum_abs


def errors(X, Y, U, V, Z, beta):
    return np.sqrt(2 * max(divergence(X, U, V, beta), 0.0)), np.sqrt(2 * max(divergence(Y, V, Z, beta), 0.0))


def objective(X, Y, U, V, Z, beta, l1=0.0, l2=0.0):
    return (divergence(X, U, V, beta) + divergence(Y, V, Z, beta) + l1 * (U.sum() + V.sum() + Z.sum())
            + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum()))


def fit(X, Y, U, V, Z, beta, max_iter, tol, alpha=0.5, l1=0.0, l2=0.0, mask=7):
    """The reference's loop (cmf_solvers.py:132-195): error at init, a step per iteration, every 10th iteration when tol > 0 the
    stopping test (previous - error) / error_at_init < tol.  Returns (U, V, Z, n_iter, ratios) -- ratios: the left side of the
    test at every check."""
    ex, ey = errors(X, Y, U, V, Z, beta)
    prev = init = alpha * ex + (1 - alpha) * ey
    ratios = []
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        U, V, Z = step(X, Y, U, V, Z, beta, l1, l2, mask)
        if tol > 0 and n_iter % 10 == 0:
            ex, ey = errors(X, Y, U, V, Z, beta)
            err = alpha * ex + (1 - alpha) * ey
            ratios.append((prev - err) / init)
            if ratios[-1] < tol:
                break
            prev = err
    return U, V, Z, n_iter, ratios


def fit_problem(seed, m=60, d=80, p=40, k=6):
    """The fit case of the GPU test: strictly positive float32-exact data and custom initial factors."""
    rng = np.random.RandomState(seed)

    def f32(a):
        return np.asarray(a, dtype=np.float32).astype(np.float64)
    W, H, G = (np.abs(rng.randn(n, k)) + 0.1 for n in (m, d, p))
    X = f32((W @ H.T) * np.exp(0.3 * rng.randn(m, d)) + 0.05)
    Y = f32((H @ G.T) * np.exp(0.3 * rng.randn(d, p)) + 0.05)
    U, V, Z = (f32(np.abs(rng.randn(n, k)) + 0.1) for n in (m, d, p))
    return X, Y, U, V, Z


FIT_TOL = 1e-2
FIT_SEEDS = {0.0: 3, 0.5: 2, 1.5: 6}   # beta -> seed; test_beta_host.py asserts the 10 % margin of every check for these
