"""NumPy yardstick of the Huber loss of the ALS solver (helper of test_als_huber_host.py / test_gpu_als_huber.py; not collected).

A relation with a delta d > 0 contributes  sum_O w rho_d(t - a.b)  instead of  1/2 sum_O w (t - a.b)^2:

    rho_d(r) = 1/2 r^2 if |r| <= d,  d (|r| - 1/2 d) otherwise;       omega(r) = 1 if |r| <= d,  d / |r| otherwise
    rho_d(r) <= rho_d(r0) + 1/2 omega(r0) (r^2 - r0^2),  tight at r = +-r0                                  (``bound``)

With r0 the residual under the current row the majoriser of a row is the ALS row problem under w omega on the same targets.  So
nothing is solved here: ``reweighted`` puts w omega, taken at the given factors, in place of w, and ``sweep`` hands the reweighted
relations to the yardsticks of the routes -- ``als_yardstick.sweep`` (exact, coordinate descent, conjugate gradients),
``nncg_yardstick.sweep`` (projected conjugate gradients), ``als_dual_yardstick.dual_rows`` (dual) and ``als_bias_yardstick``
(adjusted targets, bias blocks) -- in front of every sweep, as the device runs its reweighting pass.

``dtype=np.float32`` runs the scores, the residuals and omega in float32 as well (and then the routes' own float32 forms): it
exists only to size the tolerances of the device tests by ``als_yardstick.tolerance``, in the sense of logit_yardstick."""
import copy

import numpy as np
import scipy.sparse as sp

import als_yardstick as A
import nncg_yardstick as N
import als_dual_yardstick as D
import als_bias_yardstick as B

U_BIT, V_BIT, Z_BIT = A.U_BIT, A.V_BIT, A.Z_BIT


def omega(r, delta, dtype=np.float64):
    r = np.abs(np.asarray(r, dtype=dtype))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r <= dtype(delta), dtype(1), dtype(delta) / r).astype(dtype)


def rho(r, delta):
    r = np.abs(np.asarray(r, dtype=np.float64))
    return np.where(r <= delta, 0.5 * r * r, delta * (r - 0.5 * delta))


def bound(r, r0, delta):
    """The half-quadratic majoriser of rho_delta at r0, evaluated at r."""
    r, r0 = np.asarray(r, np.float64), np.asarray(r0, np.float64)
    return rho(r0, delta) + 0.5 * omega(r0, delta) * (r * r - r0 * r0)


def residuals(rel, Fa, Fb, dtype=np.float64):
    """t - a.b on the stored entries of an observed relation (pattern order), Fa / Fb the factors of its rows / columns."""
    Fa, Fb = np.asarray(Fa, dtype=dtype), np.asarray(Fb, dtype=dtype)
    s = np.einsum("ij,ij->i", Fa[rel.r], Fb[rel.c]).astype(dtype)
    return (rel.t.astype(dtype) - s).astype(dtype)


def with_weights(rel, w):
    """``rel`` with the weights ``w`` (pattern order) on the same pattern and targets."""
    out = copy.copy(rel)
    w = np.asarray(w, np.float64)
    out.w = w
    order = np.lexsort((rel.r, rel.c))
    (ip0, c0, t0, _), (ip1, r1, t1, _) = rel.images
    out.images = ((ip0, c0, t0, w), (ip1, r1, t1, w[order]))
    return out


def reweighted(rel, Fa, Fb, delta, dtype=np.float64):
    """An ``als_yardstick.Relation`` with the same targets and the weights w omega, omega taken at the factors Fa / Fb of the
    relation's rows / columns.  A relation without a delta, or a full one, is returned as it is."""
    if not delta or not rel.observed:
        return rel
    om = omega(residuals(rel, Fa, Fb, dtype), delta, dtype)
    return with_weights(rel, (rel.w.astype(dtype) * om).astype(dtype).astype(np.float64))


def loss(rel, Fa, Fb, delta):
    """sum_O w rho_delta(t - a.b), float64."""
    return float((rel.w * rho(residuals(rel, Fa, Fb), delta)).sum())


def sweep(Rx, Ry, U, V, Z, which, l2, *, deltas=(None, None), non_negative=False, nn_sweeps=0, cg_steps=0, nn_cg_steps=0, dual_max=0,
          bx=None, by=None, rows=None, dtype=np.float64):
    """The rows ``rows`` (None = all) of the swept factor ``which`` by the route the device gives it, the Huber relations reweighted
    at the current factors first (under biases ``bx`` / ``by``: on the adjusted targets)."""
    Rx = reweighted(B.adjusted(Rx, bx, dtype), U, V, deltas[0], dtype)
    Ry = reweighted(B.adjusted(Ry, by, dtype), V, Z, deltas[1], dtype)
    k = np.asarray(U if U is not None else V).shape[1]
    full = any(not rel.observed for rel, _, _, _ in A._sides(Rx, Ry, U, V, Z, which))
    how = A.route(A.observed(Rx, Ry, which), non_negative, nn_sweeps, cg_steps, nn_cg_steps, dual_max, shared_term=full, k_pad=D.k_pad(k))
    if how == A.ROWS_DUAL:
        return D.dual_rows(Rx, Ry, U, V, Z, which, l2, dual_max, rows=rows, dtype=dtype, non_negative=non_negative)
    return N.sweep(Rx, Ry, U, V, Z, which, l2, non_negative=non_negative, nn_sweeps=nn_sweeps, cg_steps=cg_steps, nn_cg_steps=nn_cg_steps,
                   rows=rows, dtype=dtype)


def bias_sweep(rel, Fa, Fb, bias, lb, axis, delta, dtype=np.float64):
    """``als_bias_yardstick.bias_sweep`` under the weights w omega, omega at the residuals of the biased model."""
    if delta:
        om = omega(residuals(B.adjusted(rel, bias, dtype), Fa, Fb, dtype), delta, dtype)
        rel = with_weights(rel, (rel.w.astype(dtype) * om).astype(dtype).astype(np.float64))
    return B.bias_sweep(rel, Fa, Fb, bias, lb, axis, dtype)


def step(Rx, Ry, U, V, Z, l2, *, deltas=(None, None), mask=7, nn_mask=0, bx=None, by=None, lb=0.0, dtype=np.float64, **route):
    """One iteration V, U, Z (then, under biases, the bias blocks as ``als_bias_yardstick.step`` sweeps them); returns new
    (U, V, Z, bx, by), the inputs are left alone.  ``route``: nn_sweeps, cg_steps, nn_cg_steps, dual_max."""
    F = {w: np.array(M, dtype=dtype) for w, M in zip("UVZ", (U, V, Z))}
    for w, bit in (("V", V_BIT), ("U", U_BIT), ("Z", Z_BIT)):
        if mask & bit:
            F[w] = sweep(Rx, Ry, F["U"], F["V"], F["Z"], w, l2, deltas=deltas, non_negative=bool(nn_mask & bit), bx=bx, by=by, dtype=dtype,
                         **route)
    out = []
    for which, (rel, Fa, Fb, bias) in enumerate(((Rx, F["U"], F["V"], bx), (Ry, F["V"], F["Z"], by))):
        if bias is not None:
            mu, r, c = bias
            if mask & B.BIAS_BITS[which][0]:
                r = bias_sweep(rel, Fa, Fb, (mu, r, c), lb, 0, deltas[which], dtype)
            if mask & B.BIAS_BITS[which][1]:
                c = bias_sweep(rel, Fa, Fb, (mu, r, c), lb, 1, deltas[which], dtype)
            bias = (mu, np.array(r, dtype=np.float64), np.array(c, dtype=np.float64))
        out.append(bias)
    return F["U"], F["V"], F["Z"], out[0], out[1]


def relation_terms(Rx, Ry, U, V, Z, deltas=(None, None), bx=None, by=None):
    """(term_x, term_y) of the objective: sum w rho_delta of a Huber relation, half the squared residual of another."""
    out = []
    for rel, Fa, Fb, delta, bias in ((Rx, U, V, deltas[0], bx), (Ry, V, Z, deltas[1], by)):
        rel = B.adjusted(rel, bias)
        out.append(loss(rel, Fa, Fb, delta) if delta and rel.observed else 0.5 * A.residual_sq(rel, Fa, Fb))
    return tuple(out)


def objective(Rx, Ry, U, V, Z, l2, *, deltas=(None, None), bx=None, by=None, lb=0.0):
    U, V, Z = (np.asarray(F, np.float64) for F in (U, V, Z))
    val = sum(relation_terms(Rx, Ry, U, V, Z, deltas, bx, by)) + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum())
    for bias in (bx, by):
        if bias is not None:
            val += 0.5 * lb * ((np.asarray(bias[1]) ** 2).sum() + (np.asarray(bias[2]) ** 2).sum())
    return float(val)


def errors(Rx, Ry, U, V, Z, deltas=(None, None), bx=None, by=None):
    """What the estimator's error metric takes from each relation: sqrt(2 term) -- the root of the squared residuals of a Frobenius
    relation, sqrt(2 sum w rho) of a Huber one."""
    tx, ty = relation_terms(Rx, Ry, U, V, Z, deltas, bx, by)
    return float(np.sqrt(2.0 * tx)), float(np.sqrt(2.0 * ty))


def fit(Rx, Ry, U, V, Z, max_iter, l2, *, deltas=(None, None), mask=7, nn_mask=0, bx=None, by=None, lb=0.0, dtype=np.float64, trace=None,
        **route):
    """``max_iter`` iterations without a stopping test; returns (U, V, Z, bx, by); ``trace`` (a list) receives the objective after
    every iteration."""
    for _ in range(max_iter):
        U, V, Z, bx, by = step(Rx, Ry, U, V, Z, l2, deltas=deltas, mask=mask, nn_mask=nn_mask, bx=bx, by=by, lb=lb, dtype=dtype, **route)
        if trace is not None:
            trace.append(objective(Rx, Ry, U, V, Z, l2, deltas=deltas, bx=bx, by=by, lb=lb))
    return U, V, Z, bx, by


class Planted:
    """The planted problem of the issue: X 120 x 150 of rank 3, 30 % observed, 5 % of the observed entries shifted by +-10; Y full."""
    l2, max_iter, k = 0.5, 10, 3

    def __init__(self, seed, k=3):
        m, d, p, rank = 120, 150, 20, 3
        rng = np.random.RandomState(seed)
        U0, V0, Z0 = rng.randn(m, rank), rng.randn(d, rank), rng.randn(p, rank)
        M = rng.rand(m, d) < 0.3
        X = U0 @ V0.T + 0.1 * rng.randn(m, d)
        out = M & (rng.rand(m, d) < 0.05)
        sign = rng.choice([-1, 1], (m, d))
        self.clean, self.noisy = U0 @ V0.T, X.copy()     # the planted product; the data before the outliers
        X[out] += 10.0 * sign[out]
        self.Y = V0 @ Z0.T + 0.1 * rng.randn(d, p)
        self.U, self.V, self.Z = 0.1 * rng.randn(m, k), 0.1 * rng.randn(d, k), 0.1 * rng.randn(p, k)
        self.k = k
        self.X, self.M, self.outliers = X, M, out
        self.W = sp.csr_matrix(M.astype(np.float64))
        self.Rx, self.Ry = A.Relation(X, self.W), A.Relation(self.Y, None)

    def heldout_rmse(self, U, V):
        """RMSE of U V^T against the planted product on the unobserved cells."""
        E = (np.asarray(U, np.float64) @ np.asarray(V, np.float64).T - self.clean)[~self.M]
        return float(np.sqrt(np.mean(E * E)))


def planted(seed, k=3):
    return Planted(seed, k)
