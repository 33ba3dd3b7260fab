"""NumPy yardstick of the ALS solver's logistic loss (helper of test_als_logit_host.py / test_gpu_als_logit.py; not collected),
built on als_yardstick's ``Relation`` / ``shared`` / ``cd_rows``.

    minimise  sum_{logistic sides} sum_O w [softplus(a.b) - t (a.b)]  +  1/2 sum_{Frobenius sides} (as als_yardstick)
              + l2/2 (|U|^2 + |V|^2 + |Z|^2),   l2 > 0

in the sweep order V, U, Z, the new V used for U and Z.  ``logit = (x is logistic, y is logistic)``; a logistic relation is
OBSERVED (weights W), its targets in [0, 1].  The Jaakkola-Jordan bound, tight at s = +-xi,

    w [softplus(s) - t s]  <=  1/2 w kappa(xi) s^2 - w (t - 1/2) s + const,     kappa(xi) = tanh(xi / 2) / (2 xi),   kappa(0) = 1/4

with xi the score under the CURRENT row turns the row update into als_yardstick's system with w kappa for w and w (t - 1/2) for
w t (``systems``):

    H_i = sum_{e in O_i} w_e kappa_e b_e b_e^T + S + l2 I,      g_i = sum_{e in O_i} w_e (t_e - 1/2) b_e + N_i.

A sweep solves it exactly (signed; a non-negative factor with ``nn_sweeps = 0`` is then projected, without a descent guarantee) or,
for a non-negative factor with ``nn_sweeps > 0``, runs that many passes of ``cd_rows`` from the current row.  Either way no row
raises the bound above its value at the current row, where it equals the loss: the objective never rises.  A sweep that reads no
logistic relation is als_yardstick's sweep.

``dtype=np.float64`` is the yardstick; ``dtype=np.float32`` runs the same formulas on float32 arrays (the score, kappa, each
product w kappa, w t and w t - w / 2 rounded once) and sizes the tolerances by als_yardstick.tolerance."""
import numpy as np

import als_yardstick as A
from als_yardstick import Relation, as_relation, U_BIT, V_BIT, Z_BIT   # noqa: F401  (re-exported for the tests)

KAPPA_GUARD = 1e-4


def kappa(s, dtype=np.float64):
    """tanh(s / 2) / (2 s), 1/4 where |s| < 1e-4 (there the quotient is within 2^-24 of 1/4 and loses its digits in float32)."""
    s = np.asarray(s, dtype=dtype)
    small = np.abs(s) < dtype(KAPPA_GUARD)
    safe = np.where(small, dtype(1), s)
    return np.where(small, dtype(0.25), np.tanh(dtype(0.5) * safe) / (dtype(2) * safe)).astype(dtype)


def sigmoid(s):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(s, np.float64)))


def pointwise(s, t):
    """softplus(s) - t s, without overflow."""
    s = np.asarray(s, np.float64)
    return np.maximum(s, 0.0) + np.log1p(np.exp(-np.abs(s))) - t * s


def bound(s, xi, t):
    """The Jaakkola-Jordan majoriser of ``pointwise`` at xi, as a function of s (constant included)."""
    s, xi = np.asarray(s, np.float64), np.asarray(xi, np.float64)
    return 0.5 * kappa(xi) * (s * s - xi * xi) - (t - 0.5) * s + pointwise(xi, 0.0) - 0.5 * xi


def _side_logit(which, logit):
    """Per side of the sweep (als_yardstick._sides' order): is its relation logistic?"""
    return {"U": [logit[0]], "Z": [logit[1]], "V": [logit[0], logit[1]]}[which]


def logistic_sweep(which, logit):
    return any(_side_logit(which, logit))


def systems(Rx, Ry, U, V, Z, which, l2, *, logit=(True, False), rows=None, dtype=np.float64):
    """(H [n, k, k], g [n, k]) of the rows ``rows`` (None = all) of the sweep of factor ``which``: the majoriser's system at the
    current rows for a logistic side, als_yardstick's sums for a Frobenius one."""
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], dtype=dtype)
    k = F.shape[1]
    rows = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    H = np.zeros((len(rows), k, k), dtype=dtype)
    g = np.zeros((len(rows), k), dtype=dtype)
    for (rel, trans, B, _), lg in zip(A._sides(Rx, Ry, U, V, Z, which), _side_logit(which, logit)):
        if not rel.observed:
            if lg:
                raise ValueError("a logistic relation must be observed")
            continue
        B = np.asarray(B, dtype=dtype)
        indptr, idx, t, w = rel.images[1 if trans else 0]
        w = w.astype(dtype)
        pv = (w * t.astype(dtype)).astype(dtype)
        for n, i in enumerate(rows):
            a, b = indptr[i], indptr[i + 1]
            if a == b:
                continue
            Bi = B[idx[a:b]]
            if lg:
                s = (Bi @ F[i]).astype(dtype)
                e = (w[a:b] * kappa(s, dtype)).astype(dtype)
                p = (pv[a:b] - dtype(0.5) * w[a:b]).astype(dtype)
            else:
                e, p = w[a:b], pv[a:b]
            Bs = Bi * np.sqrt(e).astype(dtype)[:, None]
            H[n] += Bs.T @ Bs
            g[n] += Bi.T @ p
    S, Nf = A.shared(Rx, Ry, U, V, Z, which, rows=rows, dtype=dtype)
    if S is not None:
        H += S[None]
    if Nf is not None:
        g += Nf
    H[:, np.arange(k), np.arange(k)] += dtype(l2)
    return H, g


def sweep(Rx, Ry, U, V, Z, which, l2, *, logit=(True, False), non_negative=False, nn_sweeps=0, dtype=np.float64, chunk=64):
    """The swept factor ``which``, by the route the device gives it."""
    if not logistic_sweep(which, logit):
        return A.sweep(Rx, Ry, U, V, Z, which, l2, non_negative=non_negative, nn_sweeps=nn_sweeps, dtype=dtype, chunk=chunk)
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], dtype=dtype)
    descend = bool(non_negative and nn_sweeps)
    out = np.empty_like(F)
    for r0 in range(0, F.shape[0], chunk):
        sel = np.arange(r0, min(r0 + chunk, F.shape[0]))
        H, g = systems(Rx, Ry, U, V, Z, which, l2, logit=logit, rows=sel, dtype=dtype)
        out[sel] = A.cd_rows(H, g, F[sel], nn_sweeps, dtype) if descend else np.linalg.solve(H, g[:, :, None])[:, :, 0]
    if descend:
        out[A.no_information(Rx, Ry, U, V, Z, which)] = 0
    return np.maximum(out, dtype(0)) if non_negative and not descend else out


def step(X, Y, Wx, Wy, U, V, Z, l2, *, logit=(True, False), mask=7, nn_mask=0, nn_sweeps=0, dtype=np.float64):
    """One iteration V, U, Z; returns new (U, V, Z), the inputs are left alone.  X / Y may be ``Relation`` objects."""
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    F = {w: np.array(M, dtype=dtype) for w, M in zip("UVZ", (U, V, Z))}
    for w, bit in (("V", V_BIT), ("U", U_BIT), ("Z", Z_BIT)):
        if mask & bit:
            F[w] = sweep(Rx, Ry, F["U"], F["V"], F["Z"], w, l2, logit=logit, non_negative=bool(nn_mask & bit), nn_sweeps=nn_sweeps, dtype=dtype)
    return F["U"], F["V"], F["Z"]


def loss(rel, A_, B):
    """sum_O w [softplus(a.b) - t a.b] of one observed relation, float64."""
    A_, B = np.asarray(A_, np.float64), np.asarray(B, np.float64)
    s = np.einsum("ij,ij->i", A_[rel.r], B[rel.c])
    return float((rel.w * pointwise(s, rel.t)).sum())


def objective(X, Y, Wx, Wy, U, V, Z, l2, *, logit=(True, False)):
    Rx, Ry = as_relation(X, Wx), as_relation(Y, Wy)
    U, V, Z = (np.asarray(F, np.float64) for F in (U, V, Z))
    jx = loss(Rx, U, V) if logit[0] else 0.5 * A.residual_sq(Rx, U, V)
    jy = loss(Ry, V, Z) if logit[1] else 0.5 * A.residual_sq(Ry, V, Z)
    return jx + jy + 0.5 * l2 * ((U ** 2).sum() + (V ** 2).sum() + (Z ** 2).sum())


def planted(seed):
    """The planted problem of the tests, drawn from RandomState(seed) in this order: U0, V0, Z0 (rank 3), P = sigmoid(2 U0 V0^T),
    labels T = rand < P, observed mask M = rand < 0.3, W = M .* (2 where T = 1, else 1), Y = V0 Z0^T + 0.1 randn (fitted full), then
    the start 0.1 randn of U, V, Z (k = 4).  Returns a dict."""
    import scipy.sparse as sp
    rng = np.random.RandomState(seed)
    m, d, p, r, k = 120, 150, 20, 3, 4
    U0, V0, Z0 = rng.randn(m, r), rng.randn(d, r), rng.randn(p, r)
    P = sigmoid(2.0 * U0 @ V0.T)
    T = (rng.rand(m, d) < P).astype(np.float64)
    M = rng.rand(m, d) < 0.3
    W = M * np.where(T == 1, 2.0, 1.0)
    Y = V0 @ Z0.T + 0.1 * rng.randn(d, p)
    start = [0.1 * rng.randn(n, k) for n in (m, d, p)]
    return dict(m=m, d=d, p=p, k=k, l2=0.5, P=P, T=T, M=M, W=W, Wsp=sp.csr_matrix(W), Y=Y, start=start)


def agreement(U, V, prob):
    """The share of the unobserved cells on which the sign of U V^T agrees with P > 1/2."""
    S = np.asarray(U, np.float64) @ np.asarray(V, np.float64).T
    off = ~prob["M"]
    return float(((S > 0) == (prob["P"] > 0.5))[off].mean())
