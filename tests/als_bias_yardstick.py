"""NumPy yardstick of the biased ALS model (helper of test_als_bias_host.py / test_gpu_als_bias.py; not collected), built on
als_yardstick, which it leaves alone.

For a relation with entry weights and biases enabled (written for X; Y is the same with V, Z and its own mu, r, c)

    1/2 sum_O w_ij (x_ij - mu - r_i - c_j - u_i.v_j)^2 + l2/2 (|U|^2 + |V|^2 + |Z|^2) + lb/2 (|r|^2 + |c|^2),     mu fixed, lb >= 0

One iteration (``step``) is block coordinate descent:

    1. the factor sweeps V, U, Z of ``als_yardstick.step``, by whichever route the call names, on the relation with the ADJUSTED
       targets  bt = t - mu - r_i - c_j  (``adjusted``): a biased sweep IS ``als_yardstick.sweep`` on that relation;
    2. per biased relation r, then c from the new r (``bias_sweep``), each the exact minimiser of its block,
           r_i = sum_{j in O_i} w (t - mu - c_j - u_i.v_j) / (sum_{j in O_i} w + lb),
       exactly 0 for a row without stored entries or with a zero denominator.
    The bias blocks follow the update mask of the factor on their axis: r_x with U, c_x and r_y with V, c_y with Z.

``bias`` of a relation is None (not biased) or a tuple (mu, r, c).  ``dtype=np.float64`` is the yardstick.

``dtype=np.float32`` mirrors the roundings of the device (cmf_als_bias.hip.h), and exists only to size the tolerances:
    * bt = ((t - mu) - r_i) - c_j, each subtraction rounded once in float32, and bp = w bt rounded once (``adjusted`` hands bt on as
      the relation's targets; als_yardstick forms w t in float32);
    * a bias sweep forms every term  w (((t - mu) - other_j) - a.b)  in float32 from a float32 dot product, adds the terms and the
      weights in float64, piece by piece (``piece`` consecutive stored entries, the pieces in piece order), divides in float64 and
      rounds the quotient to float32 once.
What the mirror does not copy is the ORDER of the float32 dot (the device adds four products per lane and then a butterfly over
k_pad / 4 lanes; NumPy adds pairwise) and the order of the float64 sums inside a piece (lane groups, then group order).  The rule
of the project prices exactly that:

    tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|)      per factor and per bias vector

Derivation for a bias vector.  One term carries the error of its dot, at most about k eps |a||b|, and three subtractions and a
product, 4 eps each of the running value: (k + 4) eps max|term| in all.  The float64 sums add nothing visible (2^-53 per
addition), so the quotient sum(terms) / (sum w + lb) is a weighted MEAN of residuals with that error per term, and the final
rounding adds one eps of the result: |r32 - r64| <= (k + 5) eps max|residual| -- within the floor (k + 16) 2^-24 max|y64| when
the residuals are of the size of the biases, and priced by the first term, 4 max|y32 - y64|, when they are much larger (a start
far from the fit).  A bias vector inherits no cond(H) factor: there is no solve.  The factors are priced as in als_yardstick.
The cap of DESIGN section 17 stays: a comparison is only made where 4 max|y32 - y64| <= CAP max|y64| (``within_cap``) -- where the
float32 run itself has drifted further than that from float64, the case says nothing about the device and the fixture changes,
not the rule."""
import copy

import numpy as np

import als_yardstick as A

U_BIT, V_BIT, Z_BIT = A.U_BIT, A.V_BIT, A.Z_BIT
CAP = 1.0e-3                                    # 4 max|y32 - y64| / max|y64| above which a case is not a parity case
BIAS_BITS = ((U_BIT, V_BIT), (V_BIT, Z_BIT))     # [relation][axis]: the factor whose mask bit moves that bias block


def zero_bias(rel, mu=0.0):
    return (float(mu), np.zeros(rel.shape[0]), np.zeros(rel.shape[1]))


def weighted_mean(rel):
    """mu: the weighted mean of the stored targets, in float64 (0 without weight)."""
    s = float(rel.w.sum())
    return float((rel.w * rel.t).sum() / s) if s > 0 else 0.0


def adjusted(rel, bias, dtype=np.float64):
    """The relation the factor sweeps read: targets bt = ((t - mu) - r_i) - c_j, each operation rounded once in ``dtype``."""
    if bias is None:
        return rel
    mu, r, c = bias
    bt = ((rel.t.astype(dtype) - dtype(mu)).astype(dtype) - np.asarray(r, dtype=dtype)[rel.r]).astype(dtype)
    bt = (bt - np.asarray(c, dtype=dtype)[rel.c]).astype(dtype).astype(np.float64)
    out = copy.copy(rel)
    out.t = bt
    order = np.lexsort((rel.r, rel.c))
    (ip0, c0, _, w0), (ip1, r1, _, w1) = rel.images
    out.images = ((ip0, c0, bt, w0), (ip1, r1, bt[order], w1))
    return out


def bias_sweep(rel, Fa, Fb, bias, lb, axis, dtype=np.float64, piece=None):
    """The bias vector of ``axis`` (0 rows, 1 columns) one sweep would write: Fa / Fb the factors of the relation's rows / columns."""
    mu, r, c = bias
    indptr, idx, t, w = rel.images[axis]
    own, gathered, other = (Fa, Fb, c) if axis == 0 else (Fb, Fa, r)
    own, gathered = np.asarray(own, dtype=dtype), np.asarray(gathered, dtype=dtype)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    d = np.einsum("ij,ij->i", own[rows], gathered[idx]).astype(dtype)
    res = (((t.astype(dtype) - dtype(mu)).astype(dtype) - np.asarray(other, dtype=dtype)[idx]).astype(dtype) - d).astype(dtype)
    term = (w.astype(dtype) * res).astype(dtype).astype(np.float64)
    w64 = w.astype(dtype).astype(np.float64)
    out = np.zeros(n, dtype=np.float64)
    for i in range(n):
        a, b = int(indptr[i]), int(indptr[i + 1])
        if a == b:
            continue
        L = (b - a) if not piece or piece < 0 else int(piece)
        num = ws = 0.0
        for q in range(a, b, L):
            num += float(term[q:min(q + L, b)].sum())
            ws += float(w64[q:min(q + L, b)].sum())
        den = ws + float(lb)
        out[i] = num / den if den > 0 else 0.0
    return out.astype(dtype).astype(np.float64)


def step(X, Y, Wx, Wy, U, V, Z, bx, by, l2, lb, *, mask=7, nn_mask=0, nn_sweeps=0, cg_steps=0, dtype=np.float64, piece=None):
    """One iteration; returns new (U, V, Z, bx, by), the inputs are left alone.  X / Y may be ``Relation`` objects."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    U, V, Z = A.step(adjusted(Rx, bx, dtype), adjusted(Ry, by, dtype), None, None, U, V, Z, l2, mask=mask, nn_mask=nn_mask,
                     nn_sweeps=nn_sweeps, cg_steps=cg_steps, dtype=dtype)
    out = []
    for which, (rel, Fa, Fb, bias) in enumerate(((Rx, U, V, bx), (Ry, V, Z, by))):
        if bias is not None:
            mu, r, c = bias
            if mask & BIAS_BITS[which][0]:
                r = bias_sweep(rel, Fa, Fb, (mu, r, c), lb, 0, dtype, piece)
            if mask & BIAS_BITS[which][1]:
                c = bias_sweep(rel, Fa, Fb, (mu, r, c), lb, 1, dtype, piece)
            bias = (mu, np.array(r, dtype=np.float64), np.array(c, dtype=np.float64))
        out.append(bias)
    return U, V, Z, out[0], out[1]


def objective(X, Y, Wx, Wy, U, V, Z, bx, by, l2, lb):
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    val = A.objective(adjusted(Rx, bx), adjusted(Ry, by), None, None, U, V, Z, l2)
    for bias in (bx, by):
        if bias is not None:
            val += 0.5 * lb * (float((np.asarray(bias[1], np.float64) ** 2).sum()) + float((np.asarray(bias[2], np.float64) ** 2).sum()))
    return val


def bias_gradient(rel, Fa, Fb, bias, lb, axis):
    """The gradient of the objective with respect to the bias vector of ``axis``."""
    mu, r, c = bias
    Fa, Fb = np.asarray(Fa, np.float64), np.asarray(Fb, np.float64)
    e = rel.t - mu - np.asarray(r)[rel.r] - np.asarray(c)[rel.c] - np.einsum("ij,ij->i", Fa[rel.r], Fb[rel.c])
    vec, at = (r, rel.r) if axis == 0 else (c, rel.c)
    return lb * np.asarray(vec, np.float64) - np.bincount(at, weights=rel.w * e, minlength=len(vec))


def predict(Fa, Fb, rows, cols, bias=None, link="linear"):
    """float64: f(mu + r_i + c_j + a_i.b_j) of the pairs."""
    Fa, Fb = np.asarray(Fa, np.float64), np.asarray(Fb, np.float64)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    s = np.einsum("ij,ij->i", Fa[rows], Fb[cols])
    if bias is not None:
        s = s + bias[0] + np.asarray(bias[1], np.float64)[rows] + np.asarray(bias[2], np.float64)[cols]
    return s if link == "linear" else 1.0 / (1.0 + np.exp(-s))


def predict_bound(Fa, Fb, rows, cols, k, bias=None):
    """(k + 16) 2^-24 (|offset| + |r| + |c| + sum |a||b|) per pair."""
    Fa, Fb = np.abs(np.asarray(Fa, np.float64)), np.abs(np.asarray(Fb, np.float64))
    s = np.einsum("ij,ij->i", Fa[rows], Fb[cols])
    if bias is not None:
        s = s + abs(bias[0]) + np.abs(bias[1])[rows] + np.abs(bias[2])[cols]
    return (k + 16) * 2.0 ** -24 * s


def fit(X, Y, Wx, Wy, U, V, Z, max_iter, l2, *, x_biases=False, y_biases=False, lb=None, bx=None, by=None, mask=7, nn_mask=0,
        nn_sweeps=0, cg_steps=0, dtype=np.float64, piece=None, trace=None):
    """``max_iter`` iterations from zero biases and mu = the weighted mean of the stored targets (or from the given ``bx`` / ``by``);
    returns (U, V, Z, bx, by); ``trace`` (a list) receives the objective after every iteration."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    lb = l2 if lb is None else lb
    if bx is None and x_biases:
        bx = zero_bias(Rx, weighted_mean(Rx))
    if by is None and y_biases:
        by = zero_bias(Ry, weighted_mean(Ry))
    for _ in range(max_iter):
        U, V, Z, bx, by = step(Rx, Ry, None, None, U, V, Z, bx, by, l2, lb, mask=mask, nn_mask=nn_mask, nn_sweeps=nn_sweeps,
                               cg_steps=cg_steps, dtype=dtype, piece=piece)
        if trace is not None:
            trace.append(objective(Rx, Ry, None, None, U, V, Z, bx, by, l2, lb))
    return U, V, Z, bx, by


tolerance = A.tolerance


def within_cap(y32, y64):
    """Is the case a parity case: 4 max|y32 - y64| <= CAP max|y64| (a vector of exact zeros passes when both are)."""
    y32, y64 = np.asarray(y32, np.float64), np.asarray(y64, np.float64)
    return 4.0 * float(np.max(np.abs(y32 - y64))) <= CAP * float(np.max(np.abs(y64)))


def planted(seed, density, noise, k=3, m=120, d=150, p=20, rank=3, mu=3.5, y_noise=0.05):
    """The planted rating problem of DESIGN section 20, the one behind the table of the proposal: ONE stream RandomState(seed), in
    the order of click_problem.clicks -- the true factors U, V, Z (randn, rank ``rank``), unit-variance row and column offsets r, c,
    the noise of X, the noise of Y, the mask, the starts.  X = mu + r + c + U V^T + noise randn (m x d), observed on the cells where
    rand < ``density``; Y = V Z^T + ``y_noise`` randn (d x p), fully observed (no weights); starts 0.1 randn with ``k`` columns.
    Returns (X, Y, Wx, (U0, V0, Z0)) with Wx a SciPy sparse 0/1 matrix.  The data do not depend on ``k``; the starts do."""
    import scipy.sparse as sp
    rng = np.random.RandomState(seed)
    U, V, Z = rng.randn(m, rank), rng.randn(d, rank), rng.randn(p, rank)
    r, c = rng.randn(m), rng.randn(d)
    X = mu + r[:, None] + c[None, :] + U @ V.T + noise * rng.randn(m, d)
    Y = V @ Z.T + y_noise * rng.randn(d, p)
    Wx = sp.csr_matrix((rng.rand(m, d) < density).astype(np.float64))
    start = tuple(0.1 * rng.randn(n, k) for n in (m, d, p))
    return X, Y, Wx, start


def heldout_rmse(X, Wx, U, V, bias=None):
    """RMSE of the model on the cells of X outside the pattern of Wx."""
    rows, cols = np.nonzero(np.asarray(Wx.todense()) == 0)
    return float(np.sqrt(np.mean((predict(U, V, rows, cols, bias) - np.asarray(X)[rows, cols]) ** 2)))
