"""NumPy yardstick of the matrix-free non-negative rows of the ALS solver (helper of test_als_nncg_host.py / test_gpu_als_nncg.py;
not collected): ``nn_cg_steps`` steps of projected conjugate gradients per row of a non-negative factor that has an observed
relation, on the row system of als_yardstick.py with its matrix-free product  H x = sum_e e_e b_e (b_e . x) + S x + l2 x:

    f <- max(f, 0);   r = g - H f;   p = none
    per step:  free_j = f_j > 0 or r_j > 0;  z = r on free, 0 elsewhere;  rho = z.z;  stop unless rho is positive and finite
               p = z + (rho / rho_old) p  if the step before was a free step and free == free_old  ("conjugate"),  else p = z
               q = H p;  pq = p.q;  stop unless positive and finite;  alpha = (p.r) / pq;  t = f + alpha p
               no t_j < 0:  "free" step        f = t;  r -= alpha q;  rho_old = rho;  free_old = free
               else         "projected" step   f+ = max(t, 0);  d = f+ - f;  hd = H d;  dr = d.r;  dhd = d.hd;  stop unless both are
                            positive and finite;  theta = dr / dhd;  theta >= 1: f = f+, r -= hd;  else f = max(f + theta d, 0),
                            r -= theta hd;   p = none

A stopped row keeps what it has; a row without information is exact zeros.  z is a descent direction of the row's quadratic
q(f) = 1/2 f^T H f - g^T f that keeps f >= 0 for a small step, p (conjugate or not) has p.r = z.z > 0 on an unchanged free set, the
free step goes to the exact minimiser of the line, and the projected step searches the segment from f to the feasible f+ exactly
and never beyond f+: q never rises and f stays >= 0.

``row`` also returns the decision trace of the row -- per step ("free", conjugate?, free set) or ("proj", conjugate?, theta >= 1?,
the j with t_j < 0, free set), or "stop" -- and its decision MARGIN: the smallest relative distance of any decision from its
threshold, |r_j| / max|g| over the j with f_j = 0 (is j free?), |t_j| / max(|f_j|, |alpha p_j|) over the j that move (is t_j < 0?),
and |theta - 1|.  A float32 run whose trace differs from the float64 one took another branch: it is another computation, not a
rounding of the same one, and only a margin near zero can make that happen.  ``dtype=np.float32`` runs the same formulas on float32
arrays, as in als_yardstick.py."""
import numpy as np

import als_yardstick as A


def row(Bs, ws, pvs, S, Nrow, l2, f, steps, dtype=np.float64):
    """(f, trace, margin, passes) of one row.  Arguments as ``als_yardstick.cg_row``."""
    z0 = dtype(0)
    f = np.maximum(np.array(f, dtype=dtype), z0)
    l2 = dtype(l2)
    trace, margin, passes = [], np.inf, 1

    def times(x):
        out = l2 * x
        for B, w in zip(Bs, ws):
            out = out + B.T @ (w * (B @ x))
        if S is not None:
            out = out + S @ x
        return out.astype(dtype)

    def near(values, scale):
        nonlocal margin
        values = np.abs(np.asarray(values, dtype=np.float64))
        scale = np.asarray(scale, dtype=np.float64)
        ok = np.broadcast_to(scale, values.shape) > 0
        if ok.any():
            margin = min(margin, float((values[ok] / np.broadcast_to(scale, values.shape)[ok]).min()))
    g = np.zeros_like(f)
    for B, pv in zip(Bs, pvs):
        g = g + B.T @ pv
    if Nrow is not None:
        g = g + Nrow
    gmax = float(np.abs(g).max()) if g.size else 0.0
    r = (g - times(f)).astype(dtype)
    p = rho_old = free_old = None
    for _ in range(int(steps)):
        free = (f > 0) | (r > 0)
        near(r[f == 0], gmax)
        z = np.where(free, r, z0)
        rho = z @ z
        if not A._good(rho):
            trace.append("stop")
            break
        conj = p is not None and bool((free == free_old).all())
        p = (z + dtype(rho / rho_old) * p).astype(dtype) if conj else z.copy()
        q = times(p)
        passes += 1
        pq = p @ q
        if not A._good(pq):
            trace.append("stop")
            break
        alpha = dtype((p @ r) / pq)
        t = (f + alpha * p).astype(dtype)
        moves = (alpha * p) != 0
        near(t[moves], np.maximum(np.abs(f), np.abs(alpha * p))[moves])
        if not (t < 0).any():
            f, r = t, (r - alpha * q).astype(dtype)
            rho_old, free_old = rho, free
            trace.append(("free", conj, tuple(np.flatnonzero(free))))
            continue
        fp = np.maximum(t, z0)
        d = (fp - f).astype(dtype)
        hd = times(d)
        passes += 1
        dhd, dr = d @ hd, d @ r
        if not (A._good(dhd) and A._good(dr)):
            trace.append("stop")
            break
        theta = dtype(dr / dhd)
        full = bool(theta >= 1)
        near([float(theta) - 1.0], 1.0)
        if full:
            f, r = fp, (r - hd).astype(dtype)
        else:
            f, r = np.maximum(f + theta * d, z0).astype(dtype), (r - theta * hd).astype(dtype)
        p = None
        trace.append(("proj", conj, full, tuple(np.flatnonzero(t < 0)), tuple(np.flatnonzero(free))))
    return f, trace, margin, passes


def rows(Rx, Ry, U, V, Z, which, l2, steps, *, cx=0.0, cy=0.0, rows=None, dtype=np.float64, order=None):
    """(F [n, k], traces [n], margins [n], passes [n]) of the rows ``rows`` (None = all) of the sweep of factor ``which``, which
    must read an observed relation.  ``order``: the order in which a row's stored entries of a side enter its sums -- None: stored
    order; "reversed"; an int: a permutation per row and side from RandomState(order).  In exact arithmetic it changes nothing; in
    float32 it is another association of the same sums, which is what separates the device from NumPy."""
    F = np.asarray({"U": U, "V": V, "Z": Z}[which], dtype=dtype)
    sel = np.arange(F.shape[0]) if rows is None else np.asarray(rows)
    obs = A._observed_sides(Rx, Ry, U, V, Z, which, cx, cy, dtype)
    assert obs, "the sweep of %s reads no observed relation" % which
    S, Nf = A.shared(Rx, Ry, U, V, Z, which, cx=cx, cy=cy, rows=sel, dtype=dtype)
    out = np.zeros((len(sel), F.shape[1]), dtype=dtype)
    traces, margins, passes = [], np.full(len(sel), np.inf), np.zeros(len(sel), dtype=np.int64)
    rng = np.random.RandomState(order) if isinstance(order, int) else None
    for n, i in enumerate(sel):
        Bs, es, pvs = [], [], []
        for B, indptr, idx, pv, e in obs:
            a, b = indptr[i], indptr[i + 1]
            at = np.arange(a, b)
            at = at if order is None else (at[::-1] if rng is None else at[rng.permutation(b - a)])
            Bs.append(B[idx[at]])
            es.append(e[at])
            pvs.append(pv[at])
        if S is None and sum(len(e) for e in es) == 0:       # a row without information
            traces.append([])
            continue
        out[n], tr, margins[n], passes[n] = row(Bs, es, pvs, S, None if Nf is None else Nf[n], l2, F[i], steps, dtype)
        traces.append(tr)
    return out, traces, margins, passes


def sweep(Rx, Ry, U, V, Z, which, l2, *, non_negative=False, nn_sweeps=0, cg_steps=0, nn_cg_steps=0, cx=0.0, cy=0.0, rows=None,
          dtype=np.float64):
    """``als_yardstick.sweep``, except that a non-negative factor with an observed relation takes the new route under
    ``nn_cg_steps > 0`` (the device's als_step)."""
    if non_negative and nn_cg_steps and A.observed(Rx, Ry, which):
        return globals()["rows"](Rx, Ry, U, V, Z, which, l2, nn_cg_steps, cx=cx, cy=cy, rows=rows, dtype=dtype)[0]
    return A.sweep(Rx, Ry, U, V, Z, which, l2, non_negative=non_negative, nn_sweeps=nn_sweeps, cg_steps=cg_steps, cx=cx, cy=cy, rows=rows,
                   dtype=dtype)


def step(X, Y, Wx, Wy, U, V, Z, l2, *, mask=7, nn_mask=0, nn_sweeps=0, cg_steps=0, nn_cg_steps=0, cx=0.0, cy=0.0, dtype=np.float64):
    """One iteration V, U, Z as ``als_yardstick.step``."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    F = {w: np.array(M, dtype=dtype) for w, M in zip("UVZ", (U, V, Z))}
    for w, bit in (("V", A.V_BIT), ("U", A.U_BIT), ("Z", A.Z_BIT)):
        if mask & bit:
            F[w] = sweep(Rx, Ry, F["U"], F["V"], F["Z"], w, l2, non_negative=bool(nn_mask & bit), nn_sweeps=nn_sweeps, cg_steps=cg_steps,
                         nn_cg_steps=nn_cg_steps, cx=cx, cy=cy, dtype=dtype)
    return F["U"], F["V"], F["Z"]


def fit(X, Y, Wx, Wy, U, V, Z, max_iter, l2, *, mask=7, nn_mask=0, nn_sweeps=0, cg_steps=0, nn_cg_steps=0, cx=0.0, cy=0.0,
        dtype=np.float64, trace=None):
    """``max_iter`` iterations without a stopping test; ``trace`` (a list) receives the objective after every iteration."""
    Rx, Ry = A.as_relation(X, Wx), A.as_relation(Y, Wy)
    for _ in range(max_iter):
        U, V, Z = step(Rx, Ry, None, None, U, V, Z, l2, mask=mask, nn_mask=nn_mask, nn_sweeps=nn_sweeps, cg_steps=cg_steps,
                       nn_cg_steps=nn_cg_steps, cx=cx, cy=cy, dtype=dtype)
        if trace is not None:
            trace.append(A.objective(Rx, Ry, None, None, U, V, Z, l2, cx=cx, cy=cy))
    return U, V, Z


def quadratic(H, g, F):
    """1/2 f^T H f - g^T f of every row, float64."""
    F = np.asarray(F, dtype=np.float64)
    return 0.5 * np.einsum("ni,nij,nj->n", F, H, F) - np.einsum("ni,ni->n", g, F)
