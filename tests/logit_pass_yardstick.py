"""NumPy yardstick of the logistic loss of the ALS solver on every route (helper of test_als_logit_pass_host.py /
test_gpu_als_logit_pass.py; not collected).

With xi the score under the current row, the Jaakkola-Jordan bound (logit_yardstick.py) makes the majoriser of a row the ALS row
problem under  w kappa(xi)  for w and  w t - w / 2  for w t.  So nothing is solved here: ``reweighted`` writes a logistic relation
as the Frobenius relation with the weights  w kappa  and the targets  (w t - w / 2) / (w kappa)  (0 where the weight is 0), both
taken at the given factors, and ``sweep`` hands the reweighted relations to the yardsticks of the routes -- ``nncg_yardstick.sweep``
(exact, coordinate descent, conjugate gradients signed and projected) and ``als_dual_yardstick.dual_rows`` -- in front of every
sweep, as the device runs its reweighting pass (cmf_set_logit_pass).  The objective and the loss are logit_yardstick's.

``dtype=np.float32`` runs the score, kappa and the products in float32 as well (and then the routes' own float32 forms): it exists
only to size the tolerances of the device tests by ``als_yardstick.tolerance``."""
import copy

import numpy as np

import als_yardstick as A
import nncg_yardstick as N
import als_dual_yardstick as D
import logit_yardstick as L

U_BIT, V_BIT, Z_BIT = A.U_BIT, A.V_BIT, A.Z_BIT


def scores(rel, Fa, Fb, dtype=np.float64):
    """a.b on the stored entries of an observed relation (pattern order), Fa / Fb the factors of its rows / columns."""
    Fa, Fb = np.asarray(Fa, dtype=dtype), np.asarray(Fb, dtype=dtype)
    return np.einsum("ij,ij->i", Fa[rel.r], Fb[rel.c]).astype(dtype)


def weights(rel, Fa, Fb, dtype=np.float64):
    """(hw, hp) in pattern order: w kappa at the current scores, and w t - w / 2 (each product rounded once in ``dtype``)."""
    w, t = rel.w.astype(dtype), rel.t.astype(dtype)
    hw = (w * L.kappa(scores(rel, Fa, Fb, dtype), dtype)).astype(dtype)
    hp = ((w * t).astype(dtype) - (dtype(0.5) * w).astype(dtype)).astype(dtype)
    return hw, hp


def with_weights_and_targets(rel, w, t):
    """``rel`` with the weights ``w`` and the targets ``t`` (pattern order) on the same pattern, both images written."""
    out = copy.copy(rel)
    w, t = np.asarray(w, np.float64), np.asarray(t, np.float64)
    out.w, out.t = w, t
    order = np.lexsort((rel.r, rel.c))
    (ip0, c0, _, _), (ip1, r1, _, _) = rel.images
    out.images = ((ip0, c0, t, w), (ip1, r1, t[order], w[order]))
    return out


def reweighted(rel, Fa, Fb, dtype=np.float64):
    """An ``als_yardstick.Relation`` on the same pattern with the weights w kappa and the targets (w t - w / 2) / (w kappa), 0
    where the weight is 0; kappa at the factors Fa / Fb of the relation's rows / columns."""
    if not rel.observed:
        raise ValueError("a logistic relation must be observed")
    hw, hp = weights(rel, Fa, Fb, dtype)
    hw64, hp64 = hw.astype(np.float64), hp.astype(np.float64)
    t = np.divide(hp64, hw64, out=np.zeros_like(hp64), where=hw64 != 0)
    return with_weights_and_targets(rel, hw64, t)


def _reweight_both(Rx, Ry, U, V, Z, logit, dtype):
    return (reweighted(Rx, U, V, dtype) if logit[0] else Rx), (reweighted(Ry, V, Z, dtype) if logit[1] else Ry)


def sweep(Rx, Ry, U, V, Z, which, l2, *, logit=(True, False), non_negative=False, nn_sweeps=0, cg_steps=0, nn_cg_steps=0, dual_max=0,
          rows=None, dtype=np.float64):
    """The rows ``rows`` (None = all) of the swept factor ``which`` by the route the device gives it under cmf_set_logit_pass, the
    logistic relations reweighted at the current factors first."""
    Rx, Ry = _reweight_both(Rx, Ry, U, V, Z, logit, dtype)
    k = np.asarray(U if U is not None else V).shape[1]
    full = any(not rel.observed for rel, _, _, _ in A._sides(Rx, Ry, U, V, Z, which))
    how = A.route(A.observed(Rx, Ry, which), non_negative, nn_sweeps, cg_steps, nn_cg_steps, dual_max, shared_term=full, k_pad=D.k_pad(k))
    if how == A.ROWS_DUAL:
        return D.dual_rows(Rx, Ry, U, V, Z, which, l2, dual_max, rows=rows, dtype=dtype, non_negative=non_negative)
    return N.sweep(Rx, Ry, U, V, Z, which, l2, non_negative=non_negative, nn_sweeps=nn_sweeps, cg_steps=cg_steps, nn_cg_steps=nn_cg_steps,
                   rows=rows, dtype=dtype)


def step(Rx, Ry, U, V, Z, l2, *, logit=(True, False), mask=7, nn_mask=0, dtype=np.float64, **route):
    """One iteration V, U, Z; returns new (U, V, Z), the inputs are left alone.  ``route``: nn_sweeps, cg_steps, nn_cg_steps,
    dual_max."""
    F = {w: np.array(M, dtype=dtype) for w, M in zip("UVZ", (U, V, Z))}
    for w, bit in (("V", V_BIT), ("U", U_BIT), ("Z", Z_BIT)):
        if mask & bit:
            F[w] = sweep(Rx, Ry, F["U"], F["V"], F["Z"], w, l2, logit=logit, non_negative=bool(nn_mask & bit), dtype=dtype, **route)
    return F["U"], F["V"], F["Z"]


def objective(Rx, Ry, U, V, Z, l2, *, logit=(True, False)):
    return L.objective(Rx, Ry, None, None, U, V, Z, l2, logit=logit)


def fit(Rx, Ry, U, V, Z, max_iter, l2, *, logit=(True, False), mask=7, nn_mask=0, dtype=np.float64, trace=None, **route):
    """``max_iter`` iterations without a stopping test; returns (U, V, Z); ``trace`` (a list) receives the objective after every
    iteration."""
    for _ in range(max_iter):
        U, V, Z = step(Rx, Ry, U, V, Z, l2, logit=logit, mask=mask, nn_mask=nn_mask, dtype=dtype, **route)
        if trace is not None:
            trace.append(objective(Rx, Ry, U, V, Z, l2, logit=logit))
    return U, V, Z
