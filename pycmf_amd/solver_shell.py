"""Host-side solver objects: the drop-in seam of the reference.

The reference's driver builds a solver object and calls exactly one method on it,
``fit_iterative_update(X, Y, U, V, Z) -> (U, V, Z, n_iter)``
(pycmf/cmf.py:437-454).  ``HipMUSolver`` and ``HipNewtonSolver`` accept the same
constructor keywords as the reference classes (pycmf/cmf_solvers.py:98-103) and
expose the same three methods (``fit_iterative_update`` :132, ``update_step``
:124, ``compute_error`` :128), but every flop of the update runs in
libcmfhip.so on the GPU:  X and Y are uploaded once, the factors stay resident
for the whole loop, and one scalar comes back per convergence check.

Semantics kept from the reference:
* U, V, Z are mutated in place and also returned (:195, :255, :324).
* the convergence test runs every 10th iteration when tol > 0 (:175-187) with
  the same verbose print format (:178-181, :190-193).
* constructing a solver with ``random_state`` seeds NumPy's *global* RNG
  (:121-122); stochastic Newton draws its per-row samples from that stream in
  the reference's order so that results are reproducible against it.
* MU ignores alpha (its error metric uses the constructor default 0.5, :99).
"""
import numbers
import os
import time

import numpy as np

from . import _lib


LOSSES = ("frobenius", "kullback-leibler", "beta-divergence")   # of the multiplicative-update solver
ALS_LOSSES = ("frobenius", "logistic")                           # of the ALS solver
ALL_LOSSES = LOSSES + tuple(v for v in ALS_LOSSES if v not in LOSSES)
BETA_NAMES = {"frobenius": 2.0, "kullback-leibler": 1.0, "itakura-saito": 0.0}


def check_loss(loss, solver="mu", n_gpus=1):
    """Validate the ``loss`` keyword (no device is touched): 'frobenius' | 'kullback-leibler' | 'beta-divergence' | 'logistic'; the
    middle two need the MU solver and one GPU, 'logistic' the ALS solver and one GPU."""
    if not isinstance(loss, str) or loss not in ALL_LOSSES:
        raise ValueError("Invalid loss parameter: got %r instead of one of %r" % (loss, list(ALL_LOSSES)))
    if loss == "beta-divergence":
        if solver != "mu":
            raise ValueError("loss='beta-divergence' is implemented by the multiplicative-update solver only: solver='mu', got %r" % (solver,))
        if n_gpus != 1:
            raise ValueError("loss='beta-divergence' runs on one GPU: n_gpus must be 1, got %r (the sharded form is not built)" % (n_gpus,))
    if loss == "logistic":
        if solver != "als":
            raise ValueError("loss='logistic' is implemented by the alternating-least-squares solver only: solver='als', got %r" % (solver,))
        if n_gpus != 1:
            raise ValueError("loss='logistic' runs on one GPU: n_gpus must be 1, got %r (the sharded form is not built)" % (n_gpus,))
    if loss == "kullback-leibler":
        if solver != "mu":
            raise ValueError("loss='kullback-leibler' is implemented by the multiplicative-update solver only: solver='mu', got %r" % (solver,))
        if n_gpus != 1:
            raise ValueError("loss='kullback-leibler' runs on one GPU: n_gpus must be 1, got %r (the sharded form is not built)" % (n_gpus,))


def check_kl_data(X, Y):
    """The generalised Kullback-Leibler divergence is defined for non-negative data only."""
    for name, M in (("X", X), ("Y", Y)):
        if M is None:
            continue
        vals = M.data if hasattr(M, "tocsr") else np.asarray(M)
        if vals.size and vals.min() < 0:
            raise ValueError("loss='kullback-leibler' needs non-negative data: %s has negative entries" % name)


def check_logistic(x_link="linear", y_link="linear", x_entry_weights="observed", y_entry_weights="observed", als_cg_steps=0,
                   x_background_weight=0.0, y_background_weight=0.0, x_biases=False, y_biases=False, have_x=True, have_y=True,
                   logit_pass=False):
    """What ``loss='logistic'`` (solver='als') cannot do, refused before any device is touched.  The relations whose link is 'logit'
    are the logistic ones: at least one must be; each needs entry weights that resolve to a CSR pattern (a SciPy sparse W or
    'observed' -- ``have_x`` / ``have_y``: the relation is part of the call), and takes no conjugate-gradient rows (unless
    ``logit_pass``: the reweighting pass in front of every sweep, ``als_logit_pass``), no background weight and no biases.  Returns
    (x is logistic, y is logistic)."""
    import scipy.sparse as sp
    logit = (x_link == "logit", y_link == "logit")
    if not any(logit):
        raise ValueError("loss='logistic' fits the relations whose link is 'logit': x_link or y_link must be 'logit', got x_link=%r, "
                         "y_link=%r" % (x_link, y_link))
    if als_cg_steps and not logit_pass:
        raise ValueError("als_cg_steps=%r with loss='logistic' is not built (the conjugate-gradient rows have no reweighting pass): "
                         "als_cg_steps must be 0; use the exact rows or als_nn_sweeps" % (als_cg_steps,))
    for name, on, have, W, c0, biases in (("x", logit[0], have_x, x_entry_weights, x_background_weight, x_biases),
                                          ("y", logit[1], have_y, y_entry_weights, y_background_weight, y_biases)):
        if not on or not have:
            continue
        if W is None or not (isinstance(W, str) or sp.issparse(W)):
            raise ValueError("loss='logistic' with %s_link='logit' needs %s_entry_weights that name the observed entries: pass a SciPy sparse "
                             "W or 'observed', got %s; the logistic loss over every cell is not built"
                             % (name, name, "None" if W is None else "a dense array"))
        if c0:
            raise ValueError("%s_background_weight=%r on a logistic relation (%s_link='logit') is not built: it must be 0" % (name, c0, name))
        if biases:
            raise ValueError("%s_biases=True on a logistic relation (%s_link='logit') is not built: it must be False" % (name, name))
    return logit


def check_logistic_data(values, name):
    """The targets of a logistic relation (``name`` 'X' | 'Y': the values on its observed entries) must lie in [0, 1]; soft labels
    are allowed."""
    v = np.asarray(values, dtype=np.float64)
    if v.size and not (np.isfinite(v).all() and v.min() >= 0.0 and v.max() <= 1.0):
        raise ValueError("loss='logistic' needs targets in [0, 1]: the observed entries of %s range over [%g, %g]" % (name, np.nanmin(v), np.nanmax(v)))


def check_beta(beta_loss):
    """``beta_loss`` under ``loss='beta-divergence'`` as a float: 'frobenius' (2) | 'kullback-leibler' (1) | 'itakura-saito' (0) or
    a finite number in [0, 2]; no device is touched."""
    if isinstance(beta_loss, str):
        if beta_loss not in BETA_NAMES:
            raise ValueError("Invalid beta_loss parameter: got %r instead of one of %r, or a number in [0, 2]" % (beta_loss, list(BETA_NAMES)))
        return BETA_NAMES[beta_loss]
    if isinstance(beta_loss, (bool, np.bool_)) or not isinstance(beta_loss, (numbers.Real, np.integer, np.floating)):
        raise ValueError("Invalid beta_loss parameter: got %r instead of one of %r, or a number in [0, 2]" % (beta_loss, list(BETA_NAMES)))
    beta = float(beta_loss)
    if not np.isfinite(beta) or beta < 0 or beta > 2:
        raise ValueError("loss='beta-divergence' is built for beta_loss in [0, 2], got %r" % (beta_loss,))
    return beta


def check_beta_extras(x_entry_weights=None, y_entry_weights=None, x_background_weight=0.0, y_background_weight=0.0, x_biases=False, y_biases=False):
    """Entry weights, background weights and biases belong to the Frobenius objective: none of them with loss='beta-divergence'."""
    for name, v in (("x_entry_weights", x_entry_weights), ("y_entry_weights", y_entry_weights)):
        if v is not None:
            raise ValueError("%s is implemented for loss='frobenius' only, not with loss='beta-divergence'" % name)
    for name, v in (("x_background_weight", x_background_weight), ("y_background_weight", y_background_weight), ("x_biases", x_biases), ("y_biases", y_biases)):
        if v:
            raise ValueError("%s belongs to solver='als' and the Frobenius objective: it must stay %r with loss='beta-divergence'" % (name, type(v)(0)))


def check_beta_data(X, Y, beta, read_x=True, read_y=True):
    """The beta-divergence needs non-negative data, and at beta = 0 (Itakura-Saito) no zero in any relation a sweep reads -- the
    divergence is infinite there; a SciPy-sparse relation has implicit zeros (sklearn refuses the same case)."""
    for name, M, read in (("X", X, read_x), ("Y", Y, read_y)):
        if M is None:
            continue
        sparse = hasattr(M, "tocsr")
        vals = M.data if sparse else np.asarray(M)
        if vals.size and vals.min() < 0:
            raise ValueError("loss='beta-divergence' needs non-negative data: %s has negative entries" % name)
        if beta == 0 and read:
            if sparse and M.nnz < M.shape[0] * M.shape[1]:
                raise ValueError("beta_loss=0 (Itakura-Saito) needs strictly positive data: %s is sparse, its implicit zeros make the divergence infinite" % name)
            if vals.size and vals.min() <= 0:
                raise ValueError("beta_loss=0 (Itakura-Saito) needs strictly positive data: %s has zeros, which make the divergence infinite" % name)


class EntryWeights:
    """Per-entry weights of one relation as the device takes them.  ``kind`` 'dense': ``W`` and ``data`` are dense float64 arrays of
    the relation's shape (a sparse relation densified on the host).  ``kind`` 'csr': the observed pattern ``indptr`` / ``indices``
    with the relation's values ``t`` and the weights ``w`` on it, stored zeros of either included."""

    def __init__(self, kind, W=None, data=None, indptr=None, indices=None, t=None, w=None):
        self.kind, self.W, self.data, self.indptr, self.indices, self.t, self.w = kind, W, data, indptr, indices, t, w


def _canonical_csr(A):
    A = A.tocsr()
    if not A.has_canonical_format:
        A = A.copy()               # never canonicalise the caller's matrix in place
        A.sum_duplicates()         # (keeps explicit zeros: a stored zero stays an observed entry)
    return A


def _check_weight_values(vals, name):
    vals = np.asarray(vals, dtype=np.float64)
    if vals.size and not np.isfinite(vals).all():
        raise ValueError("%s_entry_weights must be finite: found NaN or infinite weights" % name)
    if vals.size and vals.min() < 0:
        raise ValueError("%s_entry_weights must be non-negative: found negative weights" % name)
    return vals


def resolve_entry_weights(M, W, name):
    """Validate the weights ``W`` of relation ``M`` (``name`` 'x' | 'y') and put them in the form the device takes; no device is
    touched.  ``W``: None | dense array of M's shape | SciPy sparse matrix (its stored pattern is the observed set, its values the
    weights) | 'observed' (M must be SciPy sparse: its stored entries, explicit zeros included, carry weight 1)."""
    import scipy.sparse as sp
    if W is None:
        return None
    if M is None:
        raise ValueError("%s_entry_weights given for a relation that is not" % name)
    if isinstance(W, str):
        if W != "observed":
            raise ValueError("%s_entry_weights: got %r instead of an array, a SciPy sparse matrix, 'observed' or None" % (name, W))
        if not sp.issparse(M):
            raise ValueError("%s_entry_weights='observed' needs a SciPy sparse %s (its stored entries are the observed ones); "
                             "for a dense relation pass a 0/1 array" % (name, name.upper()))
        A = _canonical_csr(M)
        return EntryWeights("csr", indptr=A.indptr.astype(np.int64), indices=A.indices.astype(np.int32),
                            t=np.asarray(A.data, dtype=np.float64), w=np.ones(A.nnz))
    if sp.issparse(W):
        if W.shape != M.shape:
            raise ValueError("%s_entry_weights has shape %s, the relation %s" % (name, W.shape, M.shape))
        P = _canonical_csr(W)
        w = _check_weight_values(P.data, name)
        rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
        if sp.issparse(M):
            t = np.asarray(M.tocsr()[rows, P.indices], dtype=np.float64).ravel() if P.nnz else np.zeros(0)
        else:
            t = np.asarray(M, dtype=np.float64)[rows, P.indices]
        return EntryWeights("csr", indptr=P.indptr.astype(np.int64), indices=P.indices.astype(np.int32), t=t, w=w)
    W = np.asarray(W)
    if W.dtype.kind not in "fiub":
        raise ValueError("%s_entry_weights: got an array of dtype %s instead of numbers" % (name, W.dtype))
    if W.shape != M.shape:
        raise ValueError("%s_entry_weights has shape %s, the relation %s" % (name, W.shape, M.shape))
    W = _check_weight_values(W, name)
    return EntryWeights("dense", W=W, data=(M.toarray() if sp.issparse(M) else M))


def check_entry_weights(x_entry_weights, y_entry_weights, solver="mu", loss="frobenius", n_gpus=1):
    """Per-entry weights need the multiplicative-update solver (or solver='als'), the Frobenius loss and one GPU (no device is
    touched)."""
    if x_entry_weights is None and y_entry_weights is None:
        return
    if solver not in ("mu", "als"):
        raise ValueError("x_entry_weights / y_entry_weights are implemented by the multiplicative-update solver only: solver='mu', got %r" % (solver,))
    if loss not in ("frobenius", "logistic"):
        raise ValueError("x_entry_weights / y_entry_weights are implemented for loss='frobenius' only, got %r" % (loss,))
    if n_gpus != 1:
        raise ValueError("x_entry_weights / y_entry_weights run on one GPU: n_gpus must be 1, got %r (the sharded form is not built)" % (n_gpus,))


def check_background_weight(value, name, solver="als", entry_weights="observed"):
    """``x_background_weight`` / ``y_background_weight`` (``name`` 'x' | 'y'): a finite number >= 0, non-zero with solver='als' only
    and only for a relation whose entry weights are a SciPy sparse W or 'observed' (``entry_weights``: what the call was given).
    Returns the value as a float; no device is touched."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (numbers.Real, np.integer, np.floating)):
        raise ValueError("%s_background_weight must be a finite number >= 0, got %r" % (name, value))
    value = float(value)
    if not np.isfinite(value) or value < 0:
        raise ValueError("%s_background_weight must be a finite number >= 0, got %r" % (name, value))
    if value == 0:
        return 0.0
    if solver != "als":
        raise ValueError("%s_background_weight is the implicit-feedback model of solver='als': it must be 0 with solver=%r, got %r" % (name, solver, value))
    if entry_weights is None:
        raise ValueError("%s_background_weight=%r needs %s_entry_weights: the confidences of the stored entries (a SciPy sparse W, or "
                         "'observed'); without them every cell already counts with weight 1" % (name, value, name))
    import scipy.sparse as sp
    if not (isinstance(entry_weights, str) or sp.issparse(entry_weights)):
        raise ValueError("%s_background_weight=%r with dense %s_entry_weights: the background is the weight of the cells OUTSIDE a stored "
                         "pattern, which a dense W does not have; pass a SciPy sparse W or 'observed'" % (name, value, name))
    return value


def check_huber_delta(value, name, solver="als", n_gpus=1, entry_weights="observed", link="linear", background_weight=0.0, have=True):
    """``x_huber_delta`` / ``y_huber_delta`` (``name`` 'x' | 'y'): None, or a finite number > 0 -- with solver='als' on one GPU only,
    and (``have``: the relation is part of the call) for a relation with a linear link whose entry weights are a SciPy sparse W or
    'observed' and that has no background weight.  Returns None or the value as a float; no device is touched."""
    if value is None:
        return None
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (numbers.Real, np.integer, np.floating)):
        raise ValueError("%s_huber_delta must be None or a finite number > 0, got %r" % (name, value))
    value = float(value)
    if not np.isfinite(value) or not value > 0 or not np.isfinite(np.float32(value)) or not np.float32(value) > 0:
        raise ValueError("%s_huber_delta must be None or a finite number > 0, got %r" % (name, value))
    if solver != "als":
        raise ValueError("%s_huber_delta is the Huber loss of solver='als': it must be None with solver=%r, got %r" % (name, solver, value))
    if n_gpus != 1:
        raise ValueError("%s_huber_delta runs on one GPU: n_gpus must be 1, got %r (the sharded form is not built)" % (name, n_gpus))
    if not have:
        return value
    import scipy.sparse as sp
    if entry_weights is None or not (isinstance(entry_weights, str) or sp.issparse(entry_weights)):
        raise ValueError("%s_huber_delta=%r needs %s_entry_weights that name the observed entries: pass a SciPy sparse W or 'observed', got "
                         "%s; the Huber loss over every cell is not built" % (name, value, name, "None" if entry_weights is None else "a dense array"))
    if link == "logit":
        raise ValueError("%s_huber_delta=%r on a relation with %s_link='logit' is not built: the Huber loss is a loss of the linear link"
                         % (name, value, name))
    if background_weight:
        raise ValueError("%s_huber_delta=%r together with %s_background_weight=%r is not built: the Huber loss runs over the stored "
                         "entries only" % (name, value, name, background_weight))
    return value


def check_biases(flag, name, solver="als", entry_weights="observed", background_weight=0.0):
    """``x_biases`` / ``y_biases`` (``name`` 'x' | 'y'): a bool; True with solver='als' only, for a relation whose entry weights
    resolve to a CSR pattern (a SciPy sparse W or 'observed') and that has no background weight.  Returns the flag as a bool; no
    device is touched."""
    if not isinstance(flag, (bool, np.bool_)):
        raise ValueError("%s_biases must be True or False, got %r" % (name, flag))
    if not flag:
        return False
    if solver != "als":
        raise ValueError("%s_biases is the rating model of solver='als' (mu + row bias + column bias + u.v): it must be False with "
                         "solver=%r; pass solver='als'" % (name, solver))
    import scipy.sparse as sp
    if entry_weights is None or not (isinstance(entry_weights, str) or sp.issparse(entry_weights)):
        raise ValueError("%s_biases=True needs %s_entry_weights that name the observed entries: pass %s_entry_weights='observed' (a SciPy "
                         "sparse %s) or a SciPy sparse W; biases of a relation that counts in every cell are not built" % (name, name, name, name.upper()))
    if background_weight:
        raise ValueError("%s_biases=True together with %s_background_weight=%r is not built: pass %s_background_weight=0 (ratings), or "
                         "%s_biases=False (implicit feedback)" % (name, name, background_weight, name, name))
    return True


def check_bias_l2(bias_l2):
    """``bias_l2``: None (the fit's l2_reg) or a finite number >= 0; returns it as None or a float.  No device is touched."""
    if bias_l2 is None:
        return None
    if isinstance(bias_l2, (bool, np.bool_)) or not isinstance(bias_l2, (numbers.Real, np.integer, np.floating)) or \
            not np.isfinite(float(bias_l2)) or float(bias_l2) < 0:
        raise ValueError("bias_l2 must be None (use l2_reg) or a finite number >= 0, got %r; pass bias_l2=0 for unregularised biases" % (bias_l2,))
    return float(bias_l2)


def _check_bias_init(init, shape, name):
    """A starting point (offset, rows, cols) of a relation's biases -- rows / cols may be None (zeros) -- as float64."""
    if init is None:
        return None
    offset, rows, cols = init
    out = [float(offset)]
    if not np.isfinite(out[0]):
        raise ValueError("%s_bias_init: the offset must be finite, got %r" % (name, offset))
    for v, n, what in ((rows, shape[0], "rows"), (cols, shape[1], "cols")):
        v = np.zeros(n) if v is None else np.asarray(v, dtype=np.float64).ravel()
        if v.shape != (n,) or not np.isfinite(v).all():
            raise ValueError("%s_bias_init: %s must hold %d finite values" % (name, what, n))
        out.append(v)
    return tuple(out)


def check_background_floor(ew, value, name):
    """Every stored weight of the resolved ``ew`` must be >= the background weight, compared as the device does, in float32."""
    if not value or ew is None:
        return
    w = np.asarray(ew.w, dtype=np.float32)
    if w.size and w.min() < np.float32(value):
        raise ValueError("%s_entry_weights has a stored weight %r below %s_background_weight=%r: a stored entry must count at least as "
                         "much as an unobserved cell" % (name, float(w.min()), name, value))


def implicit_confidence(R, alpha=1.0, background=1.0):
    """``(P, W)`` of the implicit-feedback model for a SciPy sparse matrix ``R`` of counts (clicks, plays, purchases): ``P`` is the
    pattern of R with ones (the targets), ``W = background + alpha * R`` on the same pattern (the confidences).  Fit with
    ``CMF(solver='als', ...).fit(P, Y, x_entry_weights=W, x_background_weight=background)``.  Negative or non-finite counts are a
    ``ValueError``; stored zeros stay stored (target 1, confidence ``background``)."""
    import scipy.sparse as sp
    if not sp.issparse(R):
        raise ValueError("implicit_confidence takes a SciPy sparse matrix of counts, got %s" % type(R).__name__)
    for v, nm in ((alpha, "alpha"), (background, "background")):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
            raise ValueError("implicit_confidence: %s must be a finite number >= 0, got %r" % (nm, v))
    A = _canonical_csr(R)
    counts = np.asarray(A.data, dtype=np.float64)
    if counts.size and not np.isfinite(counts).all():
        raise ValueError("implicit_confidence: the counts must be finite: found NaN or infinite values")
    if counts.size and counts.min() < 0:
        raise ValueError("implicit_confidence: the counts must be non-negative: found negative values")
    P = sp.csr_matrix((np.ones(A.nnz), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    W = sp.csr_matrix((float(background) + float(alpha) * counts, A.indices.copy(), A.indptr.copy()), shape=A.shape)
    return P, W


def _as_f64(a):
    return a if (isinstance(a, np.ndarray) and a.dtype == np.float64) else np.asarray(a, dtype=np.float64)


class _HipIterativeSolver:
    def __init__(self, max_iter=200, tol=1e-4, beta_loss="frobenius",
                 l1_reg=0, l2_reg=0, alpha=0.5, verbose=0,
                 U_non_negative=True, V_non_negative=True, Z_non_negative=True,
                 update_U=True, update_V=True, update_Z=True,
                 x_link="linear", y_link="linear", hessian_pertubation=0.2,
                 sg_sample_ratio=1., random_state=None, device=0, stream=None, sg_sampler="numpy",
                 cython_variant=False):
        # like the reference, any beta_loss sklearn can parse is accepted and then ignored: only the
        # Frobenius objective is implemented by either solver (cmf_solvers.py:106, :166).  The one exception is
        # HipMUSolver(loss="beta-divergence"), which parses it into its attribute ``beta``
        if isinstance(beta_loss, str) and beta_loss not in ("frobenius", "kullback-leibler", "itakura-saito"):
            raise ValueError("Invalid beta_loss parameter: got %r" % (beta_loss,))
        self.max_iter = max_iter
        self.tol = tol
        self.beta_loss = 2.0
        self.l1_reg = l1_reg
        self.l2_reg = l2_reg
        self.alpha = alpha
        self.verbose = verbose
        self.U_non_negative = U_non_negative
        self.V_non_negative = V_non_negative
        self.Z_non_negative = Z_non_negative
        self.update_U = update_U
        self.update_V = update_V
        self.update_Z = update_Z
        self.x_link = x_link
        self.y_link = y_link
        self.hessian_pertubation = hessian_pertubation
        self.sg_sample_ratio = sg_sample_ratio
        self.device = device
        self.stream = stream
        if sg_sampler not in ("numpy", "device"):
            raise ValueError("sg_sampler must be 'numpy' (reference RNG stream) or 'device', got %r" % (sg_sampler,))
        self.sg_sampler = sg_sampler
        # True: numerics of the reference's (unused) Cython twin, whose Z sweep shares U's routine and
        # therefore has no l2 term in its logit Hessian (cmf_newton_solver.pyx:287-290; SURVEY N-cy1)
        self.cython_variant = bool(cython_variant)
        self._sample_seed = (int(random_state) if isinstance(random_state, (int, np.integer)) else 0) << 20
        self._ctx = None
        self._bound = None
        if random_state is not None:
            np.random.seed(random_state)

    # ------------------------------------------------------------------ device state
    def _update_mask(self):
        return (_lib.UPD_U if self.update_U else 0) | (_lib.UPD_V if self.update_V else 0) | \
            (_lib.UPD_Z if self.update_Z else 0)

    def _nn_mask(self):
        return (1 if self.U_non_negative else 0) | (2 if self.V_non_negative else 0) | \
            (4 if self.Z_non_negative else 0)

    def bind_data(self, X, Y, k):
        """Upload X and Y ahead of the factors (the initialisers use the device copies)."""
        m = X.shape[0] if X is not None else None
        d = X.shape[1] if X is not None else Y.shape[0]
        p = Y.shape[1] if Y is not None else None
        if m is None or p is None:
            return None
        return self._bind_dims(X, Y, m, d, p, k)

    def _bind(self, X, Y, U, V, Z):
        """Upload X, Y (once per distinct pair) and size the device problem."""
        m, k = U.shape
        return self._bind_dims(X, Y, m, V.shape[0], Z.shape[0], k)

    def rebind(self):
        """Forget the uploaded X / Y: the next call uploads them again.  The device copies are cached by the
        IDENTITY of the arrays (``id(X), id(Y)`` and the shapes), which is what lets a loop of ``update_step`` /
        ``compute_error`` calls on the same matrices (tests/test_cmf.py:126-162 upstream) pay one upload; a caller
        who edits X or Y IN PLACE between calls must call this (the reference re-reads X on every call)."""
        self._bound = None

    def _bind_dims(self, X, Y, m, d, p, k):
        key = (id(X), id(Y), m, d, p, k) + self._weights_key()
        if getattr(self, "loss", "frobenius") == "kullback-leibler" and self._bound != key:
            check_kl_data(X, Y)
        if getattr(self, "loss", "frobenius") == "beta-divergence" and self._bound != key:
            check_beta_data(X, Y, self.beta, self.update_U or self.update_V, self.update_Z or self.update_V)
        wx, wy = self._resolve_weights(X, Y) if self._bound != key else (None, None)   # ValueError before any device is opened
        if self._ctx is None:
            self._ctx = _lib.Context(self.device, self.stream)
            mode = os.environ.get("PYCMF_AMD_SPARSE_MODE")  # "dense" | "native": override the auto choice
            if mode:
                self._ctx.set_option("sparse_mode", {"auto": 0, "dense": 1, "native": 2}[mode])
            if self.cython_variant:
                self._ctx.set_option("z_logit_hessian_l2", 0)
            if os.environ.get("PYCMF_AMD_GEMM_ARITH") == "bf16x6":  # opt-in arithmetic of the k_pad = 256 data passes
                self._ctx.set_option("gemm_arith", 1)
            if os.environ.get("PYCMF_AMD_REFINE_ROWS") == "0":  # A/B: leave ill-conditioned clamped rows in float32 (recorded, warned)
                self._ctx.set_option("refine_rows", 0)
        if self._bound != key:
            self._ctx.set_problem(m, d, p, k)
            weighted = wx is not None or wy is not None
            for which, M, name, shape, ew in ((0, X, "X", (m, d), wx), (1, Y, "Y", (d, p), wy)):
                if M is None:
                    continue
                if M.shape != shape:
                    raise ValueError("%s has shape %s, factors imply %s" % (name, M.shape, shape))
                if ew is not None and ew.kind == "dense":
                    M = ew.data            # (a sparse relation under dense weights: densified on the host)
                elif weighted and ew is None and hasattr(M, "tocsr") and self._densify_unweighted:
                    M = M.toarray()        # the unweighted side of a weighted fit takes part with W = 1 through its dense image
                elif getattr(self, "_beta_path", False) and hasattr(M, "tocsr"):
                    M = M.toarray()        # the beta-divergence passes read the dense image: the denominator needs every cell
                self._ctx.set_data(which, M)
                if ew is not None and ew.kind == "dense":
                    self._ctx.set_weight(which, ew.W)
                elif ew is not None:
                    self._ctx.set_weighted_csr(which, ew.indptr, ew.indices, ew.t, ew.w)
            self._bound = key
            self._XY = (X, Y)  # keep ids alive
        return self._ctx

    #: the weighted MU passes read an unweighted relation through its dense image; a solver that takes it in any layout says False
    _densify_unweighted = True

    def _weights_key(self):
        return ()

    def _resolve_weights(self, X, Y):
        return None, None

    def _push_factors(self, U, V, Z):
        self._ctx.set_factor(_lib.CMF_U, U)
        self._ctx.set_factor(_lib.CMF_V, V)
        self._ctx.set_factor(_lib.CMF_Z, Z)

    def _pull_factors(self, U, V, Z):
        for which, F in ((_lib.CMF_U, U), (_lib.CMF_V, V), (_lib.CMF_Z, Z)):
            if isinstance(F, np.ndarray) and F.dtype == np.float64 and F.flags.writeable:
                self._ctx.get_factor_into(which, F)
            else:
                F[...] = self._ctx.get_factor(which)

    def release(self):
        if self._ctx is not None:
            self._ctx.close()
        self._ctx = None
        self._bound = None

    # ------------------------------------------------------------------ reference API
    def _device_step(self, l1_reg, l2_reg, alpha):
        raise NotImplementedError("Implement in concrete subclass to use")

    def update_step(self, X, Y, U, V, Z, l1_reg, l2_reg, alpha):
        """One sweep over all factors, in place on U, V, Z (cmf_solvers.py:124)."""
        self._bind(X, Y, U, V, Z)
        self._push_factors(U, V, Z)
        self._device_step(l1_reg, l2_reg, alpha)
        self._pull_factors(U, V, Z)

    def _device_step_error(self, l1_reg, l2_reg, alpha):
        """One update step AND (||X - f(UV^T)||_F, ||Y - f(VZ^T)||_F) of its result in one device call, or None where the solver has
        no such call (then the caller runs the step and the error pass separately)."""
        return None

    def _device_error(self):
        ex2, ey2 = self._ctx.residual_sq(self.x_link, self.y_link)
        X, Y = self._XY
        ex = np.sqrt(ex2) if X is not None else 0.0
        ey = np.sqrt(ey2) if Y is not None else 0.0
        return ex, ey

    def compute_error(self, X, Y, U, V, Z):
        """alpha*||X - f(UV^T)||_F + (1-alpha)*||Y - f(VZ^T)||_F (cmf_solvers.py:128-130)."""
        self._bind(X, Y, U, V, Z)
        self._push_factors(U, V, Z)
        ex, ey = self._device_error()
        return self.alpha * ex + (1 - self.alpha) * ey

    def reconstruction_error(self):
        """||X - f(UV^T)||_F + ||Y - f(VZ^T)||_F with the factors currently on the
        device (pycmf/cmf.py:697-698)."""
        ex, ey = self._device_error()
        return ex + ey

    def _run_params(self):
        """Keyword arguments of Context.run for this solver, or None when the loop has to stay on the host (index lists drawn from
        NumPy's stream)."""
        raise NotImplementedError("Implement in concrete subclass to use")

    def fit_iterative_update(self, X, Y, U, V, Z):
        """Alternating minimisation loop (cmf_solvers.py:132-195).  The loop itself runs inside libcmfhip (``cmf_run``: error at
        init, one step per iteration, the check every 10th iteration, early stop) unless the per-row samples come from NumPy's
        global stream, which only the host can draw from; the verbose lines of the reference are printed from the trace the
        C loop returns (same text, same elapsed times, after the loop instead of during it)."""
        start_time = time.time()
        self._bind(X, Y, U, V, Z)
        self._push_factors(U, V, Z)
        self._fit_begin()
        params = self._run_params()
        if params is not None and os.environ.get("PYCMF_AMD_HOST_LOOP") != "1":
            before_run = time.time() - start_time      # upload and binding: part of the reference's clock (it starts at :144)
            n_iter, errs, secs = self._ctx.run(max_iter=self.max_iter, tol=self.tol, **params)
            self._after_run(n_iter)
            if self.verbose:
                every = int(params.get("check_every", 10))
                for i, (e, t) in enumerate(zip(errs[1:], secs[1:]), start=1):
                    print("Epoch %02d reached after %.3f seconds, error: %f" % (every * i, before_run + t, e))
                if self.tol == 0 or n_iter % every != 0:
                    print("Epoch %02d reached after %.3f seconds." % (n_iter, time.time() - start_time))
            self._fit_end()
            self._pull_factors(U, V, Z)
            return U, V, Z, n_iter
        ex, ey = self._device_error()
        previous_error = error_at_init = self.alpha * ex + (1 - self.alpha) * ey

        n_iter = 0
        for n_iter in range(1, self.max_iter + 1):
            check = self.tol > 0 and n_iter % 10 == 0
            # (MU: the check iteration is ONE call -- the step and the error of its result from the step's own products,
            # cmf_mu_step_error -- exactly what the C loop runs, so the two loops stay launch for launch the same)
            fused = self._device_step_error(self.l1_reg, self.l2_reg, self.alpha) if check else None
            if fused is None:
                self._device_step(self.l1_reg, self.l2_reg, self.alpha)
            if check:
                ex, ey = fused if fused is not None else self._device_error()
                error = self.alpha * ex + (1 - self.alpha) * ey
                if self.verbose:
                    print("Epoch %02d reached after %.3f seconds, error: %f" %
                          (n_iter, time.time() - start_time, error))
                if (previous_error - error) / error_at_init < self.tol:
                    break
                previous_error = error

        if self.verbose and (self.tol == 0 or n_iter % 10 != 0):
            self._ctx.sync()
            print("Epoch %02d reached after %.3f seconds." % (n_iter, time.time() - start_time))

        self._fit_end()
        self._pull_factors(U, V, Z)
        return U, V, Z, n_iter

    def _after_run(self, n_iter):
        pass

    def _fit_begin(self):
        pass

    def _fit_end(self):
        pass


class HipMUSolver(_HipIterativeSolver):
    """Multiplicative updates V -> U -> Z (pycmf/cmf_solvers.py:198-263) on the GPU.

    ``loss='kullback-leibler'`` (``beta_loss`` keeps its reference meaning: parsed, ignored): the same sweep order on the
    generalised Kullback-Leibler objective D(X || U V^T) + D(Y || V Z^T) -- sklearn's multiplicative update for beta_loss = 1 per
    block (``cmf_mu_kl_step``).  The error metric is then what ``compute_factorization_error`` would return under beta_loss = 1,
    sqrt(2 D) per side; the loop stays on the host (``cmf_run`` knows the Frobenius steps only).

    ``x_entry_weights`` / ``y_entry_weights`` (``resolve_entry_weights``): fixed non-negative weights per entry of X / Y on the
    Frobenius objective, 1/2 |sqrt(Wx) .* (X - U V^T)|^2 + 1/2 |sqrt(Wy) .* (Y - V Z^T)|^2 (``cmf_mu_weighted_step``); a 0/1 mask
    or ``'observed'`` fits the observed entries only.  The error metric weighs the residuals the same way; the loop stays on the
    host.

    ``loss='beta-divergence'``: here, and only here, ``beta_loss`` means something -- 'itakura-saito' (0), 'kullback-leibler' (1),
    'frobenius' (2) or a number in [0, 2], kept in the attribute ``beta`` (``beta_loss`` itself stays the constant 2.0).  The same
    sweep order on D_beta(X || U V^T) + D_beta(Y || V Z^T) by sklearn's multiplicative update for that beta per block
    (``cmf_mu_beta_step``: numerator and denominator from one fused dual-output pass); beta = 1 and beta = 2 are handed to the
    Kullback-Leibler and Frobenius paths above and give their results bit for bit.  Dense images only (a sparse relation is
    uploaded dense); no entry weights.  The error metric is sqrt(2 D_beta) per side; the loop stays on the host."""

    def __init__(self, *args, loss="frobenius", x_entry_weights=None, y_entry_weights=None, **kwargs):
        check_loss(loss)
        self.beta = None
        if loss == "beta-divergence":
            self.beta = check_beta(kwargs.get("beta_loss", args[2] if len(args) > 2 else "frobenius"))
            check_beta_extras(x_entry_weights, y_entry_weights)
        check_entry_weights(x_entry_weights, y_entry_weights, "mu", "frobenius" if loss == "beta-divergence" else loss)
        super().__init__(*args, **kwargs)
        self.loss = loss
        # which device path a step takes: beta = 2 and beta = 1 ARE the Frobenius and Kullback-Leibler paths
        self._path = loss if loss != "beta-divergence" else {2.0: "frobenius", 1.0: "kullback-leibler"}.get(self.beta, "beta-divergence")
        self._beta_path = self._path == "beta-divergence"
        self.x_entry_weights = x_entry_weights
        self.y_entry_weights = y_entry_weights
        self._weighted = x_entry_weights is not None or y_entry_weights is not None

    def _weights_key(self):
        return (id(self.x_entry_weights), id(self.y_entry_weights)) if self._weighted else ()

    def _resolve_weights(self, X, Y):
        key = (id(X), id(Y))
        if getattr(self, "_resolved_for", None) != key:
            self._resolved = (resolve_entry_weights(X, self.x_entry_weights, "x"), resolve_entry_weights(Y, self.y_entry_weights, "y"))
            self._resolved_for, self._resolved_keep = key, (X, Y)
        return self._resolved

    def check_weights(self, X, Y):
        """Raise the ValueError of unusable weights now, before any device is opened."""
        self._resolve_weights(X, Y)

    def _device_step(self, l1_reg, l2_reg, alpha):
        if self._weighted:
            self._ctx.mu_weighted_step(l1_reg, l2_reg, self._update_mask())
            return
        if self._path == "kullback-leibler":
            self._ctx.mu_kl_step(l1_reg, l2_reg, self._update_mask())
            return
        if self._beta_path:
            self._ctx.mu_beta_step(self.beta, l1_reg, l2_reg, self._update_mask())
            return
        self._ctx.mu_step(l1_reg, l2_reg, self._update_mask())

    def _device_error(self):
        if self._weighted:
            X, Y = self._XY
            ex2, ey2 = self._ctx.weighted_residual_sq(X is not None, Y is not None)
            return np.sqrt(max(ex2, 0.0)), np.sqrt(max(ey2, 0.0))
        if self._path == "frobenius":
            return super()._device_error()
        X, Y = self._XY
        if self._beta_path:
            dx, dy = self._ctx.beta_divergence(self.beta, X is not None, Y is not None)
        else:
            dx, dy = self._ctx.kl_divergence(X is not None, Y is not None)
        return np.sqrt(2.0 * max(dx, 0.0)), np.sqrt(2.0 * max(dy, 0.0))

    def _device_step_error(self, l1_reg, l2_reg, alpha):
        if self._path != "frobenius" or self._weighted:
            return None
        ex2, ey2 = self._ctx.mu_step_error(l1_reg, l2_reg, self._update_mask())
        X, Y = self._XY
        return (np.sqrt(ex2) if X is not None else 0.0), (np.sqrt(ey2) if Y is not None else 0.0)

    def _run_params(self):
        if self._path != "frobenius" or self._weighted:
            return None
        return dict(solver="mu", l1=self.l1_reg, l2=self.l2_reg, alpha_err=self.alpha, update_mask=self._update_mask())


def check_hals(U_non_negative=True, V_non_negative=True, Z_non_negative=True, n_gpus=1, n_components=None):
    """What the HALS solver cannot do, refused before any device is touched."""
    if not (U_non_negative and V_non_negative and Z_non_negative):
        raise ValueError("solver='hals' keeps every factor non-negative (that is the method): U_non_negative, V_non_negative and "
                         "Z_non_negative must be True; for signed factors use solver='newton'")
    if n_gpus != 1:
        raise ValueError("solver='hals' runs on one GPU: n_gpus must be 1, got %r (the sharded form is not built)" % (n_gpus,))
    if n_components is not None and n_components > 256:
        raise NotImplementedError("solver='hals' is built for n_components <= 256, got %d" % (n_components,))


class HipHALSSolver(_HipIterativeSolver):
    """HALS, cyclic coordinate descent on MU's objective in MU's sweep order V -> U -> Z (``cmf_hals_step``): per factor one pass
    over its k columns, every row solving its one-dimensional non-negative least-squares problems exactly -- sklearn's
    ``solver='cd'`` without shuffling, per block of the collective model.  An iteration forms the products of an MU iteration and
    needs far fewer of them.  Non-negative factors only; like MU it ignores alpha and the links.  The error metric is the
    Frobenius one; the loop stays on the host (``cmf_run`` knows the MU and Newton steps only)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        check_hals(self.U_non_negative, self.V_non_negative, self.Z_non_negative)

    def _bind_dims(self, X, Y, m, d, p, k):
        check_hals(n_components=k)
        return super()._bind_dims(X, Y, m, d, p, k)

    def _device_step(self, l1_reg, l2_reg, alpha):
        self._ctx.hals_step(l1_reg, l2_reg, self._update_mask())

    def _run_params(self):
        return None


def check_als(l1_reg=0, l2_reg=1.0, n_gpus=1, loss="frobenius", n_components=None):
    """What the ALS solver cannot do, refused before any device is touched."""
    if loss not in ALS_LOSSES:
        raise ValueError("solver='als' minimises the (weighted) Frobenius objective, or with loss='logistic' the cross-entropy of its "
                         "logit relations: loss must be 'frobenius' or 'logistic', got %r" % (loss,))
    if not l2_reg > 0:
        raise ValueError("solver='als' needs l2_reg > 0 (a row with fewer observed entries than components has a singular system "
                         "otherwise), got %r" % (l2_reg,))
    if l1_reg != 0:
        raise ValueError("solver='als' has no l1 term (its row systems are linear): l1_reg must be 0, got %r" % (l1_reg,))
    if n_gpus != 1:
        raise ValueError("solver='als' runs on one GPU: n_gpus must be 1, got %r (the sharded form is not built)" % (n_gpus,))
    if n_components is not None and n_components > 256:
        raise NotImplementedError("solver='als' is built for n_components <= 256, got %d" % (n_components,))


def check_als_nn_sweeps(als_nn_sweeps, solver="als"):
    """``als_nn_sweeps``: an integer 0 .. 1024, non-zero with solver='als' only (no device is touched)."""
    if isinstance(als_nn_sweeps, (bool, np.bool_)) or not isinstance(als_nn_sweeps, (numbers.Integral, np.integer)):
        raise ValueError("als_nn_sweeps must be an integer 0 .. 1024, got %r" % (als_nn_sweeps,))
    if als_nn_sweeps < 0 or als_nn_sweeps > 1024:
        raise ValueError("als_nn_sweeps must be an integer 0 .. 1024, got %r" % (als_nn_sweeps,))
    if als_nn_sweeps and solver != "als":
        raise ValueError("als_nn_sweeps is the non-negative row solve of solver='als': it must be 0 with solver=%r, got %r" % (solver, als_nn_sweeps))


def check_als_cg_steps(als_cg_steps, solver="als", updated_non_negative=None):
    """``als_cg_steps``: an integer 0 .. 1024, non-zero with solver='als' only and only when some updated factor is signed
    (``updated_non_negative``: the ``*_non_negative`` flags of the factors the call updates; None skips that test).  No device is
    touched."""
    if isinstance(als_cg_steps, (bool, np.bool_)) or not isinstance(als_cg_steps, (numbers.Integral, np.integer)):
        raise ValueError("als_cg_steps must be an integer 0 .. 1024, got %r" % (als_cg_steps,))
    if als_cg_steps < 0 or als_cg_steps > 1024:
        raise ValueError("als_cg_steps must be an integer 0 .. 1024, got %r" % (als_cg_steps,))
    if als_cg_steps and solver != "als":
        raise ValueError("als_cg_steps is the conjugate-gradient row solve of solver='als': it must be 0 with solver=%r, got %r" % (solver, als_cg_steps))
    if als_cg_steps and updated_non_negative is not None and all(updated_non_negative):
        raise ValueError("als_cg_steps=%r acts on signed factors only, and every factor this call updates is non-negative "
                         "(U/V/Z_non_negative=True is the default): pass *_non_negative=False, or use als_nn_sweeps" % (als_cg_steps,))


def check_als_nn_cg_steps(als_nn_cg_steps, solver="als", updated_non_negative=None, n_gpus=1, loss="frobenius", biases=False,
                          logit_pass=False):
    """``als_nn_cg_steps``: an integer 0 .. 1024; non-zero with solver='als' on one GPU only, only when some updated factor is
    non-negative (``updated_non_negative`` as in ``check_als_cg_steps``), and not with ``loss='logistic'`` (unless ``logit_pass``:
    ``als_logit_pass``) or biases.  No device is touched."""
    if isinstance(als_nn_cg_steps, (bool, np.bool_)) or not isinstance(als_nn_cg_steps, (numbers.Integral, np.integer)):
        raise ValueError("als_nn_cg_steps must be an integer 0 .. 1024, got %r" % (als_nn_cg_steps,))
    if als_nn_cg_steps < 0 or als_nn_cg_steps > 1024:
        raise ValueError("als_nn_cg_steps must be an integer 0 .. 1024, got %r" % (als_nn_cg_steps,))
    if not als_nn_cg_steps:
        return
    if solver != "als":
        raise ValueError("als_nn_cg_steps is the non-negative conjugate-gradient row solve of solver='als': it must be 0 with solver=%r, "
                         "got %r" % (solver, als_nn_cg_steps))
    if n_gpus != 1:
        raise ValueError("als_nn_cg_steps=%r runs on one GPU: n_gpus must be 1, got %r" % (als_nn_cg_steps, n_gpus))
    if updated_non_negative is not None and not any(updated_non_negative):
        raise ValueError("als_nn_cg_steps=%r acts on non-negative factors only, and every factor this call updates is signed: "
                         "pass *_non_negative=True, or use als_cg_steps" % (als_nn_cg_steps,))
    if loss == "logistic" and not logit_pass:
        raise ValueError("als_nn_cg_steps=%r with loss='logistic' is not built (the conjugate-gradient rows have no reweighting pass): "
                         "als_nn_cg_steps must be 0; use als_nn_sweeps" % (als_nn_cg_steps,))
    if biases:
        raise ValueError("als_nn_cg_steps=%r with x_biases / y_biases is not built: als_nn_cg_steps must be 0; use als_nn_sweeps" % (als_nn_cg_steps,))


def check_als_dual_max(als_dual_max, solver="als", n_gpus=1, als_cg_steps=0):
    """``als_dual_max``: an integer 0 .. 128 (a bool is refused); non-zero with solver='als' on one GPU only, and not together with
    ``als_cg_steps`` (conjugate gradients already take every sweep the dual rows could).  ``loss='logistic'``, biases and background
    weights are all accepted: the option then acts on the eligible sweeps only.  No device is touched."""
    if isinstance(als_dual_max, (bool, np.bool_)) or not isinstance(als_dual_max, (numbers.Integral, np.integer)):
        raise ValueError("als_dual_max must be an integer 0 .. 128, got %r" % (als_dual_max,))
    if als_dual_max < 0 or als_dual_max > 128:
        raise ValueError("als_dual_max must be an integer 0 .. 128, got %r" % (als_dual_max,))
    if not als_dual_max:
        return
    if solver != "als":
        raise ValueError("als_dual_max is the dual row solve of solver='als': it must be 0 with solver=%r, got %r" % (solver, als_dual_max))
    if n_gpus != 1:
        raise ValueError("als_dual_max=%r runs on one GPU: n_gpus must be 1, got %r" % (als_dual_max, n_gpus))
    if als_cg_steps:
        raise ValueError("als_dual_max=%r together with als_cg_steps=%r: conjugate gradients already take every sweep the dual rows "
                         "could (signed factors with entry weights): one of the two must be 0" % (als_dual_max, als_cg_steps))


def check_als_logit_pass(als_logit_pass, solver="als", n_gpus=1, loss="logistic"):
    """``als_logit_pass``: a bool; True with solver='als', loss='logistic' and one GPU only.  No device is touched.  Returns the bool."""
    if not isinstance(als_logit_pass, (bool, np.bool_)):
        raise ValueError("als_logit_pass must be True or False, got %r" % (als_logit_pass,))
    if not als_logit_pass:
        return False
    if solver != "als":
        raise ValueError("als_logit_pass is the reweighting pass of solver='als' under loss='logistic': it must be False with solver=%r" % (solver,))
    if loss != "logistic":
        raise ValueError("als_logit_pass=True reweights the logistic relations in front of every sweep: it needs loss='logistic', got "
                         "loss=%r" % (loss,))
    if n_gpus != 1:
        raise ValueError("als_logit_pass=True runs on one GPU: n_gpus must be 1, got %r (the sharded form is not built)" % (n_gpus,))
    return True


def check_als_l2_scale(als_l2_scale, solver="als", n_gpus=1):
    """``als_l2_scale``: a real number nu in [0, 1] (a bool is refused); non-zero with solver='als' on one GPU only.  It composes with
    every other ALS keyword.  No device is touched.  Returns nu as a float."""
    if isinstance(als_l2_scale, (bool, np.bool_)) or not isinstance(als_l2_scale, (numbers.Real, np.integer, np.floating)):
        raise ValueError("als_l2_scale must be a number in [0, 1], got %r" % (als_l2_scale,))
    nu = float(als_l2_scale)
    if not (0.0 <= nu <= 1.0):
        raise ValueError("als_l2_scale must be a number in [0, 1], got %r" % (als_l2_scale,))
    if not nu:
        return 0.0
    if solver != "als":
        raise ValueError("als_l2_scale is the frequency-scaled regulariser of solver='als': it must be 0 with solver=%r, got %r" % (solver, als_l2_scale))
    if n_gpus != 1:
        raise ValueError("als_l2_scale=%r runs on one GPU: n_gpus must be 1, got %r" % (als_l2_scale, n_gpus))
    return nu


def _relation_counts(shape, W):
    """(per row, per column) of one relation of ``shape``: the stored entries with a weight > 0 of an observed relation (``W``: a
    SciPy sparse matrix, a dense array, or resolved ``EntryWeights``), or None, None for a full one (``W`` None)."""
    if W is None:
        return None, None
    if isinstance(W, EntryWeights):
        if W.kind == "csr":
            indptr, indices, w = np.asarray(W.indptr, dtype=np.int64), np.asarray(W.indices, dtype=np.int64), np.asarray(W.w, dtype=np.float64)
        else:
            return _relation_counts(shape, np.asarray(W.W))
    elif hasattr(W, "tocsr"):
        A = _canonical_csr(W)
        if A.shape != tuple(shape):
            raise ValueError("weights of shape %s for a relation of shape %s" % (A.shape, tuple(shape)))
        indptr, indices, w = A.indptr.astype(np.int64), A.indices.astype(np.int64), np.asarray(A.data, dtype=np.float64)
    else:
        D = np.asarray(W, dtype=np.float64)
        if D.shape != tuple(shape):
            raise ValueError("weights of shape %s for a relation of shape %s" % (D.shape, tuple(shape)))
        return (D > 0).sum(axis=1).astype(np.float64), (D > 0).sum(axis=0).astype(np.float64)
    if indptr.size != shape[0] + 1:
        raise ValueError("a pattern of %d rows for a relation of shape %s" % (indptr.size - 1, tuple(shape)))
    rows = np.repeat(np.arange(shape[0]), np.diff(indptr))
    keep = w > 0
    return (np.bincount(rows[keep], minlength=shape[0]).astype(np.float64),
            np.bincount(indices[keep], minlength=shape[1]).astype(np.float64))


def l2_multipliers(shape_x, shape_y, x_weights, y_weights, x_background_weight=0.0, y_background_weight=0.0, nu=1.0):
    """``(m_U, m_V, m_Z)``: the per-row multipliers of ``l2`` of the frequency-scaled regulariser (``Context.set_l2_rows``,
    ``CMF(als_l2_scale=nu)``), NumPy float64, on the host; None for a factor that reads no relation.

        m_F[i] = max(c_F[i], 1) ** nu,      c_F[i] summed over the relations the sweep of F reads (U: X; Z: Y; V: both):

    an OBSERVED relation (``*_weights``: SciPy sparse, a dense array, or resolved ``EntryWeights``) counts the stored entries with a
    weight > 0 of that row -- of that column on the transposed side --, n; under a background weight c0 it counts n + c0 D, D the
    cells of the row (Rendle, Krichene, Zhang, Koren: |I_u| + alpha0 |I|); a FULL relation (``*_weights`` None) counts D.
    ``shape_x`` / ``shape_y``: the shapes of X (m x d) and Y (d x p), None for a relation that is not there.  nu = 1 with observed
    relations is the weighted-lambda regulariser of ALS-WR (Zhou, Wilkinson, Schreiber, Pan); nu = 0 gives all ones.  The floor at 1
    keeps lambda_i >= l2: a row without an entry still solves lambda f = 0."""
    nu = float(nu)
    if not np.isfinite(nu):
        raise ValueError("nu must be finite, got %r" % (nu,))
    if shape_x is not None and shape_y is not None and shape_x[1] != shape_y[0]:
        raise ValueError("shape_x[1] must equal shape_y[0], got %s and %s" % (tuple(shape_x), tuple(shape_y)))
    c = [None, None, None]          # U, V, Z

    def add(f, v):
        c[f] = v if c[f] is None else c[f] + v

    for shape, W, c0, frow, fcol in ((shape_x, x_weights, x_background_weight, 0, 1), (shape_y, y_weights, y_background_weight, 1, 2)):
        if shape is None:
            continue
        r, k = int(shape[0]), int(shape[1])
        nr, nc = _relation_counts((r, k), W)
        if nr is None:                          # full: every cell of the row
            nr, nc = np.full(r, float(k)), np.full(k, float(r))
        elif c0:
            nr, nc = nr + float(c0) * k, nc + float(c0) * r
        add(frow, nr)
        add(fcol, nc)
    return tuple(None if v is None else np.maximum(v, 1.0) ** nu for v in c)


class HipALSSolver(HipMUSolver):
    """Alternating least squares in MU's sweep order V -> U -> Z (``cmf_als_step`` / ``cmf_als_nnls_step``) on

        1/2 sum_{Ox} wx (x - u.v)^2 + 1/2 sum_{Oy} wy (y - v.z)^2 + l2/2 (|U|^2 + |V|^2 + |Z|^2),     l2 > 0, no l1 term.

    Every row of a swept factor is fitted through its own k x k normal equations.  A relation with entry weights
    (``x_entry_weights`` / ``y_entry_weights``: a SciPy sparse W, ``'observed'``, or a dense W, which is converted to the CSR
    pattern of its non-zeros) counts over that pattern only; a relation without weights counts in every cell with weight 1, dense
    or sparse.  The weights are resolved as ``HipMUSolver`` resolves them.

    Signed factors (``U/V/Z_non_negative=False``): the row becomes the exact minimiser of its system, the objective descends
    monotonically.  Non-negative factors are handled as ``nn_sweeps`` says:

    ``nn_sweeps=n`` (1 .. 1024; 4 is the documented choice): each row of a non-negative factor runs n passes of cyclic coordinate
    descent on its own non-negative least-squares problem, from the row it has.  Every coordinate step is an exact minimisation, so
    the objective descends monotonically WITH non-negative factors; one pass is a weighted HALS sweep (each row under its own
    Gram), many passes approach alternating non-negative least squares.  Planted rank 3, 30 % observed, 10 iterations: RMSE on the
    unobserved cells 0.068 with n = 4 against 0.066 signed and 0.084 for the weighted MU after 300 iterations.

    ``nn_sweeps=0`` (default): WITH ``*_non_negative=True`` THE SOLVED ROW IS ONLY PROJECTED, max(0, .), the way the Newton solver
    honours the keyword -- NOT THE CONSTRAINED MINIMISER, NO MONOTONE DESCENT, and much weaker (the same problem: RMSE 0.152).

    ``cg_steps=n`` (1 .. 1024; 6 is the documented choice; default 0): a SIGNED factor with an OBSERVED relation (entry weights)
    never forms its k x k systems -- each row runs n matrix-free conjugate-gradient steps from the row it has
    (``cmf_als_cg_step``), O(nnz k) per step instead of O(nnz k^2) + k^3 / 3.  Every step lowers the row's quadratic, so the
    descent stays monotone; the rows are no longer exact minimisers (planted rank 12, 50 % observed, 20 iterations: objective
    50.05 with 6 steps against 50.46 exact, 51.45 with 4, 55.3 with 3, 60.8 with 2, 144.7 with 1).  A non-negative factor keeps the route ``nn_sweeps`` names,
    a factor whose relations are all unweighted the one shared inverse; refused when every updated factor is non-negative.

    ``nn_cg_steps=n`` (1 .. 1024; default 0): a NON-NEGATIVE factor with an OBSERVED relation never forms its k x k systems either
    -- each row runs n matrix-free projected conjugate-gradient steps from the row it has (``cmf_als_nncg_step``): a CG step on the
    free coordinates while it stays feasible, otherwise an exactly searched step towards the projection.  One or two passes of
    O(nnz k) per step; every step lowers the row's quadratic and keeps the row >= 0, so the descent stays monotone WITH
    non-negative factors.  Takes precedence over ``nn_sweeps`` on such a factor; signed factors keep ``cg_steps`` (0: exact rows),
    a non-negative factor whose relations are all unweighted keeps ``nn_sweeps``.  Not with ``loss='logistic'`` or biases.

    ``dual_max=n`` (1 .. 128; default 0): permission for the DUAL form of the exact rows (``cmf_als_dual_step``).  In a sweep
    whose rows are solved exactly (signed, or non-negative under ``nn_sweeps=0``: projected) and whose relations are all observed,
    without a background weight or a logistic loss, a row with 1 .. n stored entries is solved from the system of its entries,
    K = A A^T + l2 I (A: the gathered rows scaled by sqrt(w)), K z = y, f = A^T z -- the same exact minimiser from an n x n matrix
    instead of a k x k one, when the padded n (32, 64, 128) is below k_pad.  Other rows of such a sweep keep their bits, other
    sweeps their routes; biases are honoured.  Not together with ``cg_steps``.

    ``l2_scale=nu`` (a number in [0, 1]; default 0: off): the FREQUENCY-SCALED regulariser.  Row i of factor F is penalised by
    l2 m_F[i] / 2 |f_i|^2 with m_F[i] = max(c_F[i], 1)^nu, c_F[i] the stored entries with a positive weight the sweep of F reads in
    that row (plus c0 times the cells of the row under a background weight; every cell of a relation without weights) --
    ``l2_multipliers``.  nu = 1 is the weighted-lambda regulariser of ALS-WR, 0 < nu < 1 the form of Rendle et al. for implicit
    feedback.  The multipliers are computed on the host from the resolved patterns when a problem is bound, set for the factors this
    solver updates (``cmf_set_l2_rows``) and kept on ``l2_multipliers``; every route above honours them, row by row, and every
    descent statement above holds for the objective with the scaled regulariser.  The bias blocks keep ``bias_l2`` unscaled.  A
    factor whose relations are all unweighted has equal counts, hence one l2 for its shared matrix.

    ``x_background_weight=c0`` / ``y_background_weight`` (default 0): the implicit-feedback model (Hu, Koren, Volinsky).  The
    relation must have sparse entry weights W (or ``'observed'``) with every stored weight >= c0; the cells outside W's pattern
    then count with weight c0 and target 0,

        1/2 sum_O w (t - a.b)^2 + 1/2 c0 sum_{not O} (a.b)^2,

    at the cost of the pattern alone: the rows' systems take the excess weights w - c0 and c0 B^T B (``cmf_set_background_weight``).
    All three row solves honour it.  ``pycmf_amd.implicit_confidence(R, alpha)`` makes the targets and confidences from counts.  The
    error of such a relation is sqrt(sum_O w e^2 + c0 sum_{not O} (a.b)^2) (``cmf_als_residual_sq``).  On patterns with a few very
    long columns keep the exact route for V (``cg_steps=0``), as without a background.

    ``x_biases=True`` / ``y_biases=True`` (default False): the rating model  t ~ mu + r_i + c_j + a_i.b_j  on that relation, which
    must have sparse entry weights (or ``'observed'``) and no background weight.  mu is fixed at the weighted mean of the stored
    targets; r and c are fitted by exact block minimisation after the factor sweeps of every iteration, under the regulariser
    ``bias_l2`` (None: ``l2_reg``), and the factor sweeps -- whichever route ``nn_sweeps`` / ``cg_steps`` name -- read the targets
    minus the bias terms (``cmf_als_bias_step``); the descent stays monotone.  After a fit or a step ``x_bias`` / ``y_bias`` hold
    ``(offset, rows, cols)`` as float64; ``x_bias_init`` / ``y_bias_init`` start from such a triple (rows / cols may be None:
    zeros).  The bias blocks follow the update flag of the factor on their axis (r_x: U; c_x, r_y: V; c_y: Z), so a fold-in of new
    rows against a fixed V fits their own biases too.  The error of such a relation is the weighted residual of the biased model.

    ``x_huber_delta=d`` / ``y_huber_delta`` (None, or a finite number > 0): the relation -- sparse entry weights or ``'observed'``, a
    linear link, no background weight -- is fitted under the Huber loss  sum_O w rho_d(t - a.b),  rho_d(r) = r^2 / 2 for |r| <= d and
    d (|r| - d / 2) beyond, so that a grossly wrong entry pulls its row and its column with a bounded force.  In front of every
    sweep that reads the relation one pass writes the weights w min(1, d / |r|) at the residuals under the current rows
    (``cmf_set_huber_delta``), and the sweep -- whichever route the keywords above name, the bias blocks included -- reads them
    for w: each row then never raises the half-quadratic majoriser of its loss, and the descent statements above hold for the
    Huber objective.  ``l2_scale`` keeps counting the original weights.  The error metric takes sqrt(2 sum_O w rho_d) from such a
    relation -- the root of its squared residuals while none exceeds d -- and ``huber_loss`` holds ``(L_x, L_y)`` of the last
    evaluation (0 for a relation without a delta).

    ``loss='logistic'``: the relations whose link is 'logit' (at least one) are fitted as sigmoid(a.b) under the weighted
    cross-entropy over their observed entries,  sum_O w [softplus(a.b) - t a.b],  t in [0, 1]; a relation with a linear link keeps
    its Frobenius term (observed or full), so one V sweep may mix both.  A logistic relation needs a SciPy sparse W or ``'observed'``
    and takes no ``cg_steps``, background weight or biases (``check_logistic``).  Every row is the exact minimiser of the
    Jaakkola-Jordan quadratic bound of its loss at the row it has (``cmf_set_relation_loss``): the objective descends monotonically
    with signed factors, and with non-negative ones under ``nn_sweeps > 0``.  The error metric -- the stopping test and
    ``reconstruction_error`` -- then takes from a logistic relation its cross-entropy SUM (not a root) and from a Frobenius
    relation what it takes without this keyword; ``logistic_loss`` holds ``(L_x, L_y)`` of the last evaluation (0 for a Frobenius
    relation).  ``logit_pass=True`` moves the reweighting out of the normal-equation kernel into a pass of its own in front of every
    sweep that reads a logistic relation (``cmf_set_logit_pass``): ``cg_steps``, ``nn_cg_steps`` and ``dual_max`` are then accepted
    and honour the loss, with the same descent statements (conjugate gradients, projected or not, start at the current row and never
    raise the bound; the dual rows are exact).  ``l2_scale`` keeps counting the original weights.  The error metric is unchanged.

    Under ``loss='frobenius'`` it ignores alpha and the links, like MU.  The error metric is the one of a weighted MU fit,
    sqrt(sum wx e^2) + sqrt(sum wy e^2); the loop stays on the host (``cmf_run`` knows the MU and Newton steps only)."""

    _densify_unweighted = False

    def __init__(self, *args, x_entry_weights=None, y_entry_weights=None, nn_sweeps=0, cg_steps=0, x_background_weight=0.0,
                 y_background_weight=0.0, x_biases=False, y_biases=False, bias_l2=None, x_bias_init=None, y_bias_init=None,
                 loss="frobenius", nn_cg_steps=0, dual_max=0, l2_scale=0.0, x_huber_delta=None, y_huber_delta=None, logit_pass=False,
                 **kwargs):
        check_loss(loss, "als")
        self.logit_pass = check_als_logit_pass(logit_pass, "als", 1, loss)
        self.l2_scale = check_als_l2_scale(l2_scale)
        self.l2_multipliers = None           # (m_U, m_V, m_Z) of the bound problem under l2_scale > 0
        check_als(loss=loss)
        check_als_nn_sweeps(nn_sweeps)
        check_als_cg_steps(cg_steps)
        check_als_nn_cg_steps(nn_cg_steps, loss=loss, biases=bool(x_biases) or bool(y_biases), logit_pass=self.logit_pass)
        check_als_dual_max(dual_max, als_cg_steps=cg_steps)
        self.x_background_weight = check_background_weight(x_background_weight, "x", "als", x_entry_weights)
        self.y_background_weight = check_background_weight(y_background_weight, "y", "als", y_entry_weights)
        self.x_biases = check_biases(x_biases, "x", "als", x_entry_weights, self.x_background_weight)
        self.y_biases = check_biases(y_biases, "y", "als", y_entry_weights, self.y_background_weight)
        self.bias_l2 = check_bias_l2(bias_l2)
        for init, flag, nm in ((x_bias_init, self.x_biases, "x"), (y_bias_init, self.y_biases, "y")):
            if init is not None and not flag:
                raise ValueError("%s_bias_init needs %s_biases=True" % (nm, nm))
        self.x_bias_init, self.y_bias_init = x_bias_init, y_bias_init
        self.x_bias = self.y_bias = None     # (offset, rows, cols) as float64 after a fit or a step
        super().__init__(*args, loss="frobenius", x_entry_weights=x_entry_weights, y_entry_weights=y_entry_weights, **kwargs)
        check_als(self.l1_reg, self.l2_reg)
        # which relations are logistic (loss='logistic': those with a logit link); the device path of the weights is the Frobenius one
        self.als_loss = loss
        self._logit = (False, False)
        if loss == "logistic":
            self._logit = check_logistic(self.x_link, self.y_link, x_entry_weights, y_entry_weights, cg_steps, self.x_background_weight,
                                         self.y_background_weight, self.x_biases, self.y_biases, have_x=False, have_y=False,
                                         logit_pass=self.logit_pass)
        self.logistic_loss = None            # (L_x, L_y) of the last error evaluation under loss='logistic'
        # (the relations that take part in a call are checked again when it resolves its weights: a fold-in binds one of them)
        self.x_huber_delta = check_huber_delta(x_huber_delta, "x", "als", 1, x_entry_weights, self.x_link, self.x_background_weight, have=False)
        self.y_huber_delta = check_huber_delta(y_huber_delta, "y", "als", 1, y_entry_weights, self.y_link, self.y_background_weight, have=False)
        self.huber_loss = None               # (L_x, L_y) of the last error evaluation under a Huber delta
        self.nn_sweeps = int(nn_sweeps)
        self.cg_steps = int(cg_steps)
        self.nn_cg_steps = int(nn_cg_steps)
        self.dual_max = int(dual_max)

    def _weights_key(self):
        return (super()._weights_key() + (self.x_background_weight, self.y_background_weight, self.x_biases, self.y_biases) + tuple(self._logit)
                + (self.l2_scale, self.x_huber_delta, self.y_huber_delta, self.logit_pass))

    def _bias_l2(self):
        return self.bias_l2 if self.bias_l2 is not None else float(self.l2_reg)

    def _pull_biases(self):
        for which, flag, name in ((0, self.x_biases, "x_bias"), (1, self.y_biases, "y_bias")):
            if flag and self._ctx is not None:
                setattr(self, name, (self._ctx.get_biases(which)[0], self._ctx.get_bias(which, 0), self._ctx.get_bias(which, 1)))

    def _fit_end(self):
        self._pull_biases()

    def update_step(self, X, Y, U, V, Z, l1_reg, l2_reg, alpha):
        super().update_step(X, Y, U, V, Z, l1_reg, l2_reg, alpha)
        self._pull_biases()     # (the biases stay on the device between calls on the same X, Y; x_bias / y_bias follow them)

    def _resolve_weights(self, X, Y):
        key = (id(X), id(Y))
        if getattr(self, "_als_resolved_for", None) != key:
            raw = super()._resolve_weights(X, Y)
            if any(self._logit):   # a logistic relation that is part of the call: sparse weights, targets in [0, 1]
                check_logistic(self.x_link, self.y_link, self.x_entry_weights, self.y_entry_weights, self.cg_steps, self.x_background_weight,
                               self.y_background_weight, self.x_biases, self.y_biases, have_x=X is not None, have_y=Y is not None,
                               logit_pass=self.logit_pass)
                for on, ew, nm in ((self._logit[0], raw[0], "X"), (self._logit[1], raw[1], "Y")):
                    if on and ew is not None:
                        check_logistic_data(ew.t, nm)
            check_huber_delta(self.x_huber_delta, "x", "als", 1, self.x_entry_weights, self.x_link, self.x_background_weight, have=X is not None)
            check_huber_delta(self.y_huber_delta, "y", "als", 1, self.y_entry_weights, self.y_link, self.y_background_weight, have=Y is not None)
            self._als_resolved = tuple(_weights_as_pattern(ew) for ew in raw)
            check_background_floor(self._als_resolved[0], self.x_background_weight, "x")
            check_background_floor(self._als_resolved[1], self.y_background_weight, "y")
            shapes = ((None if X is None else X.shape), (None if Y is None else Y.shape))
            self._bias_start = []
            for ew, flag, init, shape, nm in ((self._als_resolved[0], self.x_biases, self.x_bias_init, shapes[0], "x"),
                                              (self._als_resolved[1], self.y_biases, self.y_bias_init, shapes[1], "y")):
                if not flag:
                    self._bias_start.append(None)
                    continue
                if ew is None or shape is None:
                    raise ValueError("%s_biases=True needs the relation and its %s_entry_weights" % (nm, nm))
                init = _check_bias_init(init, shape, nm)
                if init is None:   # mu: the weighted mean of the stored targets, in float64
                    w, t = np.asarray(ew.w, dtype=np.float64), np.asarray(ew.t, dtype=np.float64)
                    init = (float((w * t).sum() / w.sum()) if w.sum() > 0 else 0.0, None, None)
                self._bias_start.append(init)
            self._als_resolved_for = key
        return self._als_resolved

    def _bind_dims(self, X, Y, m, d, p, k):
        check_als(n_components=k)
        fresh = self._bound != (id(X), id(Y), m, d, p, k) + self._weights_key()
        ctx = super()._bind_dims(X, Y, m, d, p, k)
        if fresh:   # (binding the weights reset the background of the relation)
            for which, c0 in ((0, self.x_background_weight), (1, self.y_background_weight)):
                if c0:
                    ctx.set_background_weight(which, c0)
            for which, M in ((0, X), (1, Y)):
                if self._logit[which] and M is not None:
                    ctx.set_relation_loss(which, "logistic")
                    if self.logit_pass:   # every route of the step then honours the loss (cmf_set_logit_pass)
                        ctx.set_logit_pass(which, True)
            for which, M, delta in ((0, X, self.x_huber_delta), (1, Y, self.y_huber_delta)):
                if delta and M is not None:
                    ctx.set_huber_delta(which, delta)
            for which, start in enumerate(self._bias_start):
                if start is not None:
                    ctx.set_biases(which, True, start[0], self._bias_l2())
                    for axis in (0, 1):
                        if start[1 + axis] is not None:
                            ctx.set_bias(which, axis, start[1 + axis])
            self.l2_multipliers = None
            if self.l2_scale:   # (set_problem cleared them) the counts of the patterns this call was given: a fold-in counts its own rows
                wx, wy = self._als_resolved
                self.l2_multipliers = l2_multipliers(None if X is None else (m, d), None if Y is None else (d, p), wx, wy,
                                                     self.x_background_weight, self.y_background_weight, self.l2_scale)
                for which, upd in ((_lib.CMF_U, self.update_U), (_lib.CMF_V, self.update_V), (_lib.CMF_Z, self.update_Z)):
                    if upd and self.l2_multipliers[which] is not None:
                        ctx.set_l2_rows(which, self.l2_multipliers[which])
        return ctx

    def _device_step(self, l1_reg, l2_reg, alpha):
        check_als(l1_reg, l2_reg)
        if self.dual_max:      # (never with cg_steps: check_als_dual_max; the bias blocks follow inside the call)
            self._ctx.als_dual_step(l2_reg, self._nn_mask(), self._update_mask(), self.dual_max, self.nn_sweeps, self.nn_cg_steps)
        elif self.nn_cg_steps:   # (never with biases, or a logistic relation without logit_pass: check_als_nn_cg_steps)
            self._ctx.als_nncg_step(l2_reg, self._nn_mask(), self._update_mask(), self.cg_steps, self.nn_cg_steps, self.nn_sweeps)
        elif self.x_biases or self.y_biases:
            self._ctx.als_bias_step(l2_reg, self._nn_mask(), self._update_mask(), self.cg_steps, self.nn_sweeps)
        elif self.cg_steps:
            self._ctx.als_cg_step(l2_reg, self._nn_mask(), self._update_mask(), self.cg_steps, self.nn_sweeps)
        elif self.nn_sweeps:
            self._ctx.als_nnls_step(l2_reg, self._nn_mask(), self._update_mask(), self.nn_sweeps)
        else:
            self._ctx.als_step(l2_reg, self._nn_mask(), self._update_mask())

    def _device_error(self):
        X, Y = self._XY
        wx, wy = self.x_entry_weights is not None, self.y_entry_weights is not None
        ex2 = ey2 = 0.0
        hx, hy = bool(self.x_huber_delta) and X is not None, bool(self.y_huber_delta) and Y is not None
        if hx or hy:   # (a Huber relation has entry weights, no background, a linear link) its squared residual is never read
            qx, qy = wx and X is not None and not (hx or self._logit[0]), wy and Y is not None and not (hy or self._logit[1])
            if qx or qy:
                ex2, ey2 = self._ctx.als_residual_sq(qx, qy) if self._needs_als_residual() else self._ctx.weighted_residual_sq(qx, qy)
        elif self._needs_als_residual():
            # (biases: the residual of the biased model, t - mu - r - c - a.b, from the same call)
            # E = sum_O w (t - s)^2 + c0 (<A^T A, B^T B> - sum_O s^2): the error over every cell; a side without a background
            # gets the bits of the weighted residual from the same call
            ex2, ey2 = self._ctx.als_residual_sq(wx and X is not None, wy and Y is not None)
        elif any(self._logit):   # (no background, no biases: refused) the squared residual of a logistic relation is never read
            qx, qy = wx and X is not None and not self._logit[0], wy and Y is not None and not self._logit[1]
            if qx or qy:
                ex2, ey2 = self._ctx.weighted_residual_sq(qx, qy)
        elif wx or wy:
            ex2, ey2 = self._ctx.weighted_residual_sq(wx and X is not None, wy and Y is not None)
        if not (wx and wy):   # a relation without weights: every cell with weight 1 -- the plain residual, whatever its layout
            fx2, fy2 = self._ctx.residual_sq("linear", "linear")
            ex2, ey2 = (ex2 if wx else fx2), (ey2 if wy else fy2)
        ex, ey = (np.sqrt(max(ex2, 0.0)) if X is not None else 0.0), (np.sqrt(max(ey2, 0.0)) if Y is not None else 0.0)
        if any(self._logit):   # a logistic relation contributes its cross-entropy sum in place of the root of its squared residuals
            lx, ly = self._ctx.als_logistic_loss(self._logit[0] and X is not None, self._logit[1] and Y is not None)
            self.logistic_loss = (lx, ly)
            ex, ey = (lx if self._logit[0] and X is not None else ex), (ly if self._logit[1] and Y is not None else ey)
        if hx or hy:   # a Huber relation contributes sqrt(2 sum w rho): the root of its squared residuals while none exceeds delta
            lx, ly = self._ctx.als_huber_loss(hx, hy)
            self.huber_loss = (lx, ly)
            ex, ey = (np.sqrt(2.0 * lx) if hx else ex), (np.sqrt(2.0 * ly) if hy else ey)
        return ex, ey

    def _needs_als_residual(self):
        return bool(self.x_background_weight or self.y_background_weight or self.x_biases or self.y_biases)

    def _device_step_error(self, l1_reg, l2_reg, alpha):
        return None

    def _run_params(self):
        return None


def _weights_as_pattern(ew):
    """Dense entry weights as the CSR pattern of their non-zeros (a zero weight and an absent entry are the same term)."""
    if ew is None or ew.kind == "csr":
        return ew
    import scipy.sparse as sp
    P = sp.csr_matrix(np.asarray(ew.W, dtype=np.float64))
    P.eliminate_zeros()
    P.sort_indices()
    rows = np.repeat(np.arange(P.shape[0]), np.diff(P.indptr))
    t = np.asarray(ew.data, dtype=np.float64)[rows, P.indices]
    return EntryWeights("csr", indptr=P.indptr.astype(np.int64), indices=P.indices.astype(np.int32), t=t, w=np.asarray(P.data, dtype=np.float64))


class HipNewtonSolver(_HipIterativeSolver):
    """Row-wise Newton-Raphson sweeps U -> Z -> V (pycmf/cmf_solvers.py:318-522) on the GPU.

    With ``sg_sample_ratio < 1`` the per-row samples are drawn on the host from
    NumPy's global RNG in the reference's order (:328-344: U rows, Z rows, then for
    every V row a U-sample followed by a Z-sample) and handed to the device as
    index lists ("parity mode", ``sg_sampler='numpy'``, the default).  With
    ``sg_sampler='device'`` the same distribution (exactly int(n*ratio) distinct
    candidates per row) is drawn on the GPU from a counter-based generator: no
    host RNG time, no index upload, but not NumPy's stream.
    """

    #: ||H||_F / hessian_pertubation above which the float32 spectral clamp of a row's Hessian leaves the stated tolerance
    #: (tests/tools/fuzz_campaign.py: every case within 3e-3 of the float64 reference below it)
    CLAMP_RATIO_WARN = 1.0e4

    #: index entries per iteration above which drawing the per-row samples from NumPy's stream on the host dominates the iteration
    #: (one np.random.permutation per row plus the upload of the lists: ~16 s per iteration at BASELINE config C3, against 0.24 s
    #: for the whole iteration with sg_sampler='device')
    HOST_SAMPLER_WARN_ENTRIES = 1.0e7

    def _fit_begin(self):
        self._ctx.newton_clamp_stats(reset=True)
        if self.sg_sample_ratio < 1. and self.sg_sampler == "numpy":
            m, d, p, _ = self._ctx.shape
            r = self.sg_sample_ratio
            entries = ((m + p) * int(d * r) if (self.update_U or self.update_Z) else 0) + (d * (int(m * r) + int(p * r)) if self.update_V else 0)
            if entries > self.HOST_SAMPLER_WARN_ENTRIES:
                import warnings
                warnings.warn("pycmf_amd: sg_sampler='numpy' draws every row's sample from NumPy's global stream on the host, like the "
                              "reference (pycmf/cmf_solvers.py:328-344): %.1e list entries per iteration here -- the host RNG and the "
                              "upload of the lists will dominate the iteration.  sg_sampler='device' draws the same distribution on "
                              "the GPU (the benchmarked path; not NumPy's stream)." % entries, RuntimeWarning, stacklevel=3)

    def _fit_end(self):
        self.clamped_rows_, self.clamp_ratio_, self.refined_rows_ = self._ctx.newton_clamp_stats()
        if self.clamp_ratio_ > self.CLAMP_RATIO_WARN:
            import warnings
            warnings.warn("pycmf_amd: %d row Hessians had eigenvalues below hessian_pertubation=%g while ||H||_F / pertubation reached "
                          "%.1e and were NOT redone in float64 (more than refine_rows_max rows in one sweep, n_components > 256, or "
                          "refinement switched off): float32 Hessians resolve the clamped directions only to about 1e-7 * that ratio, "
                          "so the factors may differ from the float64 reference by more than the stated tolerance.  A positive l2_reg "
                          "at least as large as the perturbation, or fewer components than samples per row, keeps the Hessians well "
                          "conditioned." % (self.clamped_rows_, self.hessian_pertubation, self.clamp_ratio_),
                          RuntimeWarning, stacklevel=3)

    def _run_params(self):
        if self.sg_sample_ratio < 1. and self.sg_sampler != "device":
            return None                 # NumPy's stream: the lists are drawn on the host, iteration by iteration
        return dict(solver="newton", l1=self.l1_reg, l2=self.l2_reg, alpha=self.alpha, alpha_err=self.alpha, x_link=self.x_link,
                    y_link=self.y_link, nn_mask=self._nn_mask(), update_mask=self._update_mask(), pert=self.hessian_pertubation,
                    ratio=min(float(self.sg_sample_ratio), 1.0), seed=self._sample_seed)

    def _after_run(self, n_iter):
        if self.sg_sample_ratio < 1.:
            self._sample_seed += n_iter     # the C loop drew iteration i under seed + i, like _device_step would have

    def _draw(self, rows, n, ratio):
        size = int(n * ratio)
        out = np.empty((rows, size), dtype=np.int32)
        ar = np.arange(n)
        for i in range(rows):
            out[i] = np.random.permutation(ar)[:size]
        return out

    def _device_step(self, l1_reg, l2_reg, alpha):
        m, d, p, _ = self._ctx.shape
        ratio = self.sg_sample_ratio
        u_idx = z_idx = vx_idx = vy_idx = None
        if ratio < 1. and self.sg_sampler == "device":
            self._sample_seed += 1
            self._ctx.newton_step_device_sampled(alpha, l1_reg, l2_reg, self.x_link, self.y_link, self._nn_mask(),
                                                 self._update_mask(), self.hessian_pertubation, ratio,
                                                 self._sample_seed)
            return
        if ratio < 1.:
            if self.update_U:
                u_idx = self._draw(m, d, ratio)
            if self.update_Z:
                z_idx = self._draw(p, d, ratio)
            if self.update_V:
                sm, sp_ = int(m * ratio), int(p * ratio)
                vx_idx = np.empty((d, sm), dtype=np.int32)
                vy_idx = np.empty((d, sp_), dtype=np.int32)
                am, ap = np.arange(m), np.arange(p)
                for i in range(d):
                    vx_idx[i] = np.random.permutation(am)[:sm]
                    vy_idx[i] = np.random.permutation(ap)[:sp_]
        self._ctx.newton_step(alpha, l1_reg, l2_reg, self.x_link, self.y_link,
                              self._nn_mask(), self._update_mask(),
                              self.hessian_pertubation, ratio, u_idx, z_idx, vx_idx, vy_idx)
