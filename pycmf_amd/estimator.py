"""scikit-learn style front end: ``CMF`` and ``collective_matrix_factorization``.

API-compatible counterpart of pycmf/cmf.py:215-776 (same keywords, defaults,
attributes, validation messages and init routing); the solve itself is delegated
to the HIP solver objects in :mod:`pycmf_amd.solver_shell`.
"""
import numbers
import warnings

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils import check_array

from .factor_init import initialize_mf, init_custom, DeviceOperand, DEVICE_SVD_MIN_CELLS
from .solver_shell import (HipMUSolver, HipNewtonSolver, HipHALSSolver, HipALSSolver, check_loss, check_kl_data, check_beta, check_beta_extras, check_beta_data, check_entry_weights, check_hals,
                           check_als, check_als_nn_sweeps, check_als_cg_steps, check_als_nn_cg_steps, check_als_dual_max, check_als_l2_scale, check_als_logit_pass, check_background_weight, check_huber_delta, check_biases, check_bias_l2, check_logistic)
from .topic_terms import print_topic_terms_from_matrix, print_topic_terms_with_importances

_BETA_NAMES = {'frobenius': 2, 'kullback-leibler': 1, 'itakura-saito': 0}


def _check_beta_loss(beta_loss):
    # sklearn's _beta_loss_to_float contract (used at pycmf/cmf_solvers.py:106); only
    # the Frobenius objective is implemented by either solver (:166)
    if isinstance(beta_loss, str):
        if beta_loss not in _BETA_NAMES:
            raise ValueError('Invalid beta_loss parameter: got %r instead of one of %r, or a float.'
                             % (beta_loss, list(_BETA_NAMES)))
    elif not isinstance(beta_loss, numbers.Number):
        raise ValueError('Invalid beta_loss parameter: got %r instead of one of %r, or a float.'
                         % (beta_loss, list(_BETA_NAMES)))


def collective_matrix_factorization(X, Y, U=None, V=None, Z=None,
                                    x_init=None, y_init=None, n_components=None,
                                    solver='mu', alpha=0.5, beta_loss='frobenius',
                                    tol=1e-4, max_iter=200, l1_reg=0., l2_reg=0.,
                                    random_state=None, verbose=0,
                                    U_non_negative=True, V_non_negative=True, Z_non_negative=True,
                                    update_U=True, update_V=True, update_Z=True,
                                    x_link="linear", y_link="linear",
                                    hessian_pertubation=0.2, sg_sample_ratio=1.,
                                    device=0, sg_sampler="numpy", n_gpus=1, _return_solver=False, loss="frobenius",
                                    x_entry_weights=None, y_entry_weights=None, als_nn_sweeps=0, als_cg_steps=0,
                                    x_background_weight=0.0, y_background_weight=0.0, x_biases=False, y_biases=False, bias_l2=None,
                                    _x_bias_init=None, _y_bias_init=None, als_nn_cg_steps=0, als_dual_max=0, als_l2_scale=0.0,
                                    x_huber_delta=None, y_huber_delta=None, als_logit_pass=False):
    """Factorise X ~ f(U V^T) and Y ~ f(V Z^T) with a shared V on an MI355X.

    Same contract as the reference function (pycmf/cmf.py:215-456): returns
    ``(U, V, Z, n_iter)``; with ``x_init='custom'`` / ``y_init='custom'`` the given
    U/V/Z are the starting point (and U, Z are updated in place).

    ``n_gpus > 1``: data-parallel fit on that many GPUs of the node: one worker process per GPU takes a
    row block of X / U and a column block of Y / Z, V is reassembled by RCCL once per iteration
    (pycmf_amd/multi_gpu.py).  This process touches no GPU; the initial factors come from the host initialisers.  With
    ``sg_sample_ratio < 1`` the workers draw their samples with the device sampler.

    ``loss``: 'frobenius' (default) | 'kullback-leibler' -- the generalised Kullback-Leibler objective
    D(X || U V^T) + D(Y || V Z^T), the usual loss for count data (``sklearn.decomposition.NMF(beta_loss='kullback-leibler',
    solver='mu')`` per block); needs ``solver='mu'``, ``n_gpus=1`` and non-negative X and Y (``ValueError`` otherwise, before any
    device is touched).  ``beta_loss`` keeps the reference's meaning: parsed and ignored -- except under
    ``loss='beta-divergence'``, the one value with which ``beta_loss`` selects the objective: 'itakura-saito' (0; spectra and other
    scale-free positive data), 'kullback-leibler' (1), 'frobenius' (2) or a number in [0, 2] (0.5 and 1.5: the usual compromises
    between count noise and Gaussian noise) -- ``sklearn.decomposition.NMF(solver='mu', beta_loss=...)`` per block.  Needs
    ``solver='mu'``, ``n_gpus=1``, no entry weights, background weights or biases, non-negative X and Y, and at beta = 0 strictly
    positive ones (a SciPy-sparse relation has implicit zeros) -- ``ValueError`` otherwise, before any device is touched.  A
    sparse relation is uploaded dense for 0 < beta < 2, beta != 1; beta = 1 and beta = 2 run the Kullback-Leibler and Frobenius
    paths and give their results bit for bit.

    ``x_entry_weights`` / ``y_entry_weights``: fixed non-negative weights per entry of X / Y; the fit then minimises
    1/2 |sqrt(Wx) .* (X - U V^T)|^2 + 1/2 |sqrt(Wy) .* (Y - V Z^T)|^2 -- with a 0/1 mask, the observed entries only, instead of
    training on the missing ones as zeros.  None | a dense array of the relation's shape (a sparse relation is then densified on
    the host) | a SciPy sparse matrix (its stored pattern is the observed set, its values the weights; cost proportional to the
    stored entries) | ``'observed'`` (the relation must be SciPy sparse: its stored entries, explicit zeros included, carry
    weight 1).  A relation without weights takes part with weight 1 everywhere.  Needs ``solver='mu'``, ``loss='frobenius'``
    and ``n_gpus=1`` (``ValueError`` otherwise, as for negative, NaN or infinite weights or a shape mismatch, before any device is
    touched); ``n_components`` above 256 is a ``NotImplementedError``.

    ``solver='als'``: alternating least squares on that weighted objective plus l2/2 (|U|^2 + |V|^2 + |Z|^2) -- every factor row the
    exact minimiser of its own normal equations over the observed entries (``HipALSSolver``).  Needs ``l2_reg > 0``,
    ``l1_reg == 0``, ``loss='frobenius'`` and ``n_gpus=1`` (``ValueError`` otherwise, before any device is touched).  Exact
    minimisation and monotone descent hold for signed factors (``U/V/Z_non_negative=False``); with ``*_non_negative=True`` and
    ``als_nn_sweeps=0`` (default) the solved rows are only projected, which is much weaker.

    ``loss='logistic'`` (``solver='als'``, ``n_gpus=1``): the relations whose link is ``'logit'`` -- at least one -- are fitted as
    sigmoid(a.b) under the weighted cross-entropy over their OBSERVED entries, sum_O w [softplus(a.b) - t a.b], targets in [0, 1]
    (soft labels allowed); a relation with a linear link keeps its Frobenius term.  Each logistic relation needs
    ``*_entry_weights`` that are a SciPy sparse W or ``'observed'`` (labelled subsets, class weights, thumbs up / down), and takes
    no ``als_cg_steps``, ``*_background_weight`` or ``*_biases`` (``ValueError``, before any device is touched).  Every row solves
    the Jaakkola-Jordan bound of its loss exactly: monotone descent without a step size, with signed factors and with non-negative
    ones under ``als_nn_sweeps > 0`` (``HipALSSolver``).  THE STOPPING TEST AND ``reconstruction_err_`` then take from a logistic
    relation its cross-entropy SUM and from a Frobenius relation what it contributes under ``loss='frobenius'``.

    ``als_nn_sweeps``: 0 | n in 1 .. 1024 (``solver='als'`` only; ``ValueError`` otherwise, before any device is touched).  n >= 1:
    the rows of a non-negative factor run n passes of cyclic coordinate descent on their own non-negative least-squares problems
    instead of solve-and-project -- monotone descent with non-negative factors; 4 is the documented choice (``HipALSSolver``).

    ``als_cg_steps``: 0 | n in 1 .. 1024 (``solver='als'`` only; ``ValueError`` otherwise, and when every factor the call updates
    is non-negative, before any device is touched).  n >= 1: the rows of a SIGNED factor (``*_non_negative=False``) with entry
    weights on one of its relations run n matrix-free conjugate-gradient steps from the rows they have instead of forming and
    factorising their k x k systems -- still a monotone descent, far cheaper per iteration; 6 is the documented choice
    (``HipALSSolver``).  Non-negative factors keep the route ``als_nn_sweeps`` names, unweighted sweeps the shared inverse.

    ``als_nn_cg_steps``: 0 | n in 1 .. 1024 (``solver='als'`` and ``n_gpus=1`` only; ``ValueError`` otherwise, when every factor
    the call updates is signed, and together with ``loss='logistic'`` or biases, before any device is touched).  n >= 1: the rows of
    a NON-NEGATIVE factor with entry weights on one of its relations run n matrix-free projected conjugate-gradient steps from the
    rows they have instead of forming their k x k systems -- a monotone descent with non-negative factors at O(nnz k) per pass
    (``HipALSSolver``).  Signed factors keep ``als_cg_steps``, unweighted sweeps ``als_nn_sweeps``; a background weight is honoured.

    ``als_dual_max``: 0 | n in 1 .. 128 (``solver='als'`` and ``n_gpus=1`` only, not together with ``als_cg_steps``; ``ValueError``
    otherwise, before any device is touched).  n >= 1: in a sweep whose rows are solved exactly and whose relations all have entry
    weights and no background weight or logistic loss, a row with at most n stored entries is solved from its n x n DUAL system
    (K = A A^T + l2 I, f = A^T K^-1 y) instead of its k x k one -- the same exact minimiser, far cheaper when most rows have fewer
    entries than components (``HipALSSolver``).  Every other sweep keeps its route; biases are honoured.

    ``als_l2_scale``: 0 | nu in (0, 1] (``solver='als'`` and ``n_gpus=1`` only; ``ValueError`` otherwise, and for a bool or a value
    outside [0, 1], before any device is touched).  nu > 0: the frequency-scaled regulariser -- row i of a factor is penalised by
    l2_reg max(c_i, 1)^nu / 2 |f_i|^2, c_i the stored entries with a positive weight its sweep reads (plus the background weight
    times the cells of the row; every cell of a relation without weights): ``pycmf_amd.l2_multipliers``.  nu = 1 is ALS-WR's
    weighted-lambda regulariser.  Composes with every other ALS keyword; the bias blocks keep ``bias_l2`` unscaled
    (``HipALSSolver``).

    ``x_background_weight`` / ``y_background_weight``: 0 | c0 > 0 (``solver='als'`` only) -- implicit feedback.  The relation's
    entry weights must be a SciPy sparse W or ``'observed'`` with every stored weight >= c0; the cells outside that pattern then
    count with weight c0 and target 0 instead of not at all: 1/2 sum_O w (t - a.b)^2 + 1/2 c0 sum_{not O} (a.b)^2, at the cost of
    the stored entries alone (``HipALSSolver``; ``pycmf_amd.implicit_confidence`` makes targets and confidences from counts).
    ``ValueError`` before any device is touched: a non-zero value with another solver, without entry weights for that relation or
    with dense ones; a bool, a non-finite or a negative value; a stored weight below the background.

    ``x_biases`` / ``y_biases``: False | True (``solver='als'`` only) -- explicit ratings: the relation is fitted as
    mu + r_i + c_j + a_i.b_j, mu the weighted mean of its stored targets, r and c fitted under the regulariser ``bias_l2`` (None:
    ``l2_reg``) by exact block minimisation in every iteration (``HipALSSolver``).  The relation's entry weights must be a SciPy
    sparse W or ``'observed'``, and it must have no background weight.  ``ValueError`` before any device is touched: True with
    another solver, without such entry weights or with a background weight; a ``bias_l2`` that is not None or a finite number >= 0.
    The fitted biases are on the solver object (``x_bias`` / ``y_bias``) and on the estimator (``CMF.x_bias_`` / ``y_bias_``).

    ``x_huber_delta`` / ``y_huber_delta``: None | d > 0 (``solver='als'`` only) -- a robust fit of that relation: its term becomes
    the Huber loss sum_O w rho_d(t - a.b), quadratic up to |r| = d and linear beyond, so that a few grossly wrong entries (bot
    accounts, mis-keyed ratings, huge play counts) no longer bend their rows and columns.  Every sweep that reads the relation is
    preceded by one reweighting pass and then runs the route the other ALS keywords name (``HipALSSolver``).  ``ValueError`` before
    any device is touched: a bool, a non-finite or non-positive value; another solver; ``n_gpus > 1``; entry weights of that
    relation that are not a SciPy sparse W or ``'observed'``; a logit link or a background weight on it.

    ``als_logit_pass``: False | True (``solver='als'``, ``loss='logistic'`` and ``n_gpus=1`` only; ``ValueError`` otherwise) -- the
    logistic relations are reweighted by a pass of their own in front of every sweep instead of inside the normal-equation kernel,
    so that ``als_cg_steps``, ``als_nn_cg_steps`` and ``als_dual_max`` honour the logistic loss too (``HipALSSolver``): the
    matrix-free routes for logistic factorisation at large k.  Without it those keywords are refused under ``loss='logistic'`` (or,
    ``als_dual_max``, leave the logistic sweeps to the exact rows) as before.
    """
    if n_components is None:
        n_components = max(X.shape[1], Y.shape[1])
    _check_beta_loss(beta_loss)
    check_loss(loss, solver, n_gpus)
    als_logit_pass = check_als_logit_pass(als_logit_pass, solver, n_gpus, loss)
    if loss == "beta-divergence":
        beta = check_beta(beta_loss)
        check_beta_extras(x_entry_weights, y_entry_weights, x_background_weight, y_background_weight, x_biases, y_biases)
    check_entry_weights(x_entry_weights, y_entry_weights, solver, loss, n_gpus)
    check_als_nn_sweeps(als_nn_sweeps, solver)
    check_als_cg_steps(als_cg_steps, solver, [nn for nn, upd in ((U_non_negative, update_U), (V_non_negative, update_V),
                                                                 (Z_non_negative, update_Z)) if upd])
    check_als_nn_cg_steps(als_nn_cg_steps, solver, [nn for nn, upd in ((U_non_negative, update_U), (V_non_negative, update_V),
                                                                       (Z_non_negative, update_Z)) if upd],
                          n_gpus, loss, bool(x_biases) or bool(y_biases), als_logit_pass)
    check_als_dual_max(als_dual_max, solver, n_gpus, als_cg_steps)
    als_l2_scale = check_als_l2_scale(als_l2_scale, solver, n_gpus)
    x_background_weight = check_background_weight(x_background_weight, "x", solver, x_entry_weights)
    y_background_weight = check_background_weight(y_background_weight, "y", solver, y_entry_weights)
    x_biases = check_biases(x_biases, "x", solver, x_entry_weights, x_background_weight)
    y_biases = check_biases(y_biases, "y", solver, y_entry_weights, y_background_weight)
    bias_l2 = check_bias_l2(bias_l2)
    x_huber_delta = check_huber_delta(x_huber_delta, "x", solver, n_gpus, x_entry_weights, x_link, x_background_weight,
                                      have=X is not None and (update_U or update_V))
    y_huber_delta = check_huber_delta(y_huber_delta, "y", solver, n_gpus, y_entry_weights, y_link, y_background_weight,
                                      have=Y is not None and (update_Z or update_V))
    if bias_l2 is not None and solver != "als":
        raise ValueError("bias_l2 is the bias regulariser of solver='als': it must be None with solver=%r" % (solver,))

    if update_U or update_V:
        X = check_array(X, accept_sparse=('csr', 'csc'), dtype=float)
    if update_Z or update_V:
        Y = check_array(Y, accept_sparse=('csr', 'csc'), dtype=float)

    if update_V and X.shape[1] != Y.shape[0]:
        raise ValueError("Expected X.shape[1] == Y.shape[0], " +
                         "found X.shape = {}, Y.shape = {}".format(X.shape[1], Y.shape[0]))
    if loss == "kullback-leibler":
        check_kl_data(X, Y)
    if loss == "beta-divergence":
        check_beta_data(X, Y, beta, update_U or update_V, update_Z or update_V)
    if x_link not in ("linear", "logit"):
        raise ValueError("No such link %s for x_link" % x_link)
    if y_link not in ("linear", "logit"):
        raise ValueError("No such link %s for y_link" % y_link)
    if loss == "logistic":
        check_logistic(x_link, y_link, x_entry_weights, y_entry_weights, als_cg_steps, x_background_weight, y_background_weight, x_biases,
                       y_biases, have_x=X is not None and (update_U or update_V), have_y=Y is not None and (update_Z or update_V),
                       logit_pass=als_logit_pass)

    # ---- solver dispatch (cmf.py:433-453)
    common = dict(max_iter=max_iter, tol=tol, verbose=verbose, update_U=update_U, update_V=update_V,
                  update_Z=update_Z, l1_reg=l1_reg, l2_reg=l2_reg, random_state=random_state, device=device)
    if solver == "mu":
        if x_link != "linear" or y_link != "linear":
            warnings.warn("mu solver does not accept link functions other than linear, "
                          "link arguments will be ignored")
        solver_object = HipMUSolver(beta_loss=beta_loss, loss=loss, x_entry_weights=x_entry_weights, y_entry_weights=y_entry_weights,
                                    **common)
        solver_object.check_weights(X, Y)
    elif solver == "newton":
        if alpha == "auto":
            alpha = Y.shape[1] / (X.shape[0] + Y.shape[1])
        solver_object = HipNewtonSolver(alpha=alpha, U_non_negative=U_non_negative,
                                        V_non_negative=V_non_negative, Z_non_negative=Z_non_negative,
                                        x_link=x_link, y_link=y_link,
                                        hessian_pertubation=hessian_pertubation,
                                        sg_sample_ratio=sg_sample_ratio, sg_sampler=sg_sampler, **common)
    elif solver == "hals":
        check_hals(U_non_negative, V_non_negative, Z_non_negative, n_gpus, n_components)
        if x_link != "linear" or y_link != "linear":
            warnings.warn("hals solver does not accept link functions other than linear, "
                          "link arguments will be ignored")
        solver_object = HipHALSSolver(**common)
    elif solver == "als":
        check_als(l1_reg, l2_reg, n_gpus, loss, n_components)
        if loss != "logistic" and (x_link != "linear" or y_link != "linear"):
            warnings.warn("als solver does not accept link functions other than linear, "
                          "link arguments will be ignored")
        solver_object = HipALSSolver(loss=loss, x_link=x_link, y_link=y_link,
                                     U_non_negative=U_non_negative, V_non_negative=V_non_negative, Z_non_negative=Z_non_negative,
                                     x_entry_weights=x_entry_weights, y_entry_weights=y_entry_weights, nn_sweeps=als_nn_sweeps, cg_steps=als_cg_steps,
                                     x_background_weight=x_background_weight, y_background_weight=y_background_weight,
                                     x_biases=x_biases, y_biases=y_biases, bias_l2=bias_l2, x_bias_init=_x_bias_init,
                                     y_bias_init=_y_bias_init, nn_cg_steps=als_nn_cg_steps, dual_max=als_dual_max, l2_scale=als_l2_scale,
                                     x_huber_delta=x_huber_delta, y_huber_delta=y_huber_delta, logit_pass=als_logit_pass, **common)
        solver_object.check_weights(X, Y)
    else:
        raise ValueError("No such solver: %s" % solver)

    if n_gpus > 1 and (X is None or Y is None):
        n_gpus = 1     # a transform of one side only (cmf.py:726-747 with X or Y None): nothing to shard against, one GPU does it

    # Large inputs go to the GPU before the initialisers run, so that the randomized SVD behind
    # 'svd' / 'nndsvd*' can use the device copy for its products (the solver later reuses the upload).
    op_x = op_y = None
    big = [M is not None and M.shape[0] * M.shape[1] >= DEVICE_SVD_MIN_CELLS for M in (X, Y)]
    needs_dev = [i != 'custom' for i in (x_init, y_init)]   # every non-custom rule reads the data: mean and / or SVD
    if n_gpus <= 1 and X is not None and Y is not None and any(b and n for b, n in zip(big, needs_dev)):
        ctx = solver_object.bind_data(X, Y, n_components)
        if ctx is not None:
            op_x = DeviceOperand(ctx, 0, X.shape)
            op_y = DeviceOperand(ctx, 1, Y.shape)

    # ---- initial factors (cmf.py:402-430)
    init_spec = dict(x_init=x_init, y_init=y_init, n_components=n_components, random_state=random_state, x_link=x_link,
                     y_link=y_link, U_non_negative=U_non_negative, V_non_negative=V_non_negative, Z_non_negative=Z_non_negative)
    # n_gpus > 1 and inputs large enough for the device-side initialisers: rank 0 of the workers computes them on ITS GPU
    # (this process touches none); custom starts are validated here as always
    defer_init = (n_gpus > 1 and X is not None and Y is not None and any(b and n for b, n in zip(big, needs_dev))
                  and isinstance(random_state, (int, np.integer, type(None))))
    if defer_init and (x_init == 'custom' or y_init == 'custom'):
        defer_init = False
    if defer_init:
        U, V, Z = (np.zeros((n, n_components)) for n in (X.shape[0], X.shape[1], Y.shape[1]))
    else:
        U, V, Z = initial_factors(X, Y, U, V, Z, op_x=op_x, op_y=op_y, **init_spec)

    U, V, Z = _writable_f64(U), _writable_f64(V), _writable_f64(Z)
    if n_gpus > 1:
        from .multi_gpu import fit_multi_gpu
        U, V, Z = (np.ascontiguousarray(F) for F in (U, V, Z))
        params = dict(l1_reg=l1_reg, l2_reg=l2_reg, max_iter=max_iter, tol=tol, verbose=verbose,
                      alpha=(0.5 if solver == "mu" else float(alpha)), x_link=x_link, y_link=y_link,
                      U_non_negative=bool(U_non_negative), V_non_negative=bool(V_non_negative),
                      Z_non_negative=bool(Z_non_negative), hessian_pertubation=hessian_pertubation,
                      sg_sample_ratio=sg_sample_ratio,
                      random_state=(int(random_state) if isinstance(random_state, (int, np.integer)) else None),
                      # transform / partial updates (cmf.py:726-747: one code path for fit and transform): the U and Z sweeps are
                      # local to a rank, a fixed V simply skips the sum over the ranks
                      update_mask=(1 if update_U else 0) | (2 if update_V else 0) | (4 if update_Z else 0))
        if defer_init:
            params["init"] = dict(init_spec, random_state=(None if random_state is None else int(random_state)))
        n_iter, result = fit_multi_gpu(X, Y, U, V, Z, solver, int(n_gpus), params)
        solver_object.release()
        if _return_solver:
            return U, V, Z, n_iter, result
        return U, V, Z, n_iter
    U, V, Z, n_iter = solver_object.fit_iterative_update(X, Y, U, V, Z)
    if _return_solver:
        return U, V, Z, n_iter, solver_object
    solver_object.release()
    return U, V, Z, n_iter


def initial_factors(X, Y, U, V, Z, x_init, y_init, n_components, random_state, x_link, y_link,
                    U_non_negative, V_non_negative, Z_non_negative, op_x=None, op_y=None):
    """Initial U, V, Z as the reference's driver forms them (pycmf/cmf.py:402-430): per-side rule ('custom' validates the
    given arrays, a logit link forces 'random'), then the V merge.  ``op_x`` / ``op_y``: device copies of X / Y for the
    initialisers' passes over the data."""
    if x_init == 'custom':
        if X is not None:
            U = init_custom(U, X, n_components, 0, non_negative=U_non_negative, random_state=random_state)
            V = init_custom(V, X, n_components, 1, non_negative=V_non_negative, random_state=random_state)
    else:
        x_init = "random" if x_link == "logit" else x_init
        U, V = initialize_mf(X, n_components, init=x_init, random_state=random_state,
                             non_negative=(U_non_negative or V_non_negative), operand=op_x)
    if y_init == 'custom':
        if Y is not None:
            V = init_custom(V, Y, n_components, 0, non_negative=V_non_negative, random_state=random_state)
            Z = init_custom(Z, Y, n_components, 1, non_negative=Z_non_negative, random_state=random_state)
        V_from_y = V
    else:
        y_init = "random" if y_link == "logit" else y_init
        V_from_y, Z = initialize_mf(Y, n_components, init=y_init, random_state=random_state,
                                    non_negative=(Z_non_negative or V_non_negative), operand=op_y)
    if U_non_negative == Z_non_negative:
        V = (V + V_from_y) / 2
    elif Z_non_negative and not U_non_negative:
        V = V_from_y
    return U, V, Z


class FittedBias:
    """The bias terms of one relation of a fitted model: ``offset`` (mu), ``rows`` and ``cols`` (float64 vectors)."""

    def __init__(self, offset, rows, cols):
        self.offset, self.rows, self.cols = float(offset), np.asarray(rows, dtype=np.float64), np.asarray(cols, dtype=np.float64)

    def as_tuple(self):
        return self.offset, self.rows, self.cols

    def __repr__(self):
        return "FittedBias(offset=%r, rows=<%d>, cols=<%d>)" % (self.offset, self.rows.size, self.cols.size)


def _fitted_bias(triple):
    return None if triple is None else FittedBias(*triple)


def _writable_f64(F):
    if isinstance(F, np.ndarray) and F.dtype == np.float64 and F.flags.writeable:
        return F
    return np.array(F, dtype=np.float64)


class CMF(BaseEstimator, TransformerMixin):
    """Collective Matrix Factorization on MI355X; drop-in for ``pycmf.CMF``
    (pycmf/cmf.py:459-776): same constructor keywords and defaults (:620-624), same
    ``fit`` / ``fit_transform`` / ``transform`` / ``print_topic_terms`` methods and the
    attributes ``reconstruction_err_``, ``n_components_``, ``x_weights``,
    ``components``, ``y_weights``, ``n_iter_`` (:697-704).

    Extra keywords: ``device`` (GPU ordinal, default 0), ``sg_sampler`` and ``n_gpus`` (default 1; N > 1 = ``fit`` and
    ``transform`` run data-parallel on N GPUs of the node, one worker process per GPU; MU: V reassembled by ONE sum over the
    ranks per iteration -- a single RCCL all-reduce, or reduce-scatter + all-gather around a row-blocked V update when a timed
    trial on the live ranks finds that faster; a fit with a ``random_state`` pins the single all-reduce, so that it is
    reproducible run to run).

    ``n_gpus > 1`` with ``sg_sample_ratio < 1``: the samples come from the DEVICE sampler whatever ``sg_sampler`` says -- NumPy's
    stream (pycmf/cmf_solvers.py:328-344) is global and sequential, one draw per row in sweep order, and cannot be cut across
    ranks that sweep their rows concurrently.  Such a fit reproduces the reference's sampling STATISTICS (exactly
    ``int(n * ratio)`` distinct uniform indices per row), not its iterates; ``n_gpus=1, sg_sampler='numpy'`` does.

    ``sg_sampler`` (only read when ``sg_sample_ratio < 1``): ``'numpy'`` (default) draws every row's sample from NumPy's global
    stream on the host, in the reference's order -- results reproduce the reference's for the same ``random_state``, but the
    host RNG costs one ``np.random.permutation`` per row per sweep: fine at the reference's own sizes, seconds per iteration
    beyond ~1e7 drawn indices (a ``RuntimeWarning`` says so; BASELINE config C3 would spend ~16 s per iteration there).
    ``'device'`` draws the same distribution (exactly ``int(n * ratio)`` distinct indices per row, uniform) on the GPU from a
    counter-based generator: the benchmarked path (C3: 0.24 s per iteration), statistically but not numerically NumPy's stream.

    ``loss``: ``'frobenius'`` (default) or ``'kullback-leibler'``: multiplicative updates on the generalised Kullback-Leibler
    objective D(X || U V^T) + D(Y || V Z^T), for count data (the reference documents ``beta_loss='kullback-leibler'`` and does not
    implement it; ``beta_loss`` stays parsed-and-ignored here too).  Needs ``solver='mu'``, ``n_gpus=1`` and non-negative X, Y.
    ``'beta-divergence'``: the one value under which ``beta_loss`` selects the objective -- ``'itakura-saito'`` (0),
    ``'kullback-leibler'`` (1), ``'frobenius'`` (2) or a number in [0, 2]; multiplicative updates on D_beta(X || U V^T) +
    D_beta(Y || V Z^T).  Needs ``solver='mu'``, ``n_gpus=1``, no entry weights, non-negative X, Y and, at beta = 0, strictly
    positive ones (dense).
    ``reconstruction_err_`` is then sqrt(2 D_x) + sqrt(2 D_y), the stopping test the reference's on
    alpha sqrt(2 D_x) + (1 - alpha) sqrt(2 D_y).

    ``als_nn_sweeps`` (``solver='als'`` only, default 0): n >= 1 fits the rows of a non-negative factor by n passes of cyclic
    coordinate descent on their non-negative least-squares problems instead of projecting the unconstrained solution
    (``collective_matrix_factorization``); ``CMF(solver="als", l2_reg=0.05, als_nn_sweeps=4)`` is the documented choice.

    ``als_cg_steps`` (``solver='als'`` only, default 0): n >= 1 fits the rows of a signed factor that has entry weights by n
    matrix-free conjugate-gradient steps instead of exact k x k solves (``collective_matrix_factorization``);
    ``CMF(solver="als", l2_reg=0.05, als_cg_steps=6, U_non_negative=False, V_non_negative=False, Z_non_negative=False)`` is the
    documented choice.

    ``als_nn_cg_steps`` (``solver='als'`` only, default 0): n >= 1 fits the rows of a non-negative factor that has entry weights by
    n matrix-free projected conjugate-gradient steps, never forming the k x k systems (``collective_matrix_factorization``);
    ``CMF(solver="als", l2_reg=0.05, als_nn_cg_steps=4)``.  ``transform`` honours it.  It is a keyword-only OPTION, not one of the
    estimator's scikit-learn parameters: ``get_params`` lists what it listed before (grid searches and pipelines that enumerate the
    parameters see no new name), ``set_params(als_nn_cg_steps=n)``, ``clone`` and ``repr`` carry it all the same.  Needs
    scikit-learn >= 1.3 (``__sklearn_clone__``); with an older one passing the keyword is a ``NotImplementedError``.

    ``als_dual_max`` (``solver='als'`` only, default 0): n in 1 .. 128 solves the rows with at most n stored entries from their
    n x n dual systems where the sweep allows it -- the same exact rows, cheaper when rows have fewer entries than components
    (``collective_matrix_factorization``); ``CMF(solver="als", l2_reg=0.05, als_dual_max=128, U_non_negative=False,
    V_non_negative=False, Z_non_negative=False)``.  ``transform`` honours it: the fold-in of new rows is a sweep over short
    observed rows.  A keyword-only OPTION like ``als_nn_cg_steps``.

    ``als_l2_scale`` (``solver='als'`` only, default 0.0): nu in (0, 1] scales the l2 penalty of every factor row by
    max(c_i, 1)^nu, c_i the entries its sweep reads in that row (``collective_matrix_factorization``, ``pycmf_amd.l2_multipliers``):
    ``CMF(solver="als", l2_reg=0.05, als_l2_scale=1.0)`` is ALS-WR's weighted-lambda regulariser.  After a fit ``l2_multipliers_``
    holds ``(m_U, m_V, m_Z)`` (None with the option off); ``transform`` counts the rows of the X / Y it is given, so a folded-in
    row gets the penalty of its own length.  A keyword-only OPTION like ``als_nn_cg_steps``.

    ``x_huber_delta`` / ``y_huber_delta`` (``solver='als'`` only, default None): d > 0 fits that relation under the Huber loss of
    threshold d over its observed entries instead of the squared one (``collective_matrix_factorization``):
    ``CMF(solver="als", l2_reg=0.5, x_huber_delta=1.0, ...).fit(X, Y, x_entry_weights='observed')`` for ratings with gross outliers.
    ``reconstruction_err_`` and the stopping test take sqrt(2 sum_O w rho_d) from such a relation, ``huber_loss_`` holds the sums
    ``(L_x, L_y)`` after a fit (None without a delta), and ``transform`` folds new rows in under the same loss.  ``predict``,
    ``score_entries``, ``top_n``, ``ranks`` and ``evaluate`` read the fitted factors as always.  Keyword-only OPTIONS like
    ``als_nn_cg_steps``.

    ``als_logit_pass`` (``solver='als'`` with ``loss='logistic'`` only, default False): True reweights the logistic relations by a
    pass in front of every sweep, so that ``als_cg_steps``, ``als_nn_cg_steps`` and ``als_dual_max`` fit them too
    (``collective_matrix_factorization``): ``CMF(solver="als", loss="logistic", x_link="logit", l2_reg=0.5, als_logit_pass=True,
    als_cg_steps=6, U_non_negative=False, V_non_negative=False, Z_non_negative=False)``.  ``transform`` honours it;
    ``logistic_loss_``, ``reconstruction_err_`` and the stopping test are unchanged.  A keyword-only OPTION like ``als_nn_cg_steps``.
    """

    # keyword-only options outside get_params(): name -> default
    _OPTIONS = {"als_nn_cg_steps": 0, "als_dual_max": 0, "als_l2_scale": 0.0, "x_huber_delta": None, "y_huber_delta": None,
                "als_logit_pass": False}

    def __init__(self, n_components=None, x_init=None, y_init=None, solver='mu', alpha='auto',
                 beta_loss='frobenius', tol=1e-4, max_iter=600,
                 random_state=None, l1_reg=0., l2_reg=0., verbose=0,
                 U_non_negative=True, V_non_negative=True, Z_non_negative=True,
                 x_link="linear", y_link="linear", hessian_pertubation=0.2, sg_sample_ratio=1.,
                 device=0, sg_sampler="numpy", n_gpus=1, loss="frobenius", als_nn_sweeps=0, als_cg_steps=0, **options):
        unknown = sorted(set(options) - set(self._OPTIONS))
        if unknown:
            raise TypeError("CMF.__init__() got an unexpected keyword argument %r" % (unknown[0],))
        self.n_components = n_components
        self.x_init = x_init
        self.y_init = y_init
        self.solver = solver
        self.alpha = alpha
        self.beta_loss = beta_loss
        self.tol = tol
        self.max_iter = max_iter
        self.random_state = random_state
        self.l1_reg = l1_reg
        self.l2_reg = l2_reg
        self.verbose = verbose
        self.U_non_negative = U_non_negative
        self.V_non_negative = V_non_negative
        self.Z_non_negative = Z_non_negative
        self.x_link = x_link
        self.y_link = y_link
        self.hessian_pertubation = hessian_pertubation
        self.sg_sample_ratio = sg_sample_ratio
        self.device = device
        self.sg_sampler = sg_sampler
        self.n_gpus = n_gpus
        self.loss = loss
        self.als_nn_sweeps = als_nn_sweeps
        self.als_cg_steps = als_cg_steps
        if options and not hasattr(BaseEstimator, "__sklearn_clone__"):   # (scikit-learn < 1.3: clone() would drop the option in silence)
            raise NotImplementedError("CMF(%s=...) needs scikit-learn >= 1.3" % (sorted(options)[0],))
        for name, default in self._OPTIONS.items():
            setattr(self, name, options.get(name, default))

    def __repr__(self, N_CHAR_MAX=700):
        text = super().__repr__(N_CHAR_MAX=N_CHAR_MAX)
        extra = ", ".join("%s=%r" % (name, getattr(self, name)) for name, default in self._OPTIONS.items() if getattr(self, name) != default)
        if not extra or not text.endswith(")"):
            return text
        return text[:-1] + ("" if text.endswith("()") else ", ") + extra + ")"

    def set_params(self, **params):
        for name in [n for n in params if n in self._OPTIONS]:
            setattr(self, name, params.pop(name))
        return super().set_params(**params)

    def __sklearn_clone__(self):
        from sklearn.base import clone
        params = {name: clone(value, safe=False) for name, value in self.get_params(deep=False).items()}
        return type(self)(**params, **{name: getattr(self, name) for name in self._OPTIONS})

    def _kwargs(self):
        return dict(solver=self.solver, beta_loss=self.beta_loss, tol=self.tol, max_iter=self.max_iter,
                    l1_reg=self.l1_reg, l2_reg=self.l2_reg, random_state=self.random_state,
                    verbose=self.verbose, U_non_negative=self.U_non_negative,
                    V_non_negative=self.V_non_negative, Z_non_negative=self.Z_non_negative,
                    x_link=self.x_link, y_link=self.y_link,
                    hessian_pertubation=self.hessian_pertubation,
                    sg_sample_ratio=self.sg_sample_ratio, device=self.device, sg_sampler=self.sg_sampler,
                    loss=self.loss, als_nn_sweeps=self.als_nn_sweeps, als_cg_steps=self.als_cg_steps,
                    als_nn_cg_steps=self.als_nn_cg_steps, als_dual_max=self.als_dual_max, als_l2_scale=self.als_l2_scale,
                    x_huber_delta=self.x_huber_delta, y_huber_delta=self.y_huber_delta, als_logit_pass=self.als_logit_pass)

    def fit_transform(self, X, Y, U=None, V=None, Z=None, x_entry_weights=None, y_entry_weights=None, x_background_weight=0.0,
                      y_background_weight=0.0, x_biases=False, y_biases=False, bias_l2=None):
        """``x_entry_weights`` / ``y_entry_weights``: per-entry weights of X / Y for this fit (``collective_matrix_factorization``);
        ``reconstruction_err_`` is then sqrt(sum Wx (X - U V^T)^2) + sqrt(sum Wy (Y - V Z^T)^2).
        ``x_background_weight`` / ``y_background_weight`` (``solver='als'``, sparse entry weights): the weight of the cells outside
        the weights' pattern, for implicit feedback; ``reconstruction_err_`` is then sqrt(E_x) + sqrt(E_y) with
        E = sum_O w (t - a.b)^2 + c0 sum_{not O} (a.b)^2.
        Under ``loss='logistic'`` a relation with a logit link contributes its weighted cross-entropy sum to ``reconstruction_err_``
        (a Frobenius relation what it contributes otherwise), and ``logistic_loss_`` holds ``(L_x, L_y)``.
        ``x_biases`` / ``y_biases`` / ``bias_l2`` (``solver='als'``, sparse entry weights, no background weight): fit the relation as
        mu + r_i + c_j + a_i.b_j (``collective_matrix_factorization``).  The model then carries ``x_bias_`` / ``y_bias_`` (None, or an
        object with ``.offset``, ``.rows``, ``.cols``), which ``predict``, ``score_entries``, ``top_n``, ``ranks`` and ``transform``
        honour."""
        X = check_array(X, accept_sparse=('csr', 'csc'), dtype=float)
        Y = check_array(Y, accept_sparse=('csr', 'csc'), dtype=float)
        if X.shape[1] != Y.shape[0]:
            raise ValueError("Expected X.shape[1] == Y.shape[0], " +
                             "found X.shape = {}, Y.shape = {}".format(X.shape, Y.shape))
        U, V, Z, n_iter_, solver_object = collective_matrix_factorization(
            X=X, Y=Y, U=U, V=V, Z=Z, n_components=self.n_components,
            x_init=self.x_init, y_init=self.y_init, alpha=self.alpha, n_gpus=self.n_gpus,
            _return_solver=True, x_entry_weights=x_entry_weights, y_entry_weights=y_entry_weights,
            x_background_weight=x_background_weight, y_background_weight=y_background_weight, x_biases=x_biases, y_biases=y_biases,
            bias_l2=bias_l2, **self._kwargs())
        # unweighted sum of the two residual norms, evaluated on the device where the
        # data and the final factors still live (cmf.py:697-698)
        self.reconstruction_err_ = solver_object.reconstruction_error()
        self.logistic_loss_ = getattr(solver_object, "logistic_loss", None)   # (L_x, L_y) under loss='logistic', else None
        self.huber_loss_ = getattr(solver_object, "huber_loss", None)         # (L_x, L_y) under a Huber delta, else None
        self.x_bias_ = _fitted_bias(getattr(solver_object, "x_bias", None))
        self.y_bias_ = _fitted_bias(getattr(solver_object, "y_bias", None))
        self.bias_l2_ = bias_l2
        self.l2_multipliers_ = getattr(solver_object, "l2_multipliers", None)   # (m_U, m_V, m_Z) under als_l2_scale > 0, else None
        solver_object.release()
        self.n_components_ = U.shape[1]
        self.x_weights = U
        self.components = V
        self.y_weights = Z
        self.n_iter_ = n_iter_
        return U, V, Z

    def fit(self, X, Y, **params):
        self.fit_transform(X, Y, **params)
        return self

    def transform(self, X, Y, x_entry_weights=None, y_entry_weights=None, x_background_weight=0.0, y_background_weight=0.0):
        """Re-fit U and/or Z with the learnt components V held fixed; pass ``None`` for
        the side that should be left alone (cmf.py:726-747).  ``x_entry_weights`` / ``y_entry_weights``: per-entry weights of
        the given X / Y, as in ``fit_transform``; ``x_background_weight`` / ``y_background_weight`` likewise: with them this is
        the fold-in of new users (rows of X) against the fixed V under the implicit-feedback model.

        On a model fitted with biases the given relation is folded in under the same model: the fitted offset and the biases on V's
        axis (the columns of X, the rows of Y) stay fixed, the biases of the new rows of X (columns of Y) start at 0 and are fitted
        with U (Z).  The return value is unchanged; those biases are left on ``transform_x_row_bias_`` /
        ``transform_y_col_bias_`` (None for a side without biases).  Such a relation needs its ``*_entry_weights`` here too."""
        assert hasattr(self, "components")
        update_U = X is not None
        update_Z = Y is not None
        alpha = 1 if Y is None else 0 if X is None else "auto"
        U = None if update_U else self.x_weights
        Z = None if update_Z else self.y_weights
        bx = getattr(self, "x_bias_", None) if update_U else None
        by = getattr(self, "y_bias_", None) if update_Z else None
        U, V, Z, _, solver_object = collective_matrix_factorization(
            X=X, Y=Y, U=U, V=self.components, Z=Z, n_components=self.n_components,
            x_init="custom", y_init="custom", alpha=alpha,
            update_U=update_U, update_V=False, update_Z=update_Z, x_entry_weights=x_entry_weights,
            y_entry_weights=y_entry_weights, x_background_weight=x_background_weight, y_background_weight=y_background_weight,
            x_biases=bx is not None, y_biases=by is not None, bias_l2=getattr(self, "bias_l2_", None),
            _x_bias_init=None if bx is None else (bx.offset, None, bx.cols),
            _y_bias_init=None if by is None else (by.offset, by.rows, None),
            _return_solver=True, **self._kwargs())
        self.transform_x_row_bias_ = None if bx is None else solver_object.x_bias[1]
        self.transform_y_col_bias_ = None if by is None else solver_object.y_bias[2]
        if hasattr(solver_object, "release"):
            solver_object.release()
        return U, V, Z

    def _relation(self, relation):
        if relation not in ("x", "y"):
            raise ValueError("relation must be 'x' or 'y', got %r" % (relation,))
        if relation == "x":
            return self.x_weights, self.components, self.x_link, getattr(self, "x_bias_", None)
        return self.components, self.y_weights, self.y_link, getattr(self, "y_bias_", None)

    def predict(self, rows, cols, relation="x"):
        """float32[n]: the fitted value of the cells ``(rows[q], cols[q])`` of ``relation`` -- 'x': f(U V^T), 'y': f(V Z^T), f the
        estimator's own link, plus offset, row and column bias on a model fitted with biases.  Works for a model of any solver;
        the product is never formed (float32 on GPU ``self.device``, ``pycmf_amd.predict_products``)."""
        assert hasattr(self, "components")
        from .prediction import predict_products
        A, B, link, bias = self._relation(relation)
        kw = {} if bias is None else dict(offset=bias.offset, row_bias=bias.rows, col_bias=bias.cols)
        return predict_products(A, B, rows, cols, link=link, device=self.device, **kw)

    def score_entries(self, held_out, relation="x"):
        """``{'rmse', 'mae', 'n'}`` of ``predict`` over the stored entries of the SciPy sparse ``held_out`` (the relation's shape;
        stored zeros count); the reduction runs in float64 on the host."""
        assert hasattr(self, "components")
        import scipy.sparse as sp
        A, B, _, _ = self._relation(relation)
        if not sp.issparse(held_out):
            raise ValueError("held_out must be a SciPy sparse matrix whose stored entries are the cells to score, got %s" % type(held_out).__name__)
        if held_out.shape != (A.shape[0], B.shape[0]):
            raise ValueError("held_out must have shape %r, got %r" % ((A.shape[0], B.shape[0]), held_out.shape))
        H = held_out.tocoo()
        if H.nnz == 0:
            return {"rmse": float("nan"), "mae": float("nan"), "n": 0}
        e = self.predict(H.row.astype(np.int64), H.col.astype(np.int64), relation=relation).astype(np.float64) - np.asarray(H.data, dtype=np.float64)
        return {"rmse": float(np.sqrt(np.mean(e * e))), "mae": float(np.mean(np.abs(e))), "n": int(H.nnz)}

    def top_n(self, relation="x", axis=0, rows=None, n=10, exclude=None, queries=None, query_bias=None):
        """The ``n`` highest entries per row (``axis=0``) or per column (``axis=1``) of the fitted reconstruction of
        ``relation`` -- 'x': f(U V^T), 'y': f(V Z^T), f the estimator's own ``x_link`` / ``y_link`` -- as
        ``(idx int32[nq, n], val float32[nq, n])``, best first, equal scores by smaller index.  The product is never formed: scores
        and selection run on GPU ``self.device`` (one GPU whatever ``n_gpus``; float32, pycmf_amd/csrc/cmf_topk.hip.h).

        ``rows``: index array of the rows (columns for ``axis=1``) to answer for, ``None`` = all.  ``exclude``: a SciPy sparse
        matrix of the relation's shape whose stored entries are skipped (pass the training ``X``: what a user has already seen);
        a row with fewer than n candidates left has ``-1 / -inf`` in the remaining places.  ``queries``: an (nq x k) array used
        instead of the fitted rows -- the ``U`` that ``transform`` returned for new rows; ``exclude`` then has nq rows (columns
        for ``axis=1``).  ``rows`` together with ``queries`` is a ``ValueError``.

        On a model fitted with biases on ``relation`` the scores include offset and biases (``val`` is the prediction itself, the
        order includes the candidate's bias; needs ``n_components + 2 <= 256``), and ``queries`` take an optional ``query_bias``
        (one value per query, default 0: what ``transform`` left on ``transform_x_row_bias_``)."""
        assert hasattr(self, "components")
        from .prediction import model_top_n
        bias = self._relation(relation)[3] if relation in ("x", "y") else None
        return model_top_n(self.x_weights, self.components, self.y_weights, self.x_link, self.y_link, self.device,
                           relation=relation, axis=axis, rows=rows, n=n, exclude=exclude, queries=queries,
                           bias=None if bias is None else bias.as_tuple(), query_bias=query_bias)

    def ranks(self, held_out, relation="x", axis=0, exclude=None, rows=None, queries=None, query_bias=None):
        """The exact rank of every entry ``held_out`` stores in the fitted reconstruction of ``relation``, per row (``axis=0``) or
        per column (``axis=1``): ``(indptr int64[nq + 1], indices int32, rank int32, eligible int32[nq])`` -- the canonical CSR
        order of ``held_out`` (of its transpose for ``axis=1``), ``rank[e]`` = how many candidates of the row that ``exclude``
        does not store the model scores higher than entry e (equal scores: the smaller index first; 0-based, so rank r < n <=>
        the entry is place r of ``top_n(n=n, exclude=exclude)``; -1 if the entry's own score is NaN), ``eligible[i]`` = candidates
        - entries ``exclude`` stores in row i.  The product is never formed (float32, pycmf_amd/csrc/cmf_rank.hip.h; one GPU).

        ``held_out`` / ``exclude``: SciPy sparse (stored entries) or dense (non-zeros) matrices of the relation's shape -- pass
        the test split and the training ``X``.  A held-out entry that ``exclude`` stores too is a ``ValueError``: a test entry
        among the training entries is a leak.  ``rows`` / ``queries`` as in ``top_n`` (both matrices then have nq rows for
        ``queries``); ``rows`` together with ``queries`` is a ``ValueError``."""
        assert hasattr(self, "components")
        from .prediction import model_ranks
        bias = self._relation(relation)[3] if relation in ("x", "y") else None
        return model_ranks(self.x_weights, self.components, self.y_weights, self.device, held_out, relation=relation, axis=axis,
                           exclude=exclude, rows=rows, queries=queries, bias=None if bias is None else bias.as_tuple(),
                           query_bias=query_bias)

    def evaluate(self, held_out, n=(10,), relation="x", axis=0, exclude=None, rows=None, queries=None, query_bias=None):
        """Ranking metrics of the fitted model on the entries ``held_out`` stores: ``ranks`` with the same keywords, then
        ``pycmf_amd.ranking_metrics`` at the cut-offs ``n`` -- a dict with ``hit_rate@n``, ``recall@n``, ``precision@n``,
        ``ndcg@n`` per cut-off, ``mrr``, ``map``, ``auc`` and the row counts."""
        assert hasattr(self, "components")
        from .evaluation import ranking_metrics, _check_cutoffs
        _check_cutoffs(n)
        indptr, _, rank, eligible = self.ranks(held_out, relation=relation, axis=axis, exclude=exclude, rows=rows, queries=queries,
                                               query_bias=query_bias)
        return ranking_metrics(indptr, rank, eligible, n=n)

    def print_topic_terms(self, vectorizer, topn_words=10, importances=True):
        """Print the top terms per topic (cmf.py:749-776); works with both the old
        ``get_feature_names`` and the current ``get_feature_names_out`` vectorizer API."""
        getter = getattr(vectorizer, "get_feature_names_out", None) or vectorizer.get_feature_names
        idx_to_word = np.array(getter())
        if importances:
            print_topic_terms_with_importances(self.x_weights, self.y_weights, idx_to_word,
                                               topn_words=topn_words)
        else:
            print_topic_terms_from_matrix(self.x_weights, idx_to_word, topn_words=topn_words)
