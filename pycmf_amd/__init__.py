"""pycmf_amd -- MI355X-native collective matrix factorisation (drop-in for pycmf).

The public names are resolved on first use (PEP 562): ``from pycmf_amd import _lib`` -- what bench.py and the sharded
drivers need -- then imports NumPy only, not scikit-learn / SciPy / pandas behind the estimator."""

__all__ = ["CMF", "collective_matrix_factorization", "HipMUSolver", "HipNewtonSolver", "HipHALSSolver", "HipALSSolver", "top_n_products", "rank_products",
           "ranking_metrics", "implicit_confidence", "predict_products", "l2_multipliers"]


def __getattr__(name):
    if name in ("CMF", "collective_matrix_factorization"):
        from . import estimator
        return getattr(estimator, name)
    if name in ("HipMUSolver", "HipNewtonSolver", "HipHALSSolver", "HipALSSolver"):
        from . import solver_shell
        return getattr(solver_shell, name)
    if name in ("implicit_confidence", "l2_multipliers"):
        from . import solver_shell
        return getattr(solver_shell, name)
    if name == "top_n_products":
        from . import prediction
        return prediction.top_n_products
    if name == "predict_products":
        from . import prediction
        return prediction.predict_products
    if name == "rank_products":
        from . import prediction
        return prediction.rank_products
    if name == "ranking_metrics":
        from . import evaluation
        return evaluation.ranking_metrics
    raise AttributeError("module 'pycmf_amd' has no attribute %r" % name)


def __dir__():
    return sorted(list(globals()) + __all__)
