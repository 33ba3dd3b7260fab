"""Yardstick of the top-n tests: NumPy float64 on the float32-rounded factors (what the device holds), never the code under test.

Tolerance (derived, not tuned).  A float32 dot product of length k_pad, in any summation order, is within
    tau_i = 1.01 * k_pad * 2^-24 * ||q_i||_2 * max_j ||b_j||_2
of the exact one (gamma_k sum |q_t b_t| with Cauchy-Schwarz; the 1.01 covers gamma_k = k u / (1 - k u) up to k = 256).  If
s_1 >= s_2 >= ... are query i's exact raw scores over the eligible candidates and r_1 .. r_n the exact scores of the candidates the
device returned, in the order returned, a correct selection on float32 scores implies |r_t - s_t| <= 2 tau_i for every t (order
statistics move by at most the perturbation, each returned item's own score by at most tau again).  Values: |val - r_t| <= tau_i
for the identity link, <= tau_i / 4 + 2^-22 for the sigmoid (slope <= 1/4, plus a few units in the last place of a value below 1
for the float32 evaluation with the fast exp and reciprocal).
"""
import numpy as np


def f32(F):
    return np.asarray(F).astype(np.float32).astype(np.float64)


def pad_k(k):
    for kp in (32, 64, 128):
        if k <= kp:
            return kp
    return (k + 255) // 256 * 256


def exact_scores(Q, B, excl=None):
    """float64 raw scores of the float32-rounded operands; excluded entries (CSR pair over the queries) at -inf."""
    S = f32(Q) @ f32(B).T
    if excl is not None:
        indptr, indices = excl
        for i in range(S.shape[0]):
            S[i, indices[indptr[i]:indptr[i + 1]]] = -np.inf
    return S


def exact_top_n(S, n):
    """(idx, score) of the n largest entries per row, larger first, equal scores by smaller index; -1 / -inf where a row has fewer
    than n finite entries."""
    order = np.argsort(-S, axis=1, kind="stable")[:, :n]
    sc = np.take_along_axis(S, order, axis=1)
    idx = np.where(np.isfinite(sc), order, -1).astype(np.int64)
    return idx, sc


def tau(Q, B, k_pad=None):
    Q, B = f32(Q), f32(B)
    k_pad = pad_k(Q.shape[1]) if k_pad is None else k_pad
    return 1.01 * k_pad * 2.0 ** -24 * np.linalg.norm(Q, axis=1) * np.linalg.norm(B, axis=1).max()


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def check_top_n(idx, val, Q, B, n, link="linear", excl=None, label=""):
    """Every row of the case: indices distinct, in range, not excluded; |r_t - s_t| <= 2 tau_i for every t; values within their
    bound; -1 / -inf exactly in the places the eligible candidates cannot fill.  Returns the largest observed |r_t - s_t| / tau_i."""
    nq, C = Q.shape[0], B.shape[0]
    assert idx.shape == (nq, n) and val.shape == (nq, n), label
    assert idx.dtype == np.int32 and val.dtype == np.float32, label
    S = exact_scores(Q, B, excl)
    _, s_sorted = exact_top_n(S, n)
    t = tau(Q, B)
    worst = 0.0
    for i in range(nq):
        eligible = int(np.isfinite(S[i]).sum())
        have = min(n, eligible)
        got = idx[i, :have].astype(np.int64)
        assert (idx[i, have:] == -1).all() and np.isneginf(val[i, have:]).all(), "%s row %d: places beyond the %d eligible" % (label, i, eligible)
        assert (got >= 0).all() and (got < C).all(), "%s row %d: index out of range" % (label, i)
        assert len(set(got.tolist())) == have, "%s row %d: repeated index" % (label, i)
        r = S[i, got]
        assert np.isfinite(r).all(), "%s row %d: an excluded candidate was returned" % (label, i)
        dev = np.abs(r - s_sorted[i, :have])
        bound = 2.0 * t[i]
        assert (dev <= bound).all(), "%s row %d: |r_t - s_t| = %.3e above 2 tau = %.3e" % (label, i, dev.max(), bound)
        if t[i] > 0 and have:
            worst = max(worst, float(dev.max() / t[i]))
        v = val[i, :have].astype(np.float64)
        if link == "linear":
            assert (np.abs(v - r) <= t[i]).all(), "%s row %d: value off by %.3e, tau %.3e" % (label, i, np.abs(v - r).max(), t[i])
        else:
            assert (np.abs(v - sigmoid(r)) <= t[i] / 4 + 2.0 ** -22).all(), \
                "%s row %d: sigmoid value off by %.3e, bound %.3e" % (label, i, np.abs(v - sigmoid(r)).max(), t[i] / 4 + 2.0 ** -22)
    return worst
