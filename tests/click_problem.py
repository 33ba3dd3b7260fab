"""The planted click problem of the implicit-feedback tests (helper of test_als_implicit_host.py / test_gpu_als_implicit.py; not
collected): counts on a thresholded low-rank score with item popularity, a held-out quarter of the clicks, recall at n."""
import numpy as np
import scipy.sparse as sp


def clicks(seed, m=120, d=150, p=20, kt=3, dens=0.08, hold=0.25, k=8):
    r = np.random.RandomState(seed)
    Ut, Vt, Zt = r.randn(m, kt), r.randn(d, kt), r.randn(p, kt)
    pop = 0.8 * r.randn(d)
    S = Ut @ Vt.T + pop[None]
    thr = np.quantile(S + 0.5 * r.randn(m, d), 1 - dens)
    on = (S + 0.5 * r.randn(m, d)) > thr
    counts = on * (1 + r.poisson(np.maximum(0, 2 * (S - S.mean()))))
    _ = Vt @ Zt.T + 0.1 * r.randn(d, p)          # drawn and discarded: keeps the stream
    test = on & (r.rand(m, d) < hold); train = on & ~test
    Y = r.randn(d, p)                             # side information without signal
    U0, V0, Z0 = (0.1 * r.randn(n, k) for n in (m, d, p))
    return counts, train, test, Y, U0, V0, Z0


def recall_at(scores, train, test, n=10):
    """Mean over the rows with held-out clicks of (held-out clicks among the top n) / (held-out clicks); training cells are
    excluded, ties go to the smaller index."""
    sc = np.where(train, -np.inf, np.asarray(scores, np.float64))
    top = np.argsort(-sc, axis=1, kind="stable")[:, :n]
    hits = np.take_along_axis(test, top, axis=1).sum(axis=1)
    held = test.sum(axis=1)
    rows = held > 0
    return float((hits[rows] / held[rows]).mean())


def click_relations(counts, train):
    """(P, W): targets 1 and confidences 1 + count on the training clicks, SciPy CSR."""
    P = sp.csr_matrix(train.astype(np.float64))
    W = sp.csr_matrix(np.where(train, 1.0 + counts, 0.0))
    return P, W
