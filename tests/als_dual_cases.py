"""The problem of the dual-row tests (helper of test_als_dual_host.py / test_gpu_als_dual.py; not collected).

X is 48 x 160 with row lengths 0, 1, 2, 5, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 160, repeated: both sides of every class
edge (32 | 64 | 128), the empty row and rows longer than any class.  Its columns are drawn with a skew, so a few columns are hot.
Y (160 x 40) is observed too: a V row straddles both sides (its entries in X's transpose, then its entries in Y; at least the three
full rows of X, so no V row is empty).  Y is filled at rates that rise along its columns and fall along its rows: the early V rows
are hot on both sides (more than 64 entries), the late ones short, and the Z rows run from none and one entry to more than 128.
Weights in 0.5 .. 1.5 with a few STORED exact zeros; signed float32-representable data and factors."""
import numpy as np
import scipy.sparse as sp

LENGTHS = [0, 1, 2, 5, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 160]
M, D, P = 48, 160, 40
L2 = 0.05
_cache = {}


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _csr(rows, cols, vals, shape):
    """A CSR matrix that keeps its stored zeros."""
    M_ = sp.csr_matrix((vals, (rows, cols)), shape=shape)
    M_.sort_indices()
    return M_


def patterns(seed=11):
    """(Wx 48 x 160, Wy 160 x 40) as SciPy CSR with stored zero weights."""
    if ("w", seed) in _cache:
        return _cache[("w", seed)]
    rng = np.random.RandomState(seed)
    lens = (LENGTHS * 4)[:M]
    skew = 1.0 / (1.0 + np.arange(D)) ** 1.2
    skew /= skew.sum()
    r, c = [], []
    for i, n in enumerate(lens):
        cols = np.arange(D) if n == D else rng.choice(D, size=n, replace=False, p=skew)
        r += [i] * n
        c += list(cols)
    w = f32(0.5 + rng.rand(len(r)))
    w[rng.choice(len(r), size=25, replace=False)] = 0.0
    Wx = _csr(r, c, w, (M, D))
    mask = rng.rand(D, P) < np.linspace(0.0, 1.3, P)[None, :] * np.linspace(1.5, 0.15, D)[:, None]
    mask[7] = False                                  # a V row with nothing on the Y side
    mask[:, 0] = False                               # Z row 0: no stored entry
    mask[:, 1] = False
    mask[3, 1] = True                                # Z row 1: one
    ry, cy = np.nonzero(mask)
    wy = f32(0.5 + rng.rand(len(ry)))
    wy[rng.choice(len(ry), size=25, replace=False)] = 0.0
    Wy = _csr(ry, cy, wy, (D, P))
    _cache[("w", seed)] = (Wx, Wy)
    return Wx, Wy


def problem(k, seed=11):
    """(X, Y, Wx, Wy, [U, V, Z]) at k components."""
    if (k, seed) in _cache:
        return _cache[(k, seed)]
    Wx, Wy = patterns(seed)
    rng = np.random.RandomState(1000 * seed + k)
    X, Y = f32(rng.randn(M, D)), f32(rng.randn(D, P))
    F = [f32(rng.randn(n, k) / np.sqrt(k)) for n in (M, D, P)]
    _cache[(k, seed)] = (X, Y, Wx, Wy, F)
    return _cache[(k, seed)]
