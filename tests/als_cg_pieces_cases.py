"""Fixtures of the long-row tests of the CG route (helper of test_als_cg_pieces_host.py / test_gpu_als_cg_pieces.py; not collected),
and a float32 emulation of what the device does with a long row: the sum over a row's entries cut into pieces of L consecutive
entries (side 0 then side 1, stored order), the pieces added in piece order, then S x and l2 x.

Per k: RandomState(2000 + k), signed float32-rounded data and factors, l2 = 0.1, weights 0.25 + 3.75 rand (``_pattern`` of
test_gpu_als_cg.py; every weight is at least the background 0.25 the tests use).
  case A (U and Z sweeps)   X 12 x 700 with rows of LENGTHS entries and two of 1 .. 99; Y 700 x 9 observed, its TRANSPOSE with rows of
                            ZLENGTHS entries and two of 1 .. 99, one row of Y emptied
  case B (V sweep)          X 700 x 12 whose COLUMNS hold LENGTHS reversed and two of 1 .. 99; Y 12 x 300 with rows of YLENGTHS entries
                            ('observed'), or full ('dense' | 'csr': S and N)
With pieces of 64 the V rows of case B hold 640 + 300, 333 + 0, 200 + 200, 129 + 1, 128 + 65, 65 + 64, 64 + 31, 63 + 129, 1 + 0
and 0 + 17 entries: one piece exactly (not cut), one piece and one entry, two pieces, two and one, ragged last pieces, pieces that
straddle the two sides, and short rows beside them."""
import numpy as np
import scipy.sparse as sp

import als_yardstick as A

L2 = 0.1
BACKGROUNDS = (0.0, 0.25)
KS = (7, 40, 128, 256)
STEPS = {7: (1, 2, 3, 4), 40: (1, 2, 3, 8), 128: (1, 2, 3, 8), 256: (1, 2, 3, 8)}     # k = 7: test_gpu_als_cg.py on the cliff beyond 4
LENGTHS = [0, 1, 63, 64, 65, 128, 129, 200, 333, 640]
ZLENGTHS = [0, 1, 64, 65, 200, 333, 640]
YLENGTHS = [300, 0, 200, 1, 65, 64, 31, 129, 0, 17, 100, 250]
SWEEPS = {("A", "observed"): "UZ", ("B", "observed"): "V", ("B", "dense"): "V", ("B", "csr"): "V"}
_cases = {}


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _pattern(lengths, cols, rng):
    W = np.zeros((len(lengths), cols))
    for i, n in enumerate(lengths):
        W[i, rng.permutation(cols)[:n]] = _f32(0.25 + 3.75 * rng.rand(n))
    return W


def case(name, k, yform="observed"):
    """(X, Y, Wx, Wy, [U, V, Z], refs) -- built once per (name, k, yform) and never changed."""
    key = (name, k, yform)
    if key in _cases:
        return _cases[key]
    rng = np.random.RandomState(2000 + k)
    if name == "A":
        m, d, p = 12, 700, 9
        Wx = _pattern(LENGTHS + list(rng.randint(1, 100, size=2)), d, rng)
        X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
        Wy = _pattern(ZLENGTHS + list(rng.randint(1, 100, size=2)), d, rng).T.copy()
        Wy[d // 2] = 0
    else:
        m, d, p = 700, 12, 300
        Wx = _pattern(LENGTHS[::-1] + list(rng.randint(1, 100, size=2)), m, rng).T.copy()
        X, Y = _f32(rng.randn(m, d)), _f32(rng.randn(d, p))
        Wy = _pattern(YLENGTHS, p, rng) if yform == "observed" else None
        if yform == "csr":
            Y = Y * (rng.rand(d, p) < 0.3)
    F = [_f32(rng.randn(n, k)) for n in (m, d, p)]
    _cases[key] = (X, Y, sp.csr_matrix(Wx), None if Wy is None else sp.csr_matrix(Wy), F, {})
    return _cases[key]


def relations(c):
    X, Y, Wx, Wy, F, refs = c
    if "rel" not in refs:
        refs["rel"] = (A.Relation(X, Wx), A.Relation(Y, Wy))
    return refs["rel"]


def backgrounds(c, bg):
    """(cx, cy): the background on every observed relation of the case."""
    return bg, (bg if c[3] is not None else 0.0)


def row_lengths(c, which):
    """Stored entries of every row of the sweep, both sides counted together."""
    Rx, Ry = relations(c)
    return sum(rel.row_lengths(trans) for rel, trans, _, _ in A._sides(Rx, Ry, None, None, None, which) if rel.observed)


def long_rows_and_pieces(c, which, L):
    n = row_lengths(c, which)
    cut = n[n > L]
    return int(len(cut)), int(((cut + L - 1) // L).sum())


def reference(c, which, steps, bg):
    """(y64, y32) of als_yardstick.sweep, computed once."""
    X, Y, Wx, Wy, F, refs = c
    key = ("sweep", which, steps, bg)
    if key not in refs:
        Rx, Ry = relations(c)
        cx, cy = backgrounds(c, bg)
        refs[key] = tuple(A.sweep(Rx, Ry, *F, which, L2, cg_steps=steps, cx=cx, cy=cy, dtype=dt) for dt in (np.float64, np.float32))
    return refs[key]


def _cg_row_pieces(B, w, pv, S, Nrow, l2, f, steps, L):
    """float32 CG on one row, every sum over the entries cut into pieces of L, added in piece order (the device's order between
    pieces; inside one the order is NumPy's)."""
    f32 = np.float32
    cuts = list(range(0, len(w), L))

    def entries(coef):                           # sum_e coef_e b_e
        out = np.zeros(B.shape[1], dtype=f32)
        for a in cuts:
            out = out + (B[a:a + L].T @ coef[a:a + L]).astype(f32)
        return out

    def shared(x):
        sx = (S @ x).astype(f32) if S is not None else np.zeros_like(x)
        return (sx + l2 * x).astype(f32)
    f = np.array(f, dtype=f32)
    r = (entries((pv - w * (B @ f).astype(f32)).astype(f32)) - shared(f)).astype(f32)
    if Nrow is not None:
        r = (r + Nrow).astype(f32)
    p = r.copy()
    rr = f32(r @ r)
    for _ in range(steps):
        if not A._good(rr):
            break
        q = (entries((w * (B @ p).astype(f32)).astype(f32)) + shared(p)).astype(f32)
        pq = f32(p @ q)
        if not A._good(pq):
            break
        alpha = f32(rr / pq)
        f = (f + alpha * p).astype(f32)
        r = (r - alpha * q).astype(f32)
        rn = f32(r @ r)
        p = (r + f32(rn / rr) * p).astype(f32)
        rr = rn
    return f


def emulate(c, which, steps, bg, L):
    """The sweep in float32 with piece-ordered sums in EVERY row (a row of at most L entries is one piece)."""
    X, Y, Wx, Wy, F, _ = c
    Rx, Ry = relations(c)
    cx, cy = backgrounds(c, bg)
    f32 = np.float32
    obs = A._observed_sides(Rx, Ry, *F, which, cx, cy, f32)
    S, Nf = A.shared(Rx, Ry, *F, which, cx=cx, cy=cy, dtype=f32)
    Fw = F["UVZ".index(which)]
    out = np.zeros(Fw.shape, dtype=f32)
    for i in range(Fw.shape[0]):
        Bs = np.concatenate([B[idx[ip[i]:ip[i + 1]]] for B, ip, idx, pv, e in obs])
        pv = np.concatenate([pv[ip[i]:ip[i + 1]] for B, ip, idx, pv, e in obs])
        w = np.concatenate([e[ip[i]:ip[i + 1]] for B, ip, idx, pv, e in obs])
        if S is None and len(w) == 0:
            continue
        out[i] = _cg_row_pieces(Bs, w, pv, S, None if Nf is None else Nf[i], f32(L2), Fw[i], steps, L)
    return out
