"""Fixtures of the bias tests (helper of test_als_bias_host.py / test_gpu_als_bias.py; not collected): the patterns, data and
factors of als_cg_pieces_cases.py (rows of 0, 1, 63, 64, 65, 128, 129, 200, 333, 640 entries) with biases on every observed relation,
and the yardstick's float64 / float32 results on them, computed once per key and never changed.

Per (name, k): RandomState(3000 + k); mu_x = 0.75, mu_y = -0.5; r, c = 0.5 randn rounded to float32; lb = 0.3; l2 = 0.1."""
import numpy as np

import als_bias_yardstick as B
import als_cg_pieces_cases as P

L2 = P.L2
LB = 0.3
PIECE = 64
KS = P.KS
ROUTES = {"exact": dict(cg_steps=0, nn_mask=0, nn_sweeps=0), "cg": dict(cg_steps=3, nn_mask=0, nn_sweeps=0),
          "nn": dict(cg_steps=0, nn_mask=2, nn_sweeps=4)}
_bias = {}
_refs = {}


def biases(name, k):
    """(bx, by) of the case: (mu, r, c) per relation."""
    key = (name, k)
    if key not in _bias:
        X, Y = P.case(name, k)[:2]
        rng = np.random.RandomState(3000 + k)
        _bias[key] = tuple((mu, P._f32(0.5 * rng.randn(T.shape[0])), P._f32(0.5 * rng.randn(T.shape[1]))) for mu, T in ((0.75, X), (-0.5, Y)))
    return _bias[key]


def factors(name, k, nn_mask=0):
    F = P.case(name, k)[4]
    return [np.abs(F[w]) if nn_mask & (1 << w) else F[w] for w in range(3)]


def sweep_reference(name, k, which, axis, piece=PIECE):
    """(y64, y32) of one bias sweep of relation ``which`` along ``axis`` from the case's state; y32 sums pieces of ``piece``."""
    key = ("sweep", name, k, which, axis, piece)
    if key not in _refs:
        c = P.case(name, k)
        rel = P.relations(c)[which]
        F = c[4]
        Fa, Fb = (F[0], F[1]) if which == 0 else (F[1], F[2])
        b = biases(name, k)[which]
        _refs[key] = (B.bias_sweep(rel, Fa, Fb, b, LB, axis), B.bias_sweep(rel, Fa, Fb, b, LB, axis, dtype=np.float32, piece=piece))
    return _refs[key]


def step_reference(name, k, mask, route):
    """((U, V, Z, bx, by) in float64, the same in float32 with pieces of 64) of one step from the case's state."""
    key = ("step", name, k, mask, route)
    if key not in _refs:
        c = P.case(name, k)
        Rx, Ry = P.relations(c)
        kw = ROUTES[route]
        F = factors(name, k, kw["nn_mask"])
        bx, by = biases(name, k)
        _refs[key] = tuple(B.step(Rx, Ry, None, None, *F, bx, by, L2, LB, mask=mask, dtype=dt, piece=(PIECE if dt is np.float32 else None), **kw)
                           for dt in (np.float64, np.float32))
    return _refs[key]


def step_vectors(state):
    """[(name, array)] of a step's result: the three factors and the four bias vectors."""
    U, V, Z, bx, by = state
    return [("U", U), ("V", V), ("Z", Z), ("r_x", bx[1]), ("c_x", bx[2]), ("r_y", by[1]), ("c_y", by[2])]


# which of the seven vectors a step with ``mask`` moves
MOVED = {"U": 1, "V": 2, "Z": 4, "r_x": 1, "c_x": 2, "r_y": 2, "c_y": 4}


# The step cases: (case, k, mask, route) whose float32 and float64 yardstick runs agree within the cap for every vector the step
# moves (a property of the fixture alone, computed on the CPU and asserted by test_als_bias_host.py).  Case B carries the long rows
# in the V sweep, case A in the U and Z sweeps: the CG route runs masks 7 and 2 on B and masks 1 and 4 on A (4 max|y32 - y64| at
# most 0.044 of the cap there, at every k), so r_x behind a CG U sweep and c_y behind a CG Z sweep are checked up to k = 256.
# Left out, with 4 max|y32 - y64| as a multiple of the cap: the rows of U and Z of case B hold at most 12 entries (as the V rows of
# case A: at most 21), so their exact solves at k >= 128 are conditioned by l2 alone (exact, B, k = 128: U 1.2, Z 1.4 on masks 1 and
# 4, Z 1.0 on mask 7; k = 256: 1.8 .. 2.9 on every mask), and three CG steps on them part ways in the two precisions, which the bias
# sweep that follows inherits (cg, B, k = 7: r_x 1.3 on mask 1, c_y 2.1 on mask 4; k >= 40: r_x 7 .. 363, c_y 12 .. 99 on masks 7, 1
# and 4; cg, A, masks 7 and 2: c_x 2.4 .. 42, r_y 0.2 .. 39); nn, B, Z on mask 4 at k = 128: 1.05, k = 256: 1.9, U on mask 1 at
# k = 256: 2.7.
STEP_CASES = ([("B", 7, m, "exact") for m in (7, 1, 2, 4)] + [("B", 40, m, "exact") for m in (7, 1, 2, 4)] + [("B", 128, 2, "exact")] +
              [("B", 7, 7, "cg"), ("B", 7, 2, "cg"), ("B", 40, 2, "cg"), ("B", 128, 2, "cg"), ("B", 256, 2, "cg")] +
              [("A", k, m, "cg") for k in KS for m in (1, 4)] +
              [("B", 7, m, "nn") for m in (7, 1, 2, 4)] + [("B", 40, m, "nn") for m in (7, 1, 2, 4)] +
              [("B", 128, 7, "nn"), ("B", 128, 1, "nn"), ("B", 128, 2, "nn")] + [("B", 256, 7, "nn"), ("B", 256, 2, "nn")])
