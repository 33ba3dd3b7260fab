"""Case table of the plain (Frobenius) multiplicative update, shared by tests/test_mu_sweeps_host.py (CPU) and
tests/test_gpu_mu_sweeps.py (device): shapes, ranks, masks, the two input families, the float64 yardstick, the bound and a float32
emulation of one sweep in a chosen summation order (with the mutations the host file applies to it).

What is compared
----------------
``cmf_mu_step(l1, l2, mask)`` on dense inputs with gemm_arith = 0, sweep by sweep (mask 2 = V, 1 = U, 4 = Z, 5 = U|Z, 7 = all), against
``oracle.cmf_oracle.mu_update_step`` in float64 on float32-rounded inputs.  The device evaluates

    V <- V .* (X^T U + Y Z) ./ reg(V (U^T U + Z^T Z), V)          one Gram of the stacked [U; Z], then V G
    U <- U .* (X V)        ./ reg(U (V^T V), U)                    (new V under mask 7)
    Z <- Z .* (Y^T V)      ./ reg(Z (V^T V), Z)
    reg(den, F) = den + l1 + l2 F, then den == 0 -> 2^-23

i.e. the association F (B^T B) where the oracle forms (F B^T) B: the same value in exact arithmetic.

Bound (``wmu_yardstick.tau``, imported, not copied)
---------------------------------------------------
``tau(k, L) = (k + 2 L + 16) 2^-24``, relative, per element.  Data and factors are non-negative, so every sum below has non-negative
terms: no order of summation (K-steps, split-K slabs, paired slots, Gram shares, MFMA lanes) can cancel, and a sum of n terms in ANY
order carries at most gamma_n = n u relative error to first order (u = 2^-24).  For one element of F (B^T B) with L rows in B:
  * the numerator is a sum over the L streamed rows:                     gamma_L
  * every Gram entry (B^T B)_ab is a sum over the same L rows:           gamma_L   (common to all k terms of the next sum)
  * the dot product F_i . (B^T B)_:j has k terms:                        gamma_k
  * single roundings: the products inside the three sums are counted in their gammas; what remains is l2 F, two additions of the
    regulariser, the quotient and the final product -- 5, and the sum of the two numerator products of V -- 1.  16 leaves the
    second-order terms ample room and keeps the bound the one of the weighted solver.
L = m + p for V (numerator X^T U + Y Z and the stacked Gram both run over m + p rows), L = d for U and Z.  Under mask 7 the new V
enters the numerator of U and Z once and their denominator twice (both factors of V^T V): ``tau_U + 3 tau_V``.

Exact family
------------
One side of each pair (U, V), (V, Z) has one-hot rows with value 2^randint(0, 3), the other is dense with entries 2^randint(0, 4);
X = (U V^T) .* 2^randint(-2, 3) .* Bernoulli(0.7), Y likewise.  Every entry of X and Y is then a power of two >= 2^-2 or zero and every
factor entry a power of two >= 1 or zero, so every term of every numerator, Gram and denominator is a multiple of 2^-2.  ``exact()``
asserts from float64 alone that every such sum is a multiple of 2^-2 and below 2^22: every partial sum, in any order, is then exact
in float32, and the update ``float32(F) * (float32(num) / float32(den))`` (den == 0 -> 2^-23) is fixed bit for bit.  Exact cases are
single sweeps from fresh factors (masks 2, 1, 4, 5): mask 7 feeds a rounded quotient into the next sweep.

The exact family also runs with l1 = l2 = 2^-2: den + l1 + l2 F is then a sum of multiples of 2^-2 as well (factor entries are
powers of two >= 1), asserted below 2^22 like the rest.  This is where the regulariser is pinned: at the issue's l2 = 0.1 the term
l2 F is below 4 tau of the denominator wherever L exceeds a few hundred (0.1 / L against 8 L 2^-24), so the bounded family cannot
see it go missing there (tests/test_mu_sweeps_host.py prints by how much); with l1 > 0 no denominator is zero, so the 2^-23 branch
belongs to the (0, 0) runs.
"""
import functools

import numpy as np

from oracle.cmf_oracle import mu_update_step
from test_gpu_wmu import _problem
from wmu_yardstick import EPS, tau

U_BIT, V_BIT, Z_BIT = 1, 2, 4
SHAPES = {"A": (70, 333, 40), "B": (300, 1100, 530)}
KS = (7, 40, 100, 200, 300)
MASKS = (2, 1, 4, 5, 7)
EXACT_MASKS = (2, 1, 4, 5)
REGS = ((0.0, 0.0), (0.05, 0.1))
EXACT_REGS = ((0.0, 0.0), (0.25, 0.25))
OWNERS = ("V", "UZ")
f32 = np.float32


def seed_of(shape, k):
    return 1000 * sorted(SHAPES).index(shape) + k


@functools.lru_cache(maxsize=4)
def bounded(shape, k):
    """(X, Y, [U, V, Z]) of test_gpu_wmu._problem: float32-rounded float64 arrays; treat as read-only."""
    m, d, p = SHAPES[shape]
    return _problem(m, d, p, k, seed=seed_of(shape, k))


@functools.lru_cache(maxsize=64)
def yardstick(shape, k, mask, l1, l2):
    """The oracle's sweep(s) on the bounded family: (U, V, Z) in float64; treat as read-only."""
    X, Y, F = bounded(shape, k)
    U, V, Z = (f.copy() for f in F)
    mu_update_step(X, Y, U, V, Z, l1, l2, update_U=bool(mask & U_BIT), update_V=bool(mask & V_BIT), update_Z=bool(mask & Z_BIT))
    return U, V, Z


def tolerances(shape, k, mask):
    """(tol_U, tol_V, tol_Z) of one call with this mask."""
    m, d, p = SHAPES[shape]
    tU, tV = tau(k, d), tau(k, m + p)
    chained = 3 * tV if mask & V_BIT else 0.0
    return tU + chained, tV, tU + chained


def sums(X, Y, F, mask):
    """float64 numerators, Grams and denominators of the sweeps of `mask` from the factors F (fresh: not chained):
    {"V": (num, gram, den), "U": ..., "Z": ...}."""
    U, V, Z = F
    out = {}
    if mask & V_BIT:
        G = U.T @ U + Z.T @ Z
        out["V"] = (X.T @ U + Y @ Z, G, V @ G)
    if mask & (U_BIT | Z_BIT):
        G2 = V.T @ V
        if mask & U_BIT:
            out["U"] = (X @ V, G2, U @ G2)
        if mask & Z_BIT:
            out["Z"] = (Y.T @ V, G2, Z @ G2)
    return out


def exact_update(F, num, den, l1=0.0, l2=0.0):
    """float32(F) * (float32(num) / reg(float32(den))), reg(den) = den + l1 + l2 F then den == 0 -> 2^-23: mu_apply_kernel, the EPI_MU
    epilogue and factor_update_kernel."""
    den = den.astype(f32).copy()
    if l1 > 0:
        den = den + f32(l1)
    if l2 > 0:
        den = den + f32(l2) * F.astype(f32)
    den[den == 0] = f32(EPS)
    with np.errstate(over="ignore"):
        return (F.astype(f32) * (num.astype(f32) / den)).astype(np.float64)


def assert_exact_premises(S):
    """Every sum is a multiple of 2^-2 and below 2^22.  Returns the largest."""
    assert (S >= 0).all() and S.max() < 2.0 ** 22 and (S * 4 == np.round(S * 4)).all()
    return float(S.max())


@functools.lru_cache(maxsize=4)
def exact(shape, k, owner):
    """(X, Y, [U, V, Z], expected, info): expected[mask, (l1, l2)] = (U, V, Z) after one call with that mask from the fresh factors,
    for the masks of EXACT_MASKS and the pairs of EXACT_REGS; info = (largest sum, number of zero denominators under non-zero factor
    entries).  Premises asserted."""
    m, d, p = SHAPES[shape]
    rng = np.random.RandomState(seed_of(shape, k) + (7 if owner == "V" else 13))

    def dense(r):
        return 2.0 ** rng.randint(0, 4, size=(r, k))

    def onehot(r):
        F = np.zeros((r, k))
        F[np.arange(r), rng.randint(0, k, size=r)] = 2.0 ** rng.randint(0, 3, size=r)
        return F
    F = [onehot(m), dense(d), onehot(p)] if owner == "V" else [dense(m), onehot(d), dense(p)]
    X = (F[0] @ F[1].T) * 2.0 ** rng.randint(-2, 3, size=(m, d)) * (rng.rand(m, d) < 0.7)
    Y = (F[1] @ F[2].T) * 2.0 ** rng.randint(-2, 3, size=(d, p)) * (rng.rand(d, p) < 0.7)
    for A in [X, Y] + F:
        assert (A.astype(f32) == A).all()
    largest, zero_dens = 0.0, 0
    expected = {}
    for mask in EXACT_MASKS:
        S = sums(X, Y, F, mask)
        for l1, l2 in EXACT_REGS:
            new = [f.copy() for f in F]
            for name, w in (("U", 0), ("V", 1), ("Z", 2)):
                if name in S:
                    num, _, den = S[name]
                    for T in S[name] + (den + l1 + l2 * F[w],):
                        largest = max(largest, assert_exact_premises(T))
                    if l1 == 0:
                        zero_dens += int(((den == 0) & (F[w] != 0)).sum())
                    new[w] = exact_update(F[w], num, den, l1, l2)
                    assert np.isfinite(new[w]).all()
            expected[mask, (l1, l2)] = new
    return X, Y, F, expected, (largest, zero_dens)


# ------------------------------------------------------------------ float32 emulation of one call (host file)
def mm(A, B, order):
    """float32 A @ B with the reduction summed in a stated order: "asc", "desc", "blocks" (blocks of 32 terms summed ascending, then
    the block sums ascending), or "blas" (whatever float32 BLAS does: one more order, fast)."""
    A, B = np.ascontiguousarray(A, dtype=f32), np.ascontiguousarray(B, dtype=f32)
    if order == "blas":
        return A @ B
    L = A.shape[1]
    idx = range(L) if order != "desc" else range(L - 1, -1, -1)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=f32)
    if order in ("asc", "desc"):
        for l in idx:
            acc += A[:, l, None] * B[l]
        return acc
    assert order == "blocks"
    for l0 in range(0, L, 32):
        part = np.zeros_like(acc)
        for l in range(l0, min(l0 + 32, L)):
            part += A[:, l, None] * B[l]
        acc += part
    return acc


MUTATIONS = ("drop_last", "swap_k", "gram_without_z", "yz_overwrites", "no_l2", "stale_v", "block_not_updated")
# the sweeps a mutation can act in (as a mask) and whether it needs l2 > 0
MUTATION_SCOPE = {"drop_last": (2, 1, 4), "swap_k": (2, 1, 4), "gram_without_z": (2,), "yz_overwrites": (2,), "no_l2": (2, 1, 4),
                  "stale_v": (7,), "block_not_updated": (2,)}


def emulate(X, Y, F, l1, l2, mask, order, mutation=None):
    """One call in float32, every reduction through mm(order).  Returns float64 copies of (U, V, Z).
    Mutations (each what a plausible kernel slip would compute):
      drop_last          the last term of the sweep's first data product is dropped (X^T U for V, X V for U, Y^T V for Z)
      swap_k             two columns of the factor operand of that product are swapped (the Gram sees the right factor): the first
                         two columns in which the updated factor has a non-zero entry -- 0 and 1 for a dense factor; a one-hot factor
                         shows only the columns its rows point at
      gram_without_z     the Z block is missing from the stacked Gram of the V sweep
      yz_overwrites      Y Z overwrites X^T U instead of adding to it
      no_l2              l2 F is missing from the denominator
      stale_v            mask 7: the U sweep runs from the V the call started with
      block_not_updated  rows 256 .. 511 of V keep their old values"""
    l1, l2 = f32(l1), f32(l2)
    U, V, Z = (np.array(f, dtype=f32) for f in F)
    V_old = V.copy()

    def product(A, B, first, Fw):
        if first and mutation == "drop_last":
            A, B = A[:, :-1], B[:-1]
        if first and mutation == "swap_k":
            cols = np.argwhere(Fw != 0)[:, 1]
            a, b = cols[0], cols[cols != cols[0]][0]
            B = B.copy()
            B[:, [a, b]] = B[:, [b, a]]
        return mm(A, B, order)

    def update(Fw, num, G):
        den = mm(Fw, G, order)
        if l1 > 0:
            den = den + l1
        if l2 > 0 and mutation != "no_l2":
            den = den + l2 * Fw
        den[den == 0] = f32(EPS)
        with np.errstate(over="ignore"):
            return Fw * (num / den)
    if mask & V_BIT:
        xtu, yz = product(X.T, U, True, V), product(Y, Z, False, V)
        num = yz if mutation == "yz_overwrites" else xtu + yz
        S = U if mutation == "gram_without_z" else np.vstack([U, Z])
        new = update(V, num, mm(S.T, S, order))
        if mutation == "block_not_updated":
            new[256:512] = V[256:512]
        V = new
    if mask & (U_BIT | Z_BIT):
        G2 = mm(V.T, V, order)
        if mask & U_BIT:
            Vu = V_old if mutation == "stale_v" else V
            U = update(U, product(X, Vu, not mask & V_BIT, U), mm(Vu.T, Vu, order) if mutation == "stale_v" else G2)
        if mask & Z_BIT:
            Z = update(Z, product(Y.T, V, not mask & (V_BIT | U_BIT), Z), G2)
    return tuple(np.asarray(f, dtype=np.float64) for f in (U, V, Z))


def worst_ratio(got, ref, tol):
    """max |got - ref| / (tol ref) over the elements with ref != 0; inf if an element with ref == 0 is not exactly 0."""
    zero = ref == 0
    if (got[zero] != 0).any():
        return float("inf")
    if zero.all():
        return 0.0
    return float((np.abs(got[~zero] - ref[~zero]) / (tol * ref[~zero])).max())
