"""Host side of tests/test_gpu_mu_sweeps.py (no GPU): shows that the device file can fail.

1. The premises of the exact family hold for every case of the table (mu_sweep_cases.exact asserts them from float64 alone).
2. A float32 emulation of every sweep of the bounded family stays within ``tau`` of the float64 yardstick in three summation orders
   (ascending, descending, blocks of 32 then blocks): the bound is attainable.  Worst ratio over the table: 0.0412 (shape A,
   k = 100, l2 = 0.1; printed per case).
3. Seven mutations of the emulation -- each what a plausible kernel slip computes -- move at least one element by more than 4 tau on
   the bounded family and change at least one element of the exact family, in EVERY sweep they can act in, at EVERY shape and k of
   the table: the bound and the ``==`` have teeth there.  This is a condition on the inputs: if a case fails it, the case (seed,
   shape) is changed, never the bound.  Smallest multiple of tau observed over the table, per mutation (printed per case):
   drop_last 63 (shape B, k = 7), swap_k 665, stale_v 1980, yz_overwrites 8490, gram_without_z 18080, block_not_updated 149132.
   Two exceptions, both by arithmetic and not by choice of seed:
     * no_l2 on the bounded family: l2 F = 0.1 F against a denominator summed over L rows is below 4 tau = 8 L 2^-24 and more once L
       passes a few hundred, and further below it the wider the rows (shape B, k = 200: no element moves at all in float32).  It
       is asserted where it can show (shape A, k = 7: 44 tau in the V sweep, 5.6 in U, 5.0 in Z) and printed elsewhere; the exact
       family run with l1 = l2 = 2^-2 catches it in every sweep at every shape and k.
     * stale_v has no exact counterpart: the exact family has no mask 7.
"""
import numpy as np
import pytest

import mu_sweep_cases as MC

CASES = [(s, k) for s in sorted(MC.SHAPES) for k in MC.KS]


def test_the_table_is_the_one_the_issue_names():
    assert MC.SHAPES == {"A": (70, 333, 40), "B": (300, 1100, 530)} and MC.KS == (7, 40, 100, 200, 300)
    assert MC.MASKS == (2, 1, 4, 5, 7) and MC.EXACT_MASKS == (2, 1, 4, 5) and MC.REGS == ((0.0, 0.0), (0.05, 0.1))
    assert MC.tau(7, 100) == (7 + 200 + 16) * 2.0 ** -24


@pytest.mark.parametrize("owner", MC.OWNERS)
@pytest.mark.parametrize("shape, k", CASES)
def test_exact_family_premises(shape, k, owner):
    X, Y, F, expected, (largest, zero_dens) = MC.exact(shape, k, owner)
    print("exact %s k=%d owner %s: largest sum %.0f, zero denominators under non-zero entries %d" % (shape, k, owner, largest, zero_dens))
    assert largest < 2.0 ** 22
    # the one-hot side really is one-hot, the dense side really is dense, and the data has zeros and non-zeros
    hot = (0, 2) if owner == "V" else (1,)
    for w in range(3):
        nz = (F[w] != 0).sum(axis=1)
        assert (nz == 1).all() if w in hot else (nz == k).all()
    for T in (X, Y):
        assert 0.5 < (T != 0).mean() < 0.9
    # every expected array differs from the start where it is updated and equals it where it is not
    assert set(expected) == {(mask, reg) for mask in MC.EXACT_MASKS for reg in MC.EXACT_REGS}
    for (mask, _), new in expected.items():
        for w, bit in ((0, MC.U_BIT), (1, MC.V_BIT), (2, MC.Z_BIT)):
            assert (new[w] != F[w]).any() if mask & bit else (new[w] == F[w]).all()


def test_zero_denominators_are_reached():
    """The eps branch (den == 0 under a non-zero factor entry) is part of the exact family from k = 200 up, at the dense-owner side."""
    hit = {(s, k, o): MC.exact(s, k, o)[4][1] for s, k in CASES for o in MC.OWNERS}
    assert all(max(hit[(s, k, o)] for o in MC.OWNERS) > 0 for s, k in CASES if k >= 200), hit


@pytest.mark.parametrize("l1, l2", MC.REGS)
@pytest.mark.parametrize("shape, k", CASES)
def test_float32_emulation_stays_within_tau_in_three_orders(shape, k, l1, l2):
    X, Y, F = MC.bounded(shape, k)
    worst = 0.0
    for order in ("asc", "desc", "blocks"):
        for mask in (7, 5):                       # 7: V, then U and Z from the new V; 5: U and Z from the fresh V
            got = MC.emulate(X, Y, F, l1, l2, mask, order)
            ref = MC.yardstick(shape, k, mask, l1, l2)
            for w, tol in enumerate(MC.tolerances(shape, k, mask)):
                if mask & (MC.U_BIT, MC.V_BIT, MC.Z_BIT)[w]:
                    r = MC.worst_ratio(got[w], ref[w], tol)
                    assert r <= 1.0, (order, mask, w, r)
                    worst = max(worst, r)
                else:
                    assert (got[w] == F[w]).all()
    print("bounded %s k=%d l1=%g l2=%g: worst |err| / tau over three orders = %.4f" % (shape, k, l1, l2, worst))


def _moved(clean, mutated, tols, mask):
    """Largest relative move of an updated element in units of its tau (inf where a zero became non-zero)."""
    worst = 0.0
    for w, bit in ((0, MC.U_BIT), (1, MC.V_BIT), (2, MC.Z_BIT)):
        if mask & bit:
            worst = max(worst, MC.worst_ratio(mutated[w], clean[w], tols[w]))
    return worst


@pytest.mark.parametrize("mutation", MC.MUTATIONS)
@pytest.mark.parametrize("shape, k", CASES)
def test_every_mutation_is_caught(shape, k, mutation):
    X, Y, F = MC.bounded(shape, k)
    l1, l2 = (0.05, 0.1) if mutation == "no_l2" else (0.0, 0.0)
    smallest = np.inf
    for mask in MC.MUTATION_SCOPE[mutation]:
        clean = MC.emulate(X, Y, F, l1, l2, mask, "blas")
        mutated = MC.emulate(X, Y, F, l1, l2, mask, "blas", mutation)
        moved = _moved(clean, mutated, MC.tolerances(shape, k, mask), mask)
        smallest = min(smallest, moved)
        # l2 = 0.1 is below 4 tau of a denominator summed over more than a few hundred rows (mu_sweep_cases, "Exact family"): what the
        # bounded family sees of no_l2 is printed, and asserted in test_a_missing_l2_shows_on_the_bounded_family_where_it_can
        assert moved > 4.0 or mutation == "no_l2", "%s, mask %d: moves no element by more than 4 tau (%.3f)" % (mutation, mask, moved)
    print("bounded %s k=%d %s: smallest move over its sweeps = %.1f tau" % (shape, k, mutation, smallest))
    if mutation == "stale_v":
        return                                    # no exact counterpart: no mask 7 there
    reg = (0.25, 0.25) if mutation == "no_l2" else (0.0, 0.0)
    for owner in MC.OWNERS:
        Xe, Ye, Fe, expected, _ = MC.exact(shape, k, owner)
        for mask in MC.MUTATION_SCOPE[mutation]:
            clean = MC.emulate(Xe, Ye, Fe, *reg, mask, "blas")
            for w in range(3):                    # the emulation reproduces the expected arrays bit for bit ...
                assert (clean[w] == expected[mask, reg][w]).all()
            mutated = MC.emulate(Xe, Ye, Fe, *reg, mask, "blas", mutation)
            assert any((mutated[w] != expected[mask, reg][w]).any() for w in range(3)), (owner, mask)   # ... and the mutated one does not


def test_a_missing_l2_shows_on_the_bounded_family_where_it_can():
    """Shape A, k = 7: the sums are short enough (L = 110 for V, 333 for U and Z) and the rows narrow enough for l2 F = 0.1 F to weigh
    more than 4 tau of the denominator in every sweep."""
    X, Y, F = MC.bounded("A", 7)
    for mask in MC.MUTATION_SCOPE["no_l2"]:
        moved = _moved(MC.emulate(X, Y, F, 0.05, 0.1, mask, "blas"), MC.emulate(X, Y, F, 0.05, 0.1, mask, "blas", "no_l2"),
                       MC.tolerances("A", 7, mask), mask)
        print("bounded A k=7 no_l2, mask %d: %.1f tau" % (mask, moved))
        assert moved > 4.0


@pytest.mark.parametrize("order", ["asc", "desc", "blocks"])
def test_exact_family_is_order_independent(order):
    """The expected arrays are reproduced bit for bit by the float32 emulation in every order (shape A, the k with zero denominators)."""
    for owner in MC.OWNERS:
        X, Y, F, expected, _ = MC.exact("A", 200, owner)
        for mask in MC.EXACT_MASKS:
            for reg in MC.EXACT_REGS:
                got = MC.emulate(X, Y, F, *reg, mask, order)
                for w in range(3):
                    assert (got[w] == expected[mask, reg][w]).all()


def test_route_counter_is_declared_in_all_three_places():
    import os
    import re
    from pycmf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cmfhip.h")).read()
    decl = re.search(r"\bcmf_mu_route_launches\s*\(([^)]*)\)", header)
    assert decl is not None and len(decl.group(1).split(",")) == 2 == len(_lib.PROTOTYPES["cmf_mu_route_launches"])
    assert "out8" in decl.group(1) and len(_lib.Context.MU_ROUTE_FORMS) == 8 and callable(_lib.Context.mu_route_launches)
    assert "cmf_mu_route_launches" in open(os.path.join(root, "INTEGRATION.md")).read()
