"""Long rows of the CG route, host side: the tolerance of test_gpu_als_cg_pieces.py on record, re-checkable without a GPU.

The device cuts a row longer than L entries into pieces and adds the pieces' partial sums in piece order.  A float32 CG that sums
in exactly that way (als_cg_pieces_cases.emulate, L = 64, every row) is compared with the float64 yardstick on the fixtures of the
device tests, all sweeps, step counts and backgrounds: it must lie within the project's tolerance
tol = max(4 max|y32 - y64|, (k + 16) 2^-24 max|y64|) (als_yardstick.tolerance) whose float32-against-float64 term must itself stay
below the cap 1e-3 max|y64| -- so the rule needs no extra term for the piece order, and cannot quietly widen."""
import os
import re

import numpy as np
import pytest

import als_yardstick as A
import als_cg_pieces_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1e-3


@pytest.mark.parametrize("name, yform", sorted(P.SWEEPS))
@pytest.mark.parametrize("k", P.KS)
def test_piece_ordered_float32_sums_stay_within_the_tolerance(k, name, yform):
    c = P.case(name, k, yform)
    worst = worst_cap = 0.0
    for which in P.SWEEPS[(name, yform)]:
        for bg in P.BACKGROUNDS:
            for steps in P.STEPS[k]:
                y64, y32 = P.reference(c, which, steps, bg)
                cap = 4.0 * float(np.abs(y32.astype(np.float64) - y64).max()) / (CAP * float(np.abs(y64).max()))
                tol = A.tolerance(y32, y64, k)
                err = float(np.abs(P.emulate(c, which, steps, bg, 64).astype(np.float64) - y64).max())
                print("case %s Y %s k %d sweep %s bg %g, %d steps: cap %.3f, |err| / tol %.3f" % (name, yform, k, which, bg, steps, cap, err / tol))
                worst, worst_cap = max(worst, err / tol), max(worst_cap, cap)
                assert cap <= 1.0 and err <= tol
    print("case %s Y %s k %d: worst |err| / tol %.3f, worst cap %.3f" % (name, yform, k, worst, worst_cap))


def test_fixtures_hold_the_row_lengths_the_device_tests_count_on():
    """At L = 64: rows of one piece exactly (not cut), one piece and an entry, two pieces, two and an entry, a ragged last piece, a
    row whose pieces straddle the two sides, rows without an entry."""
    a, b = P.case("A", 40), P.case("B", 40)
    assert list(P.row_lengths(a, "U")[:10]) == P.LENGTHS
    assert all(z - 1 <= n <= z for n, z in zip(P.row_lengths(a, "Z"), P.ZLENGTHS))      # the emptied row of Y may take one entry away
    nv = list(P.row_lengths(b, "V"))
    assert nv[:10] == [x + y for x, y in zip(P.LENGTHS[::-1], P.YLENGTHS)] and nv[0] == 640 + 300
    assert P.long_rows_and_pieces(a, "U", 64)[0] == 6 + sum(n > 64 for n in P.row_lengths(a, "U")[10:])
    assert P.long_rows_and_pieces(b, "V", 64) != P.long_rows_and_pieces(b, "V", 128)
    assert min(A.Relation(b[1], b[3]).w.min(), A.Relation(b[0], b[2]).w.min()) >= 0.25       # the background the tests set


def test_entry_point_and_option_are_declared():
    from pycmf_amd import _lib
    header = open(os.path.join(ROOT, "include", "cmfhip.h")).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"\b(CMF_K_[A-Z_0-9]+)\s*=\s*(\d+)", header))
    assert enum["CMF_K_COUNT"] == 11
    decl = re.search(r"\bint\s+cmf_als_cg_last\s*\(([^;]*)\)\s*;", header)
    assert decl is not None and len(decl.group(1).split(",")) == 2 == len(_lib.PROTOTYPES["cmf_als_cg_last"])
    assert '"als_cg_piece"' in header and callable(_lib.Context.als_cg_last)
