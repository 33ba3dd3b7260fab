"""The plain (Frobenius) multiplicative update on the device, sweep by sweep and route by route (cmf_mu_step and the row-blocked
entry points; dense inputs, gemm_arith = 0), against the float64 oracle on float32-rounded inputs.  Cases, yardstick, bound and the
exact family: tests/mu_sweep_cases.py (the derivation of ``tau`` for the association F (B^T B) is in its docstring); that these
checks can fail: tests/test_mu_sweeps_host.py.  EVERY element of every updated factor is compared -- exactly 0 where the yardstick is
exactly 0, within tau relative elsewhere, ``==`` on the exact family; factors outside the mask keep their bytes and the padding rows
and columns of all three stay 0 (read from the padded device images).  No tolerance here is fitted to device output.

a. every sweep at default options;  b. the exact family at default options;  c. every option set that selects another route:
within tau, ``==`` on the exact family, and the launch counts (cmf_mu_route_launches, cmf_data_pass_launches) show that the route
asked for is the one that ran;  d. the row-blocked entry points for world 1, 2, 3, 5 on one context.

Byte equality in (d): V from cmf_mu_v_apply_rows block by block equals V from cmf_mu_v_apply on the same P and G byte for byte at
every k_pad -- no claim had to be replaced.

Measured on an MI355X (printed per case): worst |err| / tau over all sweeps 0.040 at default options (shape A, k = 200, mask 7),
0.043 over the option sets of (c) (gemm_split = 8); the small-Gram sets on shape B 0.009; in (d) P and G within 0.054 of
(L + 16) 2^-24, V within 0.038 and U, Z within 0.007 of their tau.
"""
import numpy as np
import pytest

import mu_sweep_cases as MC
from test_gpu_wmu import _check, _context

pytestmark = pytest.mark.gpu

CASES = [(s, k) for s in sorted(MC.SHAPES) for k in MC.KS]
BITS = ((0, MC.U_BIT), (1, MC.V_BIT), (2, MC.Z_BIT))
DEFAULTS = dict(pair_passes=1, gemm_split=0, small_tile_update=1, fused_mu_update=1, narrow_update=1, small_gram=1,
                small_gram_shares=32, data_pass_wg=15)
SENTINEL = -7.0                       # no product of non-negative inputs


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _set_options(ctx, opts):
    for name, value in dict(DEFAULTS, **opts).items():
        ctx.set_option(name, value)


def _images(ctx, lib):
    """The padded device images of U, V, Z as float32 arrays (rows_pad x k_pad)."""
    mp, dp, pp, kp = ctx.geometry()
    return [ctx.copy_to_host(lib.DeviceArray(ctx, r, kp, _ptr=ctx.factor_dev_ptr(w))) for w, r in enumerate((mp, dp, pp))]


def _reset(ctx, F):
    for w in range(3):
        ctx.set_factor(w, F[w])


def _factors(images, F, before, mask, label):
    """The valid part of the images as float64, after the checks every call owes: padding 0, unmasked factors byte for byte."""
    out = []
    for w, bit in BITS:
        rows, k = F[w].shape
        assert (images[w][rows:] == 0).all() and (images[w][:, k:] == 0).all(), "%s: padding of factor %d is not 0" % (label, w)
        if not mask & bit:
            assert images[w].tobytes() == before[w].tobytes(), "%s: factor %d is outside the mask and changed" % (label, w)
        out.append(images[w][:rows, :k].astype(np.float64))
    return out


def _sweep(ctx, lib, F, l1, l2, mask, label):
    """One cmf_mu_step from the fresh factors F: (U, V, Z) as float64, the launches it added by route form and by data-pass form."""
    _reset(ctx, F)
    before = _images(ctx, lib)
    r0, d0 = ctx.mu_route_launches(), ctx.data_pass_launches()
    ctx.mu_step(l1, l2, mask)
    r1, d1 = ctx.mu_route_launches(), ctx.data_pass_launches()
    got = _factors(_images(ctx, lib), F, before, mask, label)
    return got, {f: r1[f] - r0[f] for f in r1}, tuple(b - a for a, b in zip(d0, d1))


def _check_bounded(got, shape, k, mask, l1, l2, label):
    ref, tols = MC.yardstick(shape, k, mask, l1, l2), MC.tolerances(shape, k, mask)
    return max(_check(got[w], ref[w], tols[w], "%s, factor %d" % (label, w)) for w, bit in BITS if mask & bit)


def _check_exact(got, expected, label):
    assert len(got) == len(expected)
    for w, (g, e) in enumerate(zip(got, expected)):
        bad = g != e
        assert not bad.any(), "%s, array %d: %d elements differ, first at %s" % (label, w, int(bad.sum()), np.argwhere(bad)[0])


# ------------------------------------------------------------------ a. every sweep at default options
@pytest.mark.parametrize("l1, l2", MC.REGS)
@pytest.mark.parametrize("shape, k", CASES)
def test_sweeps_at_default_options(lib, shape, k, l1, l2):
    X, Y, F = MC.bounded(shape, k)
    ctx = _context(lib, X, Y, F, None, None)
    for mask in MC.MASKS:
        label = "%s k=%d l1=%g l2=%g mask %d" % (shape, k, l1, l2, mask)
        got, _, _ = _sweep(ctx, lib, F, l1, l2, mask, label)
        print("%s (k_pad %d): worst |err| / tau = %.4f" % (label, ctx.geometry()[3], _check_bounded(got, shape, k, mask, l1, l2, label)))
    ctx.close()


# ------------------------------------------------------------------ b. the exact family at default options
@pytest.mark.parametrize("owner", MC.OWNERS)
@pytest.mark.parametrize("shape, k", CASES)
def test_exact_family_at_default_options(lib, shape, k, owner):
    X, Y, F, expected, _ = MC.exact(shape, k, owner)
    ctx = _context(lib, X, Y, F, None, None)
    for mask in MC.EXACT_MASKS:
        for reg in MC.EXACT_REGS:
            label = "exact %s k=%d owner %s mask %d l1=l2=%g" % (shape, k, owner, mask, reg[0])
            got, _, _ = _sweep(ctx, lib, F, *reg, mask, label)
            _check_exact(got, expected[mask, reg], label)
    ctx.close()


# ------------------------------------------------------------------ c. routes
OPTION_SETS = [("default", {})] + [("%s=%d" % (n, v), {n: v}) for n, values in (
    ("pair_passes", (0, 2)), ("gemm_split", (1, 3, 8)), ("small_tile_update", (0,)), ("fused_mu_update", (0,)), ("narrow_update", (0, 1)),
    ("small_gram", (0,)), ("small_gram_shares", (1, 3, 1024)), ("data_pass_wg", (0, 3, 15))) for v in values]


def _applies(name, kp, shape):
    """Where an option set selects a route of its own (elsewhere it is the default route again)."""
    name = name.split("=")[0]
    return {"default": True, "gemm_split": True, "fused_mu_update": True, "pair_passes": kp == 128, "small_tile_update": kp in (64, 128),
            "narrow_update": kp == 256, "small_gram": kp in (64, 128) and shape == "B", "small_gram_shares": kp in (64, 128) and shape == "B",
            "data_pass_wg": kp >= 256}[name]


def expected_routes(shape, kp, mask, opts):
    """Launches one cmf_mu_step adds, by form, from k_pad, the option set and the mask alone (a form left out is not determined by
    them: sum_slabs_kernel outside the cases below follows the split heuristics).  The routes, as cmf_api.hip documents them:
      * k_pad 64 / 128 (small_tile_update and fused_mu_update on): every update is factor_update_kernel on 64-row tiles, which also
        sums the unreduced slabs of the data passes -- no sum_slabs launch for them.  At k_pad 128 the two data passes of a half-
        iteration are one gemm_pair_kernel launch (V: X^T U with Y Z; U and Z together: X V with Y^T V) unless pair_passes = 0 or a
        split is forced, and U and Z then share one factor_update2_kernel launch (pair_passes = 2: two factor_update launches).
      * otherwise, k_pad <= 256 with fused_mu_update: gemm_kernel with the EPI_MU epilogue; with the few row tiles of these shapes
        (at most 5 against 256 CUs) narrow_update cuts the 128- and 256-wide tile into 64-wide column tiles, whose image is copied
        over the factor behind the launch.
      * k_pad 512 or fused_mu_update = 0: the product, then mu_apply_kernel.
      * Grams: one of the stacked [U; Z] per V sweep, one of V per call that updates U or Z; the small-Gram kernels at k_pad 64 / 128
        on shape B (1280 rows both), the one-tile TN GEMM elsewhere -- which splits its reduction and sums its slabs with one
        sum_slabs launch unless gemm_split = 1."""
    o = dict(DEFAULTS, **opts)
    v, u, z = bool(mask & MC.V_BIT), bool(mask & MC.U_BIT), bool(mask & MC.Z_BIT)
    updates, grams = v + u + z, v + (u or z)
    e = dict.fromkeys(("epi_mu", "factor_update", "factor_update2", "pair", "gram32", "mu_apply", "narrow_copy"), 0)
    e["gram32"] = grams if o["small_gram"] and kp in (64, 128) and shape == "B" else 0
    small = bool(o["fused_mu_update"] and o["small_tile_update"] and kp in (64, 128))
    if small:
        paired = kp == 128 and o["pair_passes"] != 0 and o["gemm_split"] <= 0
        e["pair"] = (v + (u and z)) if paired else 0
        e["factor_update2"] = int(paired and u and z and o["pair_passes"] == 1)
        e["factor_update"] = updates - 2 * e["factor_update2"]
        e["sum_slabs"] = 0 if o["gemm_split"] == 1 else grams - e["gram32"]
    elif o["fused_mu_update"] and kp <= 256:
        e["epi_mu"] = updates
        e["narrow_copy"] = updates if o["narrow_update"] and kp >= 128 else 0
    else:
        e["mu_apply"] = updates
    if o["gemm_split"] == 1:
        e["sum_slabs"] = 0
    return e


def expected_data_passes(geometry, mask, wg):
    """cmf_data_pass_launches of one step: the passes with a 256-wide factor tile (k_pad >= 256), by form.  gemm() takes an operand
    whose row pitch equals k_pad for a factor-sized one (shape A: Y at k_pad 256, X at k_pad 512): those launches are not data
    passes to it and are not counted."""
    mp, dp, pp, kp = geometry
    passes = ([("tn", dp), ("nn", pp)] if mask & MC.V_BIT else []) + ([("nn", dp)] if mask & MC.U_BIT else []) + ([("tn", pp)] if mask & MC.Z_BIT else [])
    e = [0] * 5
    for form, pitch in passes:
        if kp < 256 or pitch == kp:
            continue
        bit, slot = (1, 1) if form == "tn" else (2, 2)
        e[0 if not wg & bit else (slot + 2 if wg & (bit << 2) else slot)] += 1
    return tuple(e)


@pytest.mark.parametrize("shape, k", CASES)
def test_routes(lib, shape, k):
    families = [("bounded", MC.bounded(shape, k), None)] + [("exact " + o, MC.exact(shape, k, o)[:3], MC.exact(shape, k, o)[3]) for o in MC.OWNERS]
    worst, ran = {}, set()
    for family, (X, Y, F), expected in families:
        ctx = _context(lib, X, Y, F, None, None)
        geometry = ctx.geometry()
        kp = geometry[3]
        for name, opts in OPTION_SETS:
            if not _applies(name, kp, shape):
                continue
            ran.add(name)
            _set_options(ctx, opts)
            wg = dict(DEFAULTS, **opts)["data_pass_wg"]
            runs = [(mask, reg) for mask in MC.MASKS for reg in MC.REGS] if expected is None else list(expected)
            for mask, (l1, l2) in runs:
                label = "%s %s k=%d [%s] mask %d l1=%g l2=%g" % (family, shape, k, name, mask, l1, l2)
                got, routes, passes = _sweep(ctx, lib, F, l1, l2, mask, label)
                want = expected_routes(shape, kp, mask, opts)
                assert {f: routes[f] for f in want} == want, "%s: launches %s" % (label, routes)
                assert passes == expected_data_passes(geometry, mask, wg), label
                if expected is None:
                    worst[name] = max(worst.get(name, 0.0), _check_bounded(got, shape, k, mask, l1, l2, label))
                else:
                    _check_exact(got, expected[mask, (l1, l2)], label)
        ctx.close()
    assert "default" in ran and "gemm_split=8" in ran
    for name in sorted(worst):
        print("%s k=%d (k_pad %d) [%s]: worst |err| / tau = %.4f" % (shape, k, kp, name, worst[name]))


def test_every_option_set_ran_somewhere(lib):
    """The table of option sets against the k_pad each k gives on the device: every set selects a route of its own at some case."""
    seen = set()
    ctx = lib.Context(0)
    for shape, k in CASES:
        ctx.set_problem(*MC.SHAPES[shape], k)
        seen |= {name for name, _ in OPTION_SETS if _applies(name, ctx.geometry()[3], shape)}
    ctx.close()
    assert seen == {name for name, _ in OPTION_SETS}


# ------------------------------------------------------------------ d. the row-blocked entry points
WORLDS = (1, 2, 3, 5)
BLOCKS = {("B", 2): [768, 512], ("B", 3): [512, 512, 256], ("B", 5): [256] * 5, ("A", 3): [256, 256, 0], ("A", 5): [256, 256, 0, 0, 0]}


def _dev(ctx, lib, rows, cols, fill=None):
    a = lib.DeviceArray(ctx, rows, cols)
    if fill is not None:
        ctx.copy_from_host(a, np.full((rows, cols), fill, dtype=np.float32))
    return a


def _check_product(got, ref, L, exact, label):
    """A data product or a Gram summed over L rows: (L + 16) 2^-24 relative per element (gamma_L and single roundings, non-negative
    terms); ``==`` on the exact family."""
    got = got.astype(np.float64)
    if exact:
        assert (got == ref).all(), label
        return 0.0
    return _check(got, ref, (L + 16) * 2.0 ** -24, label)


@pytest.mark.parametrize("shape, k", CASES)
def test_row_blocked_entry_points(lib, shape, k):
    m, d, p = MC.SHAPES[shape]
    families = [("bounded", MC.bounded(shape, k), None, (0.05, 0.1))]
    families += [("exact " + o, MC.exact(shape, k, o)[:3], MC.exact(shape, k, o)[3], (0.0, 0.0)) for o in MC.OWNERS]
    ctx = None
    worst = {"P": 0.0, "G": 0.0, "P by rows": 0.0, "V": 0.0, "U": 0.0, "Z": 0.0}
    for family, (X, Y, F), expected, (l1, l2) in families:
        if ctx is None:
            ctx = _context(lib, X, Y, F, None, None)
        else:
            ctx.set_data(0, X)
            ctx.set_data(1, Y)
        mp, dp, pp, kp = ctx.geometry()
        exact = expected is not None
        U, V, Z = F
        P_ref, G_ref = X.T @ U + Y @ Z, U.T @ U + Z.T @ Z
        for world in WORLDS:
            label = "%s %s k=%d world %d" % (family, shape, k, world)
            _reset(ctx, F)
            fresh = _images(ctx, lib)
            v_before = fresh[1]
            B, n = ctx.mu_blocked_layout(world)
            assert B == 256 * -(-(dp // 256) // world) and n == B * world * kp, label
            v_full = ctx.copy_to_host(lib.DeviceArray(ctx, B * world, kp, _ptr=ctx.factor_dev_ptr(1)))
            assert v_full[:dp].tobytes() == v_before.tobytes() and (v_full[dp:] == 0).all(), label + ": V across grow_v"
            blocks = [(min(r * B, dp), min(min(r * B, dp) + B, dp) - min(r * B, dp)) for r in range(world)]
            assert sum(nr for _, nr in blocks) == dp and [nr for _, nr in blocks] == BLOCKS.get((shape, world), [nr for _, nr in blocks])
            # the partial and the Gram of this shard; a longer buffer keeps its sentinel beyond d_pad
            P, G = _dev(ctx, lib, B * world + 256, kp, SENTINEL), _dev(ctx, lib, kp, kp, SENTINEL)
            ctx.mu_v_partials_split(P.data_ptr(), G.data_ptr())
            Ph, Gh = ctx.copy_to_host(P), ctx.copy_to_host(G)
            assert (Ph[dp:] == SENTINEL).all(), label + ": rows >= d_pad of P were touched"
            assert (Ph[d:dp] == 0).all() and (Ph[:dp, k:] == 0).all() and (Gh[k:] == 0).all() and (Gh[:, k:] == 0).all(), label + ": padding"
            worst["P"] = max(worst["P"], _check_product(Ph[:d, :k], P_ref, m + p, exact, label + ": P"))
            worst["G"] = max(worst["G"], _check_product(Gh[:k, :k], G_ref, m + p, exact, label + ": G"))
            # V from the whole-factor epilogue on the same P and G
            whole = _dev(ctx, lib, dp * kp + kp * kp, 1)
            ctx.copy_from_host(whole, np.concatenate([Ph[:dp].ravel(), Gh.ravel()]))
            ctx.mu_v_apply(whole.data_ptr(), l1, l2)
            v_whole = _images(ctx, lib)[1]
            ctx.set_factor(1, V)
            # rank by rank: the epilogue on the rank's rows, its share of V^T V
            G2 = _dev(ctx, lib, kp, kp)
            shares = []
            for row0, nrows in blocks:
                before = _images(ctx, lib)[1]
                ctx.mu_v_apply_rows(P.data_ptr() + 4 * row0 * kp, G.data_ptr(), row0, nrows, l1, l2)
                after = _images(ctx, lib)[1]
                keep = np.ones(dp, dtype=bool)
                keep[row0:row0 + nrows] = False
                assert after[keep].tobytes() == before[keep].tobytes(), label + ": rows outside the block changed"
                ctx.copy_from_host(G2, np.full((kp, kp), SENTINEL, dtype=np.float32))
                ctx.mu_gram_v_rows(row0, nrows, G2.data_ptr())
                shares.append(ctx.copy_to_host(G2))
                if nrows == 0:
                    assert (shares[-1] == 0).all(), label + ": the Gram of an empty block is not zero-filled"
            images = _images(ctx, lib)
            assert images[1].tobytes() == v_whole.tobytes(), label + ": V by row blocks differs from cmf_mu_v_apply on the same P and G"
            got = _factors(images, F, fresh, MC.V_BIT, label)
            if exact:
                _check_exact([got[1]], [expected[2, (l1, l2)][1]], label + ": V")
                ctx.set_factor(1, V)                 # U and Z of the exact family start from the fresh V (single sweeps)
                shares = []
                for row0, nrows in blocks:
                    ctx.mu_gram_v_rows(row0, nrows, G2.data_ptr())
                    shares.append(ctx.copy_to_host(G2))
            else:
                worst["V"] = max(worst["V"], _check(got[1], MC.yardstick(shape, k, 7, l1, l2)[1], MC.tolerances(shape, k, 7)[1], label + ": V"))
            total = np.zeros((kp, kp), dtype=np.float32)
            for s in shares:
                total += s                           # what the all-reduce does: float32, rank order
            ctx.copy_from_host(G2, total)
            ctx.mu_uz_update_gram(G2.data_ptr(), l1, l2, 5)
            got = _factors(_images(ctx, lib), F, None, 7, label)
            if exact:
                _check_exact([got[0], got[2]], [expected[5, (l1, l2)][0], expected[5, (l1, l2)][2]], label + ": U, Z")
            else:
                ref, tols = MC.yardstick(shape, k, 7, l1, l2), MC.tolerances(shape, k, 7)
                worst["U"] = max(worst["U"], _check(got[0], ref[0], tols[0], label + ": U"))
                worst["Z"] = max(worst["Z"], _check(got[2], ref[2], tols[2], label + ": Z"))
            # the partial block by block, the Gram with the last block only
            _reset(ctx, F)
            Q = _dev(ctx, lib, dp * kp + kp * kp + 1024, 1, SENTINEL)
            live = [(r0, nr) for r0, nr in blocks if nr > 0]
            done = np.zeros(dp, dtype=bool)
            for i, (row0, nrows) in enumerate(live):
                ctx.mu_v_partials_rows(Q.data_ptr(), row0, nrows, i == len(live) - 1)
                Qh = ctx.copy_to_host(Q).ravel()
                done[row0:row0 + nrows] = True
                rows = Qh[:dp * kp].reshape(dp, kp)
                assert (rows[~done] == SENTINEL).all() and (Qh[dp * kp + kp * kp:] == SENTINEL).all(), label + ": partials_rows wrote outside its block"
                assert ((Qh[dp * kp:dp * kp + kp * kp] == SENTINEL).all()) == (i < len(live) - 1), label + ": with_gram"
            worst["P by rows"] = max(worst["P by rows"], _check_product(rows[:d, :k], P_ref, m + p, exact, label + ": P by rows"))
            assert (rows[d:] == 0).all() and (rows[:, k:] == 0).all()
            assert Qh[dp * kp:dp * kp + kp * kp].tobytes() == Gh.tobytes(), label + ": the Gram of partials_rows differs from partials_split's"
            for a in (P, G, whole, G2, Q):
                a.release()
    print("%s k=%d (k_pad %d) row-blocked, worlds %s: worst |err| / bound %s" % (shape, k, kp, WORLDS, {n: "%.4f" % v for n, v in worst.items()}))
    ctx.close()


@pytest.mark.parametrize("shape, k", [("A", 40), ("B", 200)])
def test_row_blocked_refusals_leave_the_context_usable(lib, shape, k):
    X, Y, F = MC.bounded(shape, k)
    ctx = _context(lib, X, Y, F, None, None)
    mp, dp, pp, kp = ctx.geometry()
    B, n = ctx.mu_blocked_layout(2)
    P, G = _dev(ctx, lib, n // kp, kp), _dev(ctx, lib, kp, kp)
    ctx.mu_v_partials_split(P.data_ptr(), G.data_ptr())
    before = [a.tobytes() for a in _images(ctx, lib)]
    bad = [(128, 256), (0, 100), (256, dp), (dp, 256), (-256, 256)]
    for row0, nrows in bad:
        with pytest.raises(ValueError, match="256-aligned"):
            ctx.mu_v_apply_rows(P.data_ptr(), G.data_ptr(), row0, nrows, 0.0, 0.0)
        with pytest.raises(ValueError, match="256-aligned"):
            ctx.mu_gram_v_rows(row0, nrows, G.data_ptr())
        with pytest.raises(ValueError, match="256-aligned"):
            ctx.mu_v_partials_rows(P.data_ptr(), row0, nrows, True)
    for nrows in (0, -256):
        with pytest.raises(ValueError, match="256-aligned"):
            ctx.mu_v_partials_rows(P.data_ptr(), 0, nrows, True)
    with pytest.raises(ValueError, match="256-aligned"):
        ctx.mu_v_apply_rows(P.data_ptr(), G.data_ptr(), 0, -256, 0.0, 0.0)
    for call in (lambda: ctx.mu_v_partials_split(0, G.data_ptr()), lambda: ctx.mu_v_partials_split(P.data_ptr(), 0),
                 lambda: ctx.mu_v_apply_rows(0, G.data_ptr(), 0, 256, 0.0, 0.0), lambda: ctx.mu_v_apply_rows(P.data_ptr(), 0, 0, 256, 0.0, 0.0),
                 lambda: ctx.mu_gram_v_rows(0, 256, 0), lambda: ctx.mu_uz_update_gram(0, 0.0, 0.0, 5), lambda: ctx.mu_v_partials_rows(0, 0, 256, True),
                 lambda: ctx.export_factor_rows(0, 0), lambda: ctx.import_factor_rows(0, 0)):
        with pytest.raises(ValueError, match="null buffer|bad factor argument"):
            call()
    with pytest.raises(ValueError, match="world"):
        ctx.mu_blocked_layout(0)
    assert [a.tobytes() for a in _images(ctx, lib)] == before
    for mask in (7, 2):                              # a correct sweep afterwards
        got, _, _ = _sweep(ctx, lib, F, 0.05, 0.1, mask, "after the refusals")
        _check_bounded(got, shape, k, mask, 0.05, 0.1, "after the refusals, mask %d" % mask)
    ctx.close()


@pytest.mark.parametrize("shape, k", [("A", 7), ("B", 100), ("A", 300)])
def test_export_and_import_round_trip_the_bytes(lib, shape, k):
    X, Y, F = MC.bounded(shape, k)
    ctx = _context(lib, X, Y, F, None, None)
    kp = ctx.geometry()[3]
    ctx.mu_blocked_layout(3)                         # V behind a grown allocation
    ctx.mu_step(0.0, 0.0, 7)                         # factors that are not the uploaded ones
    images = _images(ctx, lib)
    bufs = []
    for w in range(3):
        rows = F[w].shape[0]
        buf = _dev(ctx, lib, rows + 1, kp, SENTINEL)
        ctx.export_factor_rows(w, buf.data_ptr())
        host = ctx.copy_to_host(buf)
        assert host[:rows].tobytes() == images[w][:rows].tobytes() and (host[rows:] == SENTINEL).all()
        bufs.append(buf)
    _reset(ctx, [f[::-1] + 1.0 for f in F])
    for w in range(3):
        ctx.import_factor_rows(w, bufs[w].data_ptr())
    assert [a.tobytes() for a in _images(ctx, lib)] == [a.tobytes() for a in images]
    ctx.close()
