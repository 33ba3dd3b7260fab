"""The one dispatcher behind the six ALS step entry points (als_step, csrc/cmf_als_steps.hip.h): entry points whose arguments name
the same routes write the same BYTES, an option of one step does not reach the next, and a refusal carries the name of the entry
point that was called.  The problem is als_dual_cases.py (row lengths on both sides of every class edge, two observed sides) at
k = 40 and 200 (k_pad 64 and 256) under als_piece = 32 and als_cg_piece = 16: rows of several pieces and long CG rows occur.  The
background context puts a weight of 0.25 on X AND on Y, so that no sweep is eligible for the dual rows (under one on X alone the Z
sweep, which reads Y alone, still is); a background weight needs every stored weight at or above it: that context binds max(w, 0.25)."""
import numpy as np
import pytest

import als_dual_cases as C
from test_gpu_als import _bind

pytestmark = pytest.mark.gpu

L2 = C.L2
KS = [40, 200]
BG = 0.25


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _ctx(lib, k, kind=""):
    """kind: '' both relations observed | 'bg' a background weight on both | 'bias' x biases bound | 'logit' Y logistic."""
    X, Y, Wx, Wy, F = C.problem(k)
    ctx = lib.Context(0)
    ctx.set_option("als_piece", 32)
    ctx.set_option("als_cg_piece", 16)
    ctx.set_problem(C.M, C.D, C.P, k)
    if kind == "bg":
        Wx, Wy = Wx.copy(), Wy.copy()
        Wx.data, Wy.data = np.maximum(Wx.data, BG), np.maximum(Wy.data, BG)
    _bind(ctx, 0, X, Wx)
    _bind(ctx, 1, (Y > 0).astype(np.float64) if kind == "logit" else Y, Wy)
    if kind == "bg":
        ctx.set_background_weight(0, BG)
        ctx.set_background_weight(1, BG)
    if kind == "bias":
        ctx.set_biases(0, True, 0.125, 0.5)
    if kind == "logit":
        ctx.set_relation_loss(1, "logistic")
    return ctx, F


def _after(ctx, F, call):
    """The float32 bytes of U, V and Z after one call from the start F."""
    for w in range(3):
        ctx.set_factor(w, F[w])
    call(ctx)
    return b"".join(ctx.get_factor(w).astype(np.float32).tobytes() for w in range(3))


def _pairs(kind):
    """(what, first call, second call): the table of equivalent entry points."""
    out = []
    if kind == "":
        for nn in (0, 5, 7):
            for m in (7, 1):
                out.append(("dual(0, s = 2) = nnls(2), nn %d mask %d" % (nn, m),
                            lambda c, nn=nn, m=m: c.als_dual_step(L2, nn, m, 0, 2, 0), lambda c, nn=nn, m=m: c.als_nnls_step(L2, nn, m, 2)))
                out.append(("dual(0) = als_step, nn %d mask %d" % (nn, m),
                            lambda c, nn=nn, m=m: c.als_dual_step(L2, nn, m, 0, 0, 0), lambda c, nn=nn, m=m: c.als_step(L2, nn, m)))
        for s in (0, 2):
            out.append(("nncg(c = 3, n = 3, s = %d) = cg(3, %d), nn 0" % (s, s),
                        lambda c, s=s: c.als_nncg_step(L2, 0, 7, 3, 3, s), lambda c, s=s: c.als_cg_step(L2, 0, 7, 3, s)))
        for nn in (0, 5):
            for s in (0, 2):
                out.append(("bias(c = 3, s = %d), no biases = cg(3, %d), nn %d" % (s, s, nn),
                            lambda c, nn=nn, s=s: c.als_bias_step(L2, nn, 7, 3, s), lambda c, nn=nn, s=s: c.als_cg_step(L2, nn, 7, 3, s)))
            out.append(("bias(c = 0, s = 2), no biases = nnls(2), nn %d" % nn,
                        lambda c, nn=nn: c.als_bias_step(L2, nn, 7, 0, 2), lambda c, nn=nn: c.als_nnls_step(L2, nn, 7, 2)))
            out.append(("bias(c = 0, s = 0), no biases = als_step, nn %d" % nn,
                        lambda c, nn=nn: c.als_bias_step(L2, nn, 7, 0, 0), lambda c, nn=nn: c.als_step(L2, nn, 7)))
    if kind == "bg":                                         # a background weight on X and on Y: no sweep is eligible
        for nn in (0, 5, 7):
            for s in (0, 2):
                out.append(("dual(128, s = %d, n = 3) = nncg(0, 3, %d), nn %d" % (s, s, nn),
                            lambda c, nn=nn, s=s: c.als_dual_step(L2, nn, 7, 128, s, 3), lambda c, nn=nn, s=s: c.als_nncg_step(L2, nn, 7, 0, 3, s)))
    return out


@pytest.mark.parametrize("kind", ["", "bg"])
@pytest.mark.parametrize("k", KS)
def test_entry_points_that_name_the_same_routes_write_the_same_bytes(lib, k, kind):
    ctx, F = _ctx(lib, k, kind)
    start = _after(ctx, F, lambda c: None)
    for what, first, second in _pairs(kind):
        a, b = _after(ctx, F, first), _after(ctx, F, second)
        assert a == b, (k, what)
        assert a != start, (k, what)                         # (the step did sweep)
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_the_dual_permission_does_not_outlive_its_step(lib, k):
    """After als_dual_step(dual_max = 128) a plain als_step from the same start writes the bytes of an als_step on a fresh context,
    and does not touch the counters of the dual sweep."""
    fresh, F = _ctx(lib, k)
    want = _after(fresh, F, lambda c: c.als_step(L2, 0, 7))
    assert fresh.als_dual_last() == (0, 0, 0, 0, 0)
    fresh.close()
    ctx, F = _ctx(lib, k)
    dual = _after(ctx, F, lambda c: c.als_dual_step(L2, 0, 7, 128))
    last = ctx.als_dual_last()
    assert sum(last[:3]) > 0 and dual != want                # rows did go dual: other bits than the formed rows'
    assert _after(ctx, F, lambda c: c.als_step(L2, 0, 7)) == want
    assert ctx.als_dual_last() == last
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_refusals_name_the_entry_point_called_and_leave_the_context_usable(lib, k):
    for kind, exc, match, refused in (
            ("bias", NotImplementedError, r"^libcmfhip: cmf_als_dual_step: nn_cg_steps with biases", lambda c: c.als_dual_step(L2, 5, 7, 128, 0, 3)),
            ("logit", NotImplementedError, r"^libcmfhip: cmf_als_nncg_step: Y has a logistic loss", lambda c: c.als_nncg_step(L2, 7, 7, 0, 3, 0)),
            ("logit", NotImplementedError, r"^libcmfhip: cmf_als_dual_step: Y has a logistic loss", lambda c: c.als_dual_step(L2, 7, 7, 128, 0, 3))):
        fresh, F = _ctx(lib, k, kind)
        want = _after(fresh, F, lambda c: c.als_step(L2, 0, 7))
        fresh.close()
        ctx, F = _ctx(lib, k, kind)
        for w in range(3):
            ctx.set_factor(w, F[w])
        with pytest.raises(exc, match=match):
            refused(ctx)
        assert all((ctx.get_factor(w) == F[w]).all() for w in range(3))      # a refused step sweeps nothing
        assert _after(ctx, F, lambda c: c.als_step(L2, 0, 7)) == want, (k, kind)
        ctx.close()
