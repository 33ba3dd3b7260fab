"""The k_pad = 256 data passes with the factor in a register ring (cmf_gemm_wg256.hip.h, FREG; option data_pass_wg bits 2 and 3):
the TN form without LDS or barrier, the NN form with X alone in LDS.  They consume the reduction in the order of gemm_kernel and of
the LDS forms (TN group s: k = 2 s + lh; NN group 4 q + e: k = 8 q + 4 lh + e; same split-K cuts), so no value of the option may
change a bit.  Equality alone would compare the library with itself: every case is also held against float64, and the per-context
launch counts (cmf_data_pass_launches) must show that the form asked for is the one that ran.

The library takes a product for a data pass when the leading dimension of its data operand differs from k_pad (cmf_api.hip, gemm():
X's is d_pad, Y's is p_pad); an operand as wide as the factor goes to the factor-side symbol of gemm_kernel whatever the option says
and is not counted.  So at 256, 256, 256 with 256 components neither pass reaches the kernels under test, and at 512, 768, 256 only
the passes over X do: the cases with 512 components or p_pad = 512 repeat those shapes where both passes reach them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEW = (7, 11, 15)   # every combination of the new bits on top of 3


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _pad(n):
    return -(-n // 256) * 256


def _launches(wg, passes, k):
    """data_pass_launches() after `passes` = [(form, columns of the data operand)], form "tn" or "nn", under data_pass_wg = wg."""
    tn = 0 if not wg & 1 else (3 if wg & 4 else 1)
    nn = 0 if not wg & 2 else (4 if wg & 8 else 2)
    want = [0] * 5
    for form, cols in passes:
        if _pad(cols) != _pad(k):   # else: not a data pass to the library
            want[tn if form == "tn" else nn] += 1
    return tuple(want)


def _context(lib, wg, split, k, X, Y, U, V, Z):
    ctx = lib.Context(0)
    ctx.set_option("data_pass_wg", wg)
    if split is not None:
        ctx.set_option("gemm_split", split)
    ctx.set_problem(X.shape[0], X.shape[1], Y.shape[1], k)
    ctx.set_data(0, X); ctx.set_data(1, Y)
    for w, F in enumerate((U, V, Z)):
        ctx.set_factor(w, F)
    return ctx


def _v_partials(lib, wg, split, k, prob):
    """[X^T U + Y Z | Gram] of cmf_mu_v_partials, copied to the host (the TN pass, the NN pass accumulated onto it), and the
    launch counts of the context that computed it."""
    import torch
    ctx = _context(lib, wg, split, k, *prob)
    buf = torch.zeros(ctx.v_buf_elems(), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()   # the fill runs on PyTorch's stream, the context launches on its own
    assert ctx.data_pass_launches() == (0, 0, 0, 0, 0)
    ctx.mu_v_partials(buf.data_ptr())
    ctx.sync()
    out, launches = buf.cpu().numpy(), ctx.data_pass_launches()
    ctx.close()
    return out, launches


# m, d, p, k, gemm_split (None: the heuristic).  X^T U reduces over m_pad, Y Z over p_pad; d_pad / 256 row tiles on both passes.
CASES = [
    pytest.param(512, 768, 256, 256, 1, id="unsplit-16-and-8-ksteps-3-row-tiles-accumulate"),
    pytest.param(512, 768, 256, 256, None, id="default-split-3-tiles-take-slabs"),
    pytest.param(256, 256, 256, 256, 8, id="slabs-of-1-kstep-every-refill-clamped"),
    pytest.param(256, 256, 256, 256, 3, id="slabs-of-3-3-2-ksteps"),
    pytest.param(256, 256, 256, 512, 1, id="two-column-tiles-ring-base-carries-n0"),
    pytest.param(256, 256, 256, 512, 8, id="two-column-tiles-slabs-of-1-kstep-every-refill-clamped"),
    pytest.param(256, 256, 256, 512, 3, id="two-column-tiles-slabs-of-3-3-2-ksteps"),
    pytest.param(300, 260, 700, 256, 1, id="ragged-zero-padding"),
]


@pytest.mark.parametrize("m,d,p,k,split", CASES)
def test_v_partials_bit_identical(lib, m, d, p, k, split):
    rng = np.random.RandomState(m + d + p + k)
    prob = (rng.randn(m, d), rng.randn(d, p), rng.randn(m, k), rng.randn(d, k), rng.randn(p, k))
    X, Y, U, V, Z = prob
    d_pad = _pad(d)
    ref = np.zeros((d_pad, k))
    ref[:d] = X.T @ U + Y @ Z
    out = {}
    for wg in (0, 3) + NEW:
        out[wg], launches = _v_partials(lib, wg, split, k, prob)
        assert launches == _launches(wg, [("tn", d), ("nn", p)], k), "data_pass_wg=%d launched %s" % (wg, launches)
    for wg in NEW:
        got = out[wg][:d_pad * k].reshape(d_pad, k)
        err = np.abs(got - ref).max()
        print("m,d,p,k=%d,%d,%d,%d split=%s wg=%d: %d / %d of %d floats differ from 0 / 3; max |new - float64| = %.3e (scale %.1f)"
              % (m, d, p, k, split, wg, int((out[0] != out[wg]).sum()), int((out[3] != out[wg]).sum()), out[wg].size, err, np.abs(ref).max()))
        assert np.isfinite(out[wg]).all() and np.abs(out[wg]).max() > 0
        assert np.array_equal(out[0], out[wg])
        assert np.array_equal(out[3], out[wg])
        # the bound of test_gpu_data_pass_wg.py, derived there: an entry sums n <= 1280 products of N(0, 1) pairs in float32, worst-case
        # rounding 0.06 against a largest entry of about 4 sqrt(n); 1e-3 of it lies above every rounding and far below a misplaced k-pair
        assert err <= 1e-3 * np.abs(ref).max()


@pytest.mark.parametrize("p", [pytest.param(256, id="passes-over-x"), pytest.param(512, id="passes-over-x-and-y")])
def test_mu_steps_bit_identical_and_match_oracle(lib, p):
    """Two full MU iterations (X^T U, Y Z, X V, Y^T V) at 512, 768, p: the library's default and every new combination against
    data_pass_wg = 0, and against the float64 oracle.  With p = 256 the two products over Y are no data passes to the library
    (the module's docstring); with p = 512 all four are."""
    from oracle import cmf_oracle as O
    rng = np.random.RandomState(5)
    m, d, k = 512, 768, 256
    X, Y = np.abs(rng.randn(m, d)), np.abs(rng.randn(d, p))
    s = np.sqrt(X.mean() / k)
    U0, V0, Z0 = s * np.abs(rng.randn(m, k)), s * np.abs(rng.randn(d, k)), s * np.abs(rng.randn(p, k))
    passes = 2 * [("tn", d), ("nn", p), ("nn", d), ("tn", p)]
    out, launches = {}, {}
    for wg in (0, None) + NEW:
        ctx = lib.Context(0)
        if wg is not None:
            ctx.set_option("data_pass_wg", wg)
        ctx.set_problem(m, d, p, k)
        ctx.set_data(0, X); ctx.set_data(1, Y)
        for w, F in enumerate((U0, V0, Z0)):
            ctx.set_factor(w, F)
        for _ in range(2):
            ctx.mu_step(0.01, 0.02, 7)
        out[wg] = [ctx.get_factor(w) for w in range(3)]
        launches[wg] = ctx.data_pass_launches()
        ctx.close()
    for wg in (0,) + NEW:
        assert launches[wg] == _launches(wg, passes, k), "data_pass_wg=%d launched %s" % (wg, launches[wg])
    # the default: every data pass on the 256-thread workgroup, in whichever of its forms
    assert launches[None][0] == 0 and sum(launches[None]) == sum(launches[0]) > 0
    Ur, Vr, Zr = U0.copy(), V0.copy(), Z0.copy()
    for _ in range(2):
        O.mu_update_step(X, Y, Ur, Vr, Zr, 0.01, 0.02)
    for wg in (None,) + NEW:
        for name, a, b, r in zip("UVZ", out[wg], out[0], (Ur, Vr, Zr)):
            print("wg=%s %s: %d entries differ from data_pass_wg=0; max rel. distance to the oracle %.3e"
                  % (wg, name, int((a != b).sum()), np.abs(a / r - 1).max()))
            assert np.array_equal(a, b)
            np.testing.assert_allclose(a, r, rtol=2e-4, atol=1e-6)   # tests/test_gpu_mu.py, test_mu_vs_oracle_ragged
