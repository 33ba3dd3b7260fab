"""The k_pad = 256 data passes on the 256-thread workgroup (cmf_gemm_wg256.hip.h: four waves, 128 x 128 wave tiles, the TN form's X
fed to the MFMAs from registers) against the 512-thread gemm_kernel they stand in for.  Both consume the reduction in the same
order element by element -- TN group s takes k = 2 s + lh, NN group 4 q + e takes k = 8 q + 4 lh + e, split-K slabs are cut at
the same places -- so option data_pass_wg must not change a single bit of any result.  Equality alone would compare the library
with itself: the new kernels' MU step is also held against the float64 oracle (cmf_solvers.py:230-263)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 256


@pytest.fixture(scope="module")
def lib():
    from pycmf_amd import _lib
    if _lib.device_count() < 1:
        pytest.fail("no GPU visible: the gpu-marked tests need an MI355X")
    return _lib


def _signed(seed, m, d, p):
    rng = np.random.RandomState(seed)
    return (rng.randn(m, d), rng.randn(d, p), rng.randn(m, K), rng.randn(d, K), rng.randn(p, K))


def _context(lib, wg, split, X, Y, U, V, Z):
    ctx = lib.Context(0)
    ctx.set_option("data_pass_wg", wg)
    if split is not None:
        ctx.set_option("gemm_split", split)
    ctx.set_problem(X.shape[0], X.shape[1], Y.shape[1], K)
    ctx.set_data(0, X); ctx.set_data(1, Y)
    for w, F in enumerate((U, V, Z)):
        ctx.set_factor(w, F)
    return ctx


def _v_partials(lib, wg, split, prob):
    """[X^T U + Y Z | Gram] of cmf_mu_v_partials, copied to the host: the TN pass, the NN pass accumulated onto it."""
    import torch
    ctx = _context(lib, wg, split, *prob)
    buf = torch.zeros(ctx.v_buf_elems(), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()   # the fill runs on PyTorch's stream, the context launches on its own
    ctx.mu_v_partials(buf.data_ptr())
    ctx.sync()
    out = buf.cpu().numpy()
    ctx.close()
    return out


# m, d, p, gemm_split (None: the heuristic).  X^T U reduces over m_pad, Y Z over p_pad; d_pad / 256 row tiles on both passes.
CASES = [
    pytest.param(512, 768, 256, 1, id="unsplit-16-and-8-ksteps-3-row-tiles-accumulate"),
    pytest.param(512, 768, 256, None, id="default-split-3-tiles-take-slabs"),
    pytest.param(256, 256, 256, 8, id="slabs-of-1-kstep"),
    pytest.param(256, 256, 256, 4, id="slabs-of-2-ksteps"),
    pytest.param(256, 256, 256, 3, id="slabs-of-3-3-2-ksteps"),
    pytest.param(300, 260, 700, 1, id="ragged-zero-padding"),
]


@pytest.mark.parametrize("m,d,p,split", CASES)
def test_v_partials_bit_identical(lib, m, d, p, split):
    prob = _signed(m + d + p, m, d, p)
    old = _v_partials(lib, 0, split, prob)
    new = _v_partials(lib, 3, split, prob)
    X, Y, U, V, Z = prob
    d_pad = -(-d // 256) * 256
    ref = np.zeros((d_pad, K))
    ref[:d] = X.T @ U + Y @ Z
    got = new[:d_pad * K].reshape(d_pad, K)
    err = np.abs(got - ref).max()
    print("m,d,p=%d,%d,%d split=%s: %d of %d floats differ; max |new - float64| = %.3e (scale %.1f)"
          % (m, d, p, split, int((old != new).sum()), old.size, err, np.abs(ref).max()))
    assert np.isfinite(new).all() and np.abs(new).max() > 0
    assert np.array_equal(old, new)
    # not the subject (the bits are), but equality of two wrong buffers must not pass.  An entry sums n <= 512 + 768 products of
    # N(0, 1) pairs in float32: the worst-case bound n eps sum |x u| = 1280 * 6e-8 * (1280 * 2 / pi) is 0.06 (0.01 at n = 512), the largest of the
    # 65536 or more entries is about 4 sqrt(n) (143; 90 at n = 512), so 1e-3 of it lies above every possible rounding and far below a misplaced or dropped k-pair (~1)
    assert err <= 1e-3 * np.abs(ref).max()


def test_mu_steps_bit_identical_and_match_oracle(lib):
    """Two full MU iterations (all four data passes: X^T U, Y Z, X V, Y^T V) at 512, 768, 256."""
    from oracle import cmf_oracle as O
    rng = np.random.RandomState(5)
    m, d, p = 512, 768, 256
    X, Y = np.abs(rng.randn(m, d)), np.abs(rng.randn(d, p))
    s = np.sqrt(X.mean() / K)
    U0, V0, Z0 = s * np.abs(rng.randn(m, K)), s * np.abs(rng.randn(d, K)), s * np.abs(rng.randn(p, K))
    out = {}
    for wg in (0, 3):
        ctx = _context(lib, wg, None, X, Y, U0, V0, Z0)
        for _ in range(2):
            ctx.mu_step(0.01, 0.02, 7)
        out[wg] = [ctx.get_factor(w) for w in range(3)]
        ctx.close()
    Ur, Vr, Zr = U0.copy(), V0.copy(), Z0.copy()
    for _ in range(2):
        O.mu_update_step(X, Y, Ur, Vr, Zr, 0.01, 0.02)
    for name, a, b, r in zip("UVZ", out[3], out[0], (Ur, Vr, Zr)):
        print("%s: %d entries differ between the kernels; max rel. distance to the oracle %.3e"
              % (name, int((a != b).sum()), np.abs(a / r - 1).max()))
        assert np.array_equal(a, b)
        np.testing.assert_allclose(a, r, rtol=2e-4, atol=1e-6)   # tests/test_gpu_mu.py, test_mu_vs_oracle_ragged
