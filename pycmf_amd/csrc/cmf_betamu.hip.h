// cmf_betamu.hip.h -- multiplicative updates for the beta-divergence objective  D_beta(X || U V^T) + D_beta(Y || V Z^T),  0 <= beta <= 2
// (beta = 0 Itakura-Saito, 1 Kullback-Leibler, 2 Frobenius; sklearn's NMF(solver="mu", beta_loss=...) per block of the collective model).
//
//   S = A B^T,  P = max(S, EPS)^(beta - 2)                       EPS = 2^-23
//   num = (T .* P) B        den = (S .* P) B        F <- F .* (num / reg(den, F))^gamma
//   gamma = 1 / (2 - beta) for beta < 1,  1 for 1 <= beta <= 2      reg(den, F) = den + l1 + l2 F, then 0 -> EPS
//
// Both products need the same S tile, so they come from ONE pass: the dual-output form of cmf_pairpass.hip.h (OUTPUTS = 2) keeps two
// accumulator sets and feeds every LDS fragment of step 3 to two MFMAs -- 6 m d k flops per sweep instead of the 8 m d k of two
// single-output passes, and one power per element of S instead of two.
//   BetaIS    beta = 0:  r = rcp(max(s, EPS)); p = r r; n = t p; d = s p.  No transcendental.
//   BetaGen   any beta:  p = exp2((beta - 2) log2(max(s, EPS))); n = t p; d = s p.
//   BetaNum<IS> / BetaDen<IS>   the single-output twins (numerator only; denominator only, no image; p in the literal form of
//             BetaIS or of BetaGen): the route of a width whose dual kernel does not ship (BETA_DUAL_KP below), and the other side of
//             the timing tool's comparison.
//   BetaDivIS / BetaDivGen   reductions: d_beta(t | max(s, EPS)) per valid element, terms in float32, float64 accumulation.
// den uses the UNCLAMPED s: a padded or all-zero owned row gives d = 0 p = 0 exactly, the padding rule of the pass; t = 0 gives
// n = 0 p = 0.  p stays finite: at most EPS^-2 = 2^46.
// log2 and exp2 are the RAW hardware instructions, __builtin_amdgcn_logf (v_log_f32) and __builtin_amdgcn_exp2f (v_exp_f32), not the
// device library's wrappers: the CDNA instruction set reference documents both with 1 ULP accuracy and denormals flushed.  Their
// argument here is never denormal (max(s, EPS) >= 2^-23; a quotient of float32 normals); a result below 2^-126 comes out as 0,
// which is finite.  The tolerances of tests/beta_yardstick.py rest on that 1 ULP.
// The update is pairpass_update_kernel<DEN_SLABS, POW>; a V sweep keeps the slabs of its X and Y passes apart and the update sums
// them in slab order, numerator and denominator alike.  No atomics: a repeated step is bit-identical.
//
// Reference counterpart: none -- pycmf/cmf.py:299-304 documents beta_loss and cmf_solvers.py:249 leaves gamma as a TODO.
#pragma once
#include "cmf_pairpass.hip.h"

namespace cmfk {

struct BetaIS { // img0 = T
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static constexpr bool ADDS = false;
    static constexpr int OUTPUTS = 2;
    static __device__ __forceinline__ void map2(float s, float t, float, float *n, float *d) {
        const float r = __builtin_amdgcn_rcpf(fmaxf(s, CMF_MU_EPS));
        const float p = r * r;
        *n = t * p;
        *d = s * p;
    }
};
// max(s, EPS)^e
static __device__ __forceinline__ float beta_pow(float s, float e) { return __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(fmaxf(s, CMF_MU_EPS))); }
struct BetaGen { // img0 = T, param = beta
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static constexpr bool ADDS = false;
    static constexpr int OUTPUTS = 2;
    static __device__ __forceinline__ void map2(float s, float t, float beta, float *n, float *d) {
        const float p = beta_pow(s, beta - 2.f);
        *n = t * p;
        *d = s * p;
    }
};
// the single-output twins; IS: p in BetaIS's literal form (beta = 0), otherwise in BetaGen's
template <bool IS>
static __device__ __forceinline__ float beta_p(float s, float beta) {
    if constexpr (IS) {
        const float r = __builtin_amdgcn_rcpf(fmaxf(s, CMF_MU_EPS));
        return r * r;
    } else
        return beta_pow(s, beta - 2.f);
}
template <bool IS>
struct BetaNum { // img0 = T, param = beta
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static constexpr bool ADDS = false;
    static constexpr bool PARAM = true;
    static __device__ __forceinline__ float map(float s, float t, float beta) {
        const float p = beta_p<IS>(s, beta);
        return t * p;
    }
};
template <bool IS>
struct BetaDen { // param = beta
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 0;
    static constexpr bool ADDS = false;
    static constexpr bool PARAM = true;
    static __device__ __forceinline__ float map(float s, float, float beta) {
        const float p = beta_p<IS>(s, beta);
        return s * p;
    }
};
struct BetaDivIS { // img0 = T:  t / s - log(t / s) - 1  (t > 0: the callers refuse zeros in the data at beta = 0)
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static constexpr bool PARAM = true;
    static __device__ __forceinline__ double term(float s, float t, float) {
        const float q = t / fmaxf(s, CMF_MU_EPS);
        float e = q - logf(q);
        e = e - 1.f;
        return (double)e;
    }
};
struct BetaDivGen { // img0 = T, param = beta (not 0, not 1):  (t^beta + (beta - 1) s^beta - beta t s^(beta - 1)) / (beta (beta - 1));  t = 0: s^beta / beta
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static constexpr bool PARAM = true;
    static __device__ __forceinline__ double term(float s, float t, float beta) {
        const float sc = fmaxf(s, CMF_MU_EPS);
        const float pw = beta_pow(sc, beta - 1.f);
        const float sb = sc * pw;
        if (!(t > 0.f)) return (double)(sb / beta);
        const float tb = __builtin_amdgcn_exp2f(beta * __builtin_amdgcn_logf(t));
        const float cross = t * pw;
        float e = tb + (beta - 1.f) * sb;
        e = e - beta * cross;
        return (double)(e / (beta * (beta - 1.f)));
    }
};

// The widths whose DUAL kernel ships.  Every width of with_kp was compiled for gfx950 and its resource usage read from the
// compiler (DESIGN section 21 has the table).  KP = 256 needs 128 registers of the owned row and 2 x 128 accumulators beside the
// staging and image registers: the compiler fills all 256 VGPRs and 256 AGPRs and still spills 188 (as stored) to 411 (transposed)
// registers to scratch, so that width does not ship the dual kernel and runs the twins (8 m d k).
constexpr int BETA_DUAL_KP = 32 | 64 | 128;

// slab 0 <- the sum of the nslab slabs in slab order (what the update kernel forms in registers)
__global__ void beta_sum_slabs_kernel(float *slabs, int nslab, int64_t stride, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = reinterpret_cast<const f32x4 *>(slabs)[i];
        for (int s = 1; s < nslab; ++s) v += reinterpret_cast<const f32x4 *>(slabs + (int64_t)s * stride)[i];
        reinterpret_cast<f32x4 *>(slabs)[i] = v;
    }
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx, after cmf_klmu.hip.h)
#ifdef CMF_BETAMU_HOST

static double beta_gamma(double beta) { return beta < 1.0 ? 1.0 / (2.0 - beta) : 1.0; }

// option "beta_route": 0 the shipped choice | 1 the dual pass (where it is built) | 2 the two single-output twins
static bool beta_dual(const cmf_ctx *c) { return c->opt_beta_route != 2 && (BETA_DUAL_KP & c->kp) != 0; }

// the share rule of the KL passes (option "kl_split" forces the count here too)
static int64_t beta_sweep_slabs(const cmf_ctx *c, int f) {
    int64_t S, S2 = 0, per;
    if (f == CMF_V) { kl_plan(c, PP_VX, &S, &per); kl_plan(c, PP_VY, &S2, &per); }
    else kl_plan(c, f == CMF_U ? PP_U : PP_Z, &S, &per);
    return S + S2;
}
// scratch of a step: numerator and denominator slabs of the widest sweep -- twice the KL step's slabs
static size_t beta_slab_bytes(const cmf_ctx *c, int mask) {
    size_t need = 0;
    const int bits[3] = {CMF_UPD_U, CMF_UPD_V, CMF_UPD_Z};
    for (int f = 0; f < 3; ++f)
        if (mask & bits[f]) need = std::max(need, (size_t)2 * beta_sweep_slabs(c, f) * c->frows_pad[f] * c->kp * sizeof(float));
    return need;
}

static int beta_check(cmf_ctx *c, const char *what, double beta) {
    if (!(beta >= 0.0 && beta <= 2.0)) return fail(CMF_EINVAL, "%s: beta must lie in [0, 2], got %g", what, beta);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: k_pad = %d (n_components above 256) is not supported by the beta-divergence passes", what, c->kp);
    return CMF_OK;
}
// a relation can take part: its dense image, and nothing bound on it that these passes would ignore
static int beta_side_ok(cmf_ctx *c, const char *what, int which) {
    const char *nm = which == 0 ? "X" : "Y";
    if (!have_data(c, which)) return fail(CMF_EINVAL, "%s: %s has not been set", what, nm);
    if (kl_native(c, which))
        return fail(CMF_EUNSUPPORTED, "%s: %s is held as native CSR only; the beta-divergence passes read the dense image (sparse_mode 1)", what, nm);
    if (c->wm_bg[which] > 0.0)
        return fail(CMF_EUNSUPPORTED, "%s: %s has a background weight bound, which only the ALS steps honour; clear it with cmf_set_background_weight(ctx, %d, 0)",
                    what, nm, which);
    if (c->als_bias[which].on)
        return fail(CMF_EUNSUPPORTED, "%s: %s has biases bound, which only cmf_als_bias_step honours; clear them with cmf_set_biases(ctx, %d, 0, 0, 0)", what, nm, which);
    if (c->wm_kind[which] != 0)
        return fail(CMF_EUNSUPPORTED, "%s: %s has entry weights bound, which the beta-divergence passes do not honour; clear them with cmf_clear_weight(ctx, %d)",
                    what, nm, which);
    return CMF_OK;
}
static int beta_sides_ok(cmf_ctx *c, const char *what, int mask) {
    if (mask & (CMF_UPD_U | CMF_UPD_V)) CHK(beta_side_ok(c, what, 0));
    if (mask & (CMF_UPD_Z | CMF_UPD_V)) CHK(beta_side_ok(c, what, 1));
    return CMF_OK;
}

// the dual kernel of the widths that ship it
template <class P>
static int beta_launch_dual(cmf_ctx *c, const PairPass &ps, const PairPassArgs &a, int64_t S) {
    const dim3 grid = pp_grid(c, ps, S);
    with_kp(c->kp, [&](auto kp) {
        constexpr int KP = decltype(kp)::value;
        if constexpr ((BETA_DUAL_KP & KP) != 0) {
            if (ps.trans) hipLaunchKernelGGL((pairpass_kernel<KP, 1, P>), grid, dim3(256), 0, c->stream, a);
            else hipLaunchKernelGGL((pairpass_kernel<KP, 0, P>), grid, dim3(256), 0, c->stream, a);
        }
    });
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// numerator and denominator slabs of one pass (slab stride = rows_pad * k_pad); *nslab = how many of each it wrote
static int beta_pass(cmf_ctx *c, const PairPass &ps, double beta, float *num, float *den, int *nslab) {
    int64_t S, per;
    kl_plan(c, ps, &S, &per);
    PairPassArgs a = pp_args(c, ps, per);
    a.img0 = ps.which == 0 ? c->X : c->Y;
    a.param = (float)beta;
    const double cells = (double)c->frows[ps.fa] * (double)c->frows[ps.fb];
    if (beta_dual(c)) {
        a.out = num;
        a.out2 = den;
        Timed tm(c, CMF_K_KLMU, 6.0 * cells * (double)c->k);
        if (beta == 0.0) CHK(beta_launch_dual<BetaIS>(c, ps, a, S));
        else CHK(beta_launch_dual<BetaGen>(c, ps, a, S));
    } else {
        {
            a.out = num;
            Timed tm(c, CMF_K_KLMU, 4.0 * cells * (double)c->k);
            if (beta == 0.0) CHK(pp_launch_pass<BetaNum<true>>(c, ps, a, S));
            else CHK(pp_launch_pass<BetaNum<false>>(c, ps, a, S));
        }
        {
            a.out = den;
            Timed tm(c, CMF_K_KLMU, 4.0 * cells * (double)c->k);
            if (beta == 0.0) CHK(pp_launch_pass<BetaDen<true>>(c, ps, a, S));
            else CHK(pp_launch_pass<BetaDen<false>>(c, ps, a, S));
        }
    }
    *nslab = (int)S;
    return CMF_OK;
}

// the passes of the sweep of factor f: numerator slabs from `base`, denominator slabs behind them; *nslab = slabs of each
static int beta_sweep_passes(cmf_ctx *c, int f, double beta, float *base, float **num, float **den, int *nslab) {
    const int64_t stride = c->frows_pad[f] * c->kp;
    *num = base;
    *den = base + beta_sweep_slabs(c, f) * stride;
    int n1 = 0, n2 = 0;
    if (f == CMF_V) {
        CHK(beta_pass(c, PP_VX, beta, *num, *den, &n1));
        CHK(beta_pass(c, PP_VY, beta, *num + (int64_t)n1 * stride, *den + (int64_t)n1 * stride, &n2));
    } else
        CHK(beta_pass(c, f == CMF_U ? PP_U : PP_Z, beta, *num, *den, &n1));
    *nslab = n1 + n2;
    return CMF_OK;
}

extern "C" int cmf_mu_beta_step(cmf_ctx *c, double beta, double l1, double l2, int mask) {
    NEED_PROBLEM(c);
    CHK(beta_check(c, "cmf_mu_beta_step", beta));
    CHK(beta_sides_ok(c, "cmf_mu_beta_step", mask));
    DeviceGuard dg(c->device);
    CHK(ensure_scratch(c, c->beta_slab, beta_slab_bytes(c, mask)));
    const int bits[3] = {CMF_UPD_V, CMF_UPD_U, CMF_UPD_Z}, fs[3] = {CMF_V, CMF_U, CMF_Z}; // sweep order V, U, Z (cmf_solvers.py:248-263)
    for (int s = 0; s < 3; ++s) {
        if (!(mask & bits[s])) continue;
        float *num, *den;
        int n = 0;
        CHK(beta_sweep_passes(c, fs[s], beta, (float *)c->beta_slab.p, &num, &den, &n));
        CHK((pp_update<DEN_SLABS, true>(c, fs[s], num, den, n, l1, l2, beta_gamma(beta))));
    }
    return CMF_OK;
}

extern "C" int cmf_mu_beta_products(cmf_ctx *c, double beta, int sweep, float *num_out, float *den_out) {
    NEED_PROBLEM(c);
    CHK(beta_check(c, "cmf_mu_beta_products", beta));
    if (sweep < 0 || sweep > 2 || !num_out || !den_out) return fail(CMF_EINVAL, "cmf_mu_beta_products: sweep must be 0 (U), 1 (V) or 2 (Z) and the outputs non-null");
    const int f = sweep == 0 ? CMF_U : sweep == 1 ? CMF_V : CMF_Z;
    const int bit = sweep == 0 ? CMF_UPD_U : sweep == 1 ? CMF_UPD_V : CMF_UPD_Z;
    CHK(beta_sides_ok(c, "cmf_mu_beta_products", bit));
    DeviceGuard dg(c->device);
    CHK(ensure_scratch(c, c->beta_slab, beta_slab_bytes(c, bit)));
    float *num, *den;
    int n = 0;
    CHK(beta_sweep_passes(c, f, beta, (float *)c->beta_slab.p, &num, &den, &n));
    const int64_t stride = c->frows_pad[f] * c->kp, n4 = stride / 4;
    {
        Timed tm(c, CMF_K_ELEMWISE);
        const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 4096);
        hipLaunchKernelGGL(beta_sum_slabs_kernel, dim3(blocks), dim3(256), 0, c->stream, num, n, stride, n4);
        hipLaunchKernelGGL(beta_sum_slabs_kernel, dim3(blocks), dim3(256), 0, c->stream, den, n, stride, n4);
        HIPCHK(hipGetLastError());
    }
    const size_t bytes = (size_t)c->frows[f] * c->kp * sizeof(float);
    HIPCHK(hipMemcpyAsync(num_out, num, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(den_out, den, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

// D_beta(T || A B^T) of one side into *out
static int beta_divergence_side(cmf_ctx *c, double beta, int which, double *out) {
    const PairPass ps = which == 0 ? PP_U : PP_VY;
    int64_t S, per;
    kl_plan(c, ps, &S, &per);
    const dim3 grid = pp_grid(c, ps, S);
    CHK(ensure_scratch(c, c->beta_part, (size_t)grid.x * grid.y * sizeof(double)));
    PairPassArgs a = pp_args(c, ps, per);
    a.img0 = which == 0 ? c->X : c->Y;
    a.part = (double *)c->beta_part.p;
    a.param = (float)beta;
    double *sum = (double *)c->beta_small.p;
    {
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)c->frows[ps.fa] * (double)c->frows[ps.fb] * (double)c->k);
        if (beta == 0.0) CHK(pp_launch_reduce<BetaDivIS>(c, ps, a, S, sum));
        else if (beta == 1.0) CHK(pp_launch_reduce<KlDivergence>(c, ps, a, S, sum)); // the closed form divides by beta - 1
        else CHK(pp_launch_reduce<BetaDivGen>(c, ps, a, S, sum));
    }
    HIPCHK(hipMemcpyAsync(out, sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_beta_divergence(cmf_ctx *c, double beta, double *dx, double *dy) {
    NEED_PROBLEM(c);
    CHK(beta_check(c, "cmf_beta_divergence", beta));
    if (dx) CHK(beta_side_ok(c, "cmf_beta_divergence", 0));
    if (dy) CHK(beta_side_ok(c, "cmf_beta_divergence", 1));
    DeviceGuard dg(c->device);
    CHK(ensure_scratch(c, c->beta_small, 64));
    if (dx) CHK(beta_divergence_side(c, beta, 0, dx));
    if (dy) CHK(beta_divergence_side(c, beta, 1, dy));
    return CMF_OK;
}

extern "C" int cmf_mu_beta_layout(cmf_ctx *c, int64_t *out4) {
    NEED_PROBLEM(c);
    if (!out4) return fail(CMF_EINVAL, "cmf_mu_beta_layout: null output");
    CHK(beta_check(c, "cmf_mu_beta_layout", 0.0));
    int64_t S, S2, per;
    kl_plan(c, PP_U, &S, &per);
    out4[0] = S;
    kl_plan(c, PP_VX, &S, &per);
    kl_plan(c, PP_VY, &S2, &per);
    out4[1] = std::max(S, S2);
    kl_plan(c, PP_Z, &S, &per);
    out4[2] = S;
    out4[3] = (int64_t)(beta_slab_bytes(c, CMF_UPD_U | CMF_UPD_V | CMF_UPD_Z) + 64);
    return CMF_OK;
}
#endif // CMF_BETAMU_HOST
