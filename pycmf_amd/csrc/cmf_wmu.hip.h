// cmf_wmu.hip.h -- multiplicative updates with per-entry weights on the Frobenius objective
//   1/2 |sqrt(Wx) .* (X - U V^T)|^2 + 1/2 |sqrt(Wy) .* (Y - V Z^T)|^2      (Wx, Wy >= 0, fixed; a 0/1 mask = observed entries only).
//
// The weighted update of a factor needs  D = (W .* (A B^T)) B : an element-wise product BETWEEN two products over the same tiles.
// The m x d intermediate is never written to memory: the fused two-product pass of cmf_pairpass.hip.h (steps 1 to 3 there) runs
// with the policies of this file.
//   WmDen    steps 1 to 3: the 16 registers times the 16 elements of W that face them, D^T += B_tile^T (W .* S)^T
//   WmDen1   W == 1: steps 1 and 3, no W loads (the unweighted relation of a weighted fit; no matrix of ones is ever allocated)
//   WmNum    step 3 alone, the registers loaded from P = W .* T (formed once when the weights are bound; for an unweighted
//            relation P is the data image itself): N = P B in the same tiles, shares and summation order as D
//   WmRes / WmRes1   step 1, then w (t - s)^2 (WmRes1: (t - s)^2) per valid element: every term in float32 in the DIRECT form
// A share whose slab already holds the other relation's contribution (V sweep: X^T side, then Y side) adds to it (acc_slabs).
// Padding: rows and columns of W, T, A and B beyond the valid extent are zero and contribute exact zeros.
//
// wmu_csr_kernel<GL>: weights held as CSR -- the loss runs over the stored pattern only.  One pattern, value arrays p = w t
// and w (and t on the row image, for the residual).  A group of GL lanes owns an output row; per stored entry the gathered row
// B_c serves the dot with the owned row (DPP group_sum), then den += (w dot) B_c and num += p B_c, in stored order.
// wmu_res_csr_kernel<GL>: sum over the stored entries of w (t - A_r . B_c)^2.
// The update: F <- F * (sum of the numerator slabs) / reg(sum of the denominator slabs, F)   (pairpass_update_kernel<DEN_SLABS>;
// cmf_solvers.py:212-228, gamma = 1).
//
// Reference counterpart: none -- its README lists "Add support for weight matrices on relations" as an open item.
#pragma once
#include "cmf_pairpass.hip.h"

namespace cmfk {

struct WmDen { // img0 = W
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static constexpr bool ADDS = true; // the Y side of a V sweep adds to the X side's slabs: so do the other two
    static __device__ __forceinline__ float map(float s, float w, float) { return w * s; }
};
struct WmDen1 {
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 0;
    static constexpr bool ADDS = true;
    static __device__ __forceinline__ float map(float s, float, float) { return s; }
};
struct WmNum { // img0 = P
    static constexpr bool DOT = false;
    static constexpr int IMAGES = 1;
    static constexpr bool ADDS = true;
    static __device__ __forceinline__ float map(float, float p, float) { return p; }
};
struct WmRes { // img0 = W, img1 = T
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 2;
    static __device__ __forceinline__ double term(float s, float w, float t) {
        const float e = t - s;
        float term = e * e;
        term = w * term;
        return (double)term;
    }
};
struct WmRes1 { // img0 = T
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static __device__ __forceinline__ double term(float s, float t, float) {
        const float e = t - s;
        return (double)(e * e);
    }
};

// ------------------------------------------------------------------ weights held as CSR
// num[r, :] (+)= sum over the stored (r, c) of p B_c,  den[r, :] (+)= sum of (w A_r . B_c) B_c;  rows beyond T.rows count as empty.
template <int GL>
__global__ __launch_bounds__(256) void wmu_csr_kernel(PairCsrView T, const float *A, const float *B, int kp, int64_t rows_pad, float *num, float *den, int add) {
    int gl;
    const int64_t row = csr_group_row<GL>(&gl);
    if (row >= rows_pad) return;
    f32x4 nu = f32x4{0.f, 0.f, 0.f, 0.f}, de = nu;
    const float *val[2] = {T.pv, T.wv};
    if (row < T.rows)
        csr_row_pairs<GL, 2>(T.indptr, T.idx, val, A, B, kp, row, gl, [&](const float *pw, float d, const f32x4 &b) {
            const float wd = pw[1] * d;
            de += wd * b;
            nu += pw[0] * b;
        });
    f32x4 *pn = reinterpret_cast<f32x4 *>(num + row * kp + 4 * gl);
    f32x4 *pd = reinterpret_cast<f32x4 *>(den + row * kp + 4 * gl);
    if (add) {
        nu += *pn;
        de += *pd;
    }
    *pn = nu;
    *pd = de;
}

// sum over the stored entries of  w (t - A_r . B_c)^2, every term in float32, one float64 partial per workgroup.  Not a policy of
// csr_reduce: inside that body the compiler contracts the dot into another fma pattern than it does here, and the sum
// this kernel returns is pinned to the bit.
template <int GL>
__global__ __launch_bounds__(256) void wmu_res_csr_kernel(PairCsrView T, const float *A, const float *B, int kp, double *partials) {
    int gl;
    const int64_t row = csr_group_row<GL>(&gl);
    double acc = 0.0;
    if (row < T.rows) {
        const f32x4 a = csr_lane4(A, row, kp, gl);
        const int64_t beg = T.indptr[row], end = T.indptr[row + 1];
        for (int64_t q = beg; q < end; ++q) {
            const int32_t j = T.idx[q];
            const float t = T.tv[q], w = T.wv[q];
            const f32x4 b = csr_lane4(B, j, kp, gl);
            float d = 0.f;
            d += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
            d = group_sum<GL>(d);
            const float e = t - d;
            if (gl == 0) acc += (double)(w * (e * e));
        }
    }
    __shared__ double red[4];
    const double v = block_sum64(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = v;
}

// ------------------------------------------------------------------ P = W .* T and the update
__global__ void wmu_mul_kernel(float *P, const float *W, const float *T, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<f32x4 *>(P)[i] = reinterpret_cast<const f32x4 *>(W)[i] * reinterpret_cast<const f32x4 *>(T)[i];
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx)
#ifdef CMF_WMU_HOST

enum { WM_NONE = 0, WM_DENSE = 1, WM_CSR = 2 }; // how the weights of a relation are held (cmf_ctx::wm_kind)

static float *wm_data(const cmf_ctx *c, int which) { return which == 0 ? c->X : c->Y; }

static void wm_free_side(cmf_ctx *c, int which) {
    als_bias_free(c, which);   // biases (cmf_als_bias.hip.h) go with the weights they were set on, as a background weight does
    als_reweight_free(c, which);  // ... and what the entry passes built for their pattern (cmf_als_reweight.hip.h; the delta stays)
    dev_free(c, c->wm_w[which]); dev_free(c, c->wm_p[which]);
    c->wm_w[which] = c->wm_p[which] = nullptr;
    for (int t = 0; t < 2; ++t) {
        WCsrDev &M = c->wm_sp[which][t];
        dev_free(c, M.indptr); dev_free(c, M.idx); dev_free(c, M.pv); dev_free(c, M.wv); dev_free(c, M.tv); dev_free(c, M.ev);
        M = WCsrDev();
    }
    c->wm_kind[which] = WM_NONE;
    c->wm_bg[which] = 0.0;   // a background weight (cmf_als_bg.hip.h) goes with the weights it was set on
}

// pp_plan's share rule (option "wmu_split" forces the count); S = 1 for weights held as CSR
static void wm_plan(const cmf_ctx *c, const PairPass &ps, int64_t *S, int64_t *per) { pp_plan(c, ps, c->opt_wmu_split, c->wm_kind[ps.which] == WM_CSR, S, per); }

// scratch of a step: numerator and denominator slabs of the widest sweep (the two passes of the V sweep share their slabs)
static int64_t wm_sweep_slabs(const cmf_ctx *c, int f) {
    int64_t S, S2 = 0, per;
    if (f == CMF_V) { wm_plan(c, PP_VX, &S, &per); wm_plan(c, PP_VY, &S2, &per); }
    else wm_plan(c, f == CMF_U ? PP_U : PP_Z, &S, &per);
    return std::max(S, S2);
}
static size_t wm_slab_bytes(const cmf_ctx *c, int mask) {
    size_t need = 0;
    const int bits[3] = {CMF_UPD_U, CMF_UPD_V, CMF_UPD_Z};
    for (int f = 0; f < 3; ++f)
        if (mask & bits[f]) need = std::max(need, (size_t)2 * wm_sweep_slabs(c, f) * c->frows_pad[f] * c->kp * sizeof(float));
    return need;
}

static int wm_check(cmf_ctx *c, const char *what) {
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: k_pad = %d (n_components above 256) is not supported by the weighted passes", what, c->kp);
    return CMF_OK;
}
// a relation can take part: weights held as CSR carry their own data; otherwise the dense image is needed
static int wm_side_ok(cmf_ctx *c, const char *what, int which) {
    if (c->wm_kind[which] == WM_CSR) return CMF_OK;
    if (!have_data(c, which)) return fail(CMF_EINVAL, "%s: %s has not been set", what, which == 0 ? "X" : "Y");
    if (!wm_data(c, which))
        return fail(CMF_EUNSUPPORTED, "%s: %s is held as native CSR without weights; an unweighted relation beside a weighted one needs its dense image "
                                      "(sparse_mode 1), or bind it through cmf_set_weighted_csr", what, which == 0 ? "X" : "Y");
    return CMF_OK;
}

// numerator and denominator slabs of one pass (slab stride = rows_pad * k_pad); the first `have` slabs hold the sweep's other
// pass and are added to; *nslab = how many slabs this pass touched
static int wm_pass(cmf_ctx *c, const PairPass &ps, float *num, float *den, int have, int *nslab) {
    if (c->wm_kind[ps.which] == WM_CSR) {
        const int64_t rows_pad = c->frows_pad[ps.fa];
        const float *A = c->F[ps.fa], *B = c->F[ps.fb];
        const WCsrDev &M = c->wm_sp[ps.which][ps.trans ? 1 : 0];
        PairCsrView v{M.indptr, M.idx, M.pv, M.wv, M.tv, M.rows};
        Timed tm(c, CMF_K_KLMU, 6.0 * (double)M.nnz * (double)c->kp);
        const int gl = c->kp / 4, rpw = 64 / gl;
        const unsigned blocks = (unsigned)(rows_pad / (4 * rpw));
        const int add = have > 0 ? 1 : 0;
        with_kp(c->kp, [&](auto kp) {
            hipLaunchKernelGGL((wmu_csr_kernel<decltype(kp)::value / 4>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, num, den, add);
        });
        HIPCHK(hipGetLastError());
        *nslab = 1;
        return CMF_OK;
    }
    int64_t S, per;
    wm_plan(c, ps, &S, &per);
    const bool weighted = c->wm_kind[ps.which] == WM_DENSE;
    PairPassArgs a = pp_args(c, ps, per);
    a.acc_slabs = have;
    const double cells = (double)c->frows[ps.fa] * (double)c->frows[ps.fb];
    {
        Timed tm(c, CMF_K_KLMU, 4.0 * cells * (double)c->k);
        a.img0 = c->wm_w[ps.which];
        a.out = den;
        if (weighted) CHK(pp_launch_pass<WmDen>(c, ps, a, S));
        else CHK(pp_launch_pass<WmDen1>(c, ps, a, S));
    }
    {
        Timed tm(c, ps.trans ? CMF_K_GEMM_TN : CMF_K_GEMM_NN, 2.0 * cells * (double)c->k);
        a.img0 = weighted ? c->wm_p[ps.which] : wm_data(c, ps.which);
        a.out = num;
        CHK(pp_launch_pass<WmNum>(c, ps, a, S));
    }
    *nslab = (int)S;
    return CMF_OK;
}

extern "C" int cmf_mu_weighted_step(cmf_ctx *c, double l1, double l2, int mask) {
    NEED_PROBLEM(c);
    CHK(wm_check(c, "cmf_mu_weighted_step"));
    if (mask & (CMF_UPD_U | CMF_UPD_V)) CHK(wm_side_ok(c, "cmf_mu_weighted_step", 0));
    if (mask & (CMF_UPD_Z | CMF_UPD_V)) CHK(wm_side_ok(c, "cmf_mu_weighted_step", 1));
    for (int w = 0; w < 2; ++w)
        if (c->wm_bg[w] > 0.0 && (mask & ((w == 0 ? CMF_UPD_U : CMF_UPD_Z) | CMF_UPD_V)))
            return fail(CMF_EUNSUPPORTED, "cmf_mu_weighted_step: %s has a background weight bound, which only the ALS steps honour; "
                                          "clear it with cmf_set_background_weight(ctx, %d, 0)", w == 0 ? "X" : "Y", w);
    for (int w = 0; w < 2; ++w)
        if (c->als_bias[w].on && (mask & ((w == 0 ? CMF_UPD_U : CMF_UPD_Z) | CMF_UPD_V)))
            return fail(CMF_EUNSUPPORTED, "cmf_mu_weighted_step: %s has biases bound, which only cmf_als_bias_step honours; "
                                          "clear them with cmf_set_biases(ctx, %d, 0, 0, 0)", w == 0 ? "X" : "Y", w);
    DeviceGuard dg(c->device);
    CHK(ensure_scratch(c, c->wm_slab, wm_slab_bytes(c, mask)));
    float *base = (float *)c->wm_slab.p;
    const int bits[3] = {CMF_UPD_V, CMF_UPD_U, CMF_UPD_Z}, fs[3] = {CMF_V, CMF_U, CMF_Z}; // sweep order V, U, Z (cmf_solvers.py:248-263)
    for (int s = 0; s < 3; ++s) {
        if (!(mask & bits[s])) continue;
        const int f = fs[s];
        float *num = base, *den = base + wm_sweep_slabs(c, f) * c->frows_pad[f] * c->kp;
        int n1 = 0, n2 = 0;
        if (f == CMF_V) {
            CHK(wm_pass(c, PP_VX, num, den, 0, &n1));
            CHK(wm_pass(c, PP_VY, num, den, n1, &n2));
        } else
            CHK(wm_pass(c, f == CMF_U ? PP_U : PP_Z, num, den, 0, &n1));
        CHK(pp_update<DEN_SLABS>(c, f, num, den, std::max(n1, n2), l1, l2));
    }
    return CMF_OK;
}

// sum of w (t - s)^2 over one relation into *out
// (targets: what the CSR pass reads as t -- the adjusted targets of a biased relation for cmf_als_residual_sq; null: t itself)
static int wm_residual_side(cmf_ctx *c, int which, double *out, const float *targets = nullptr) {
    const PairPass ps = which == 0 ? PP_U : PP_VY;
    CHK(ensure_scratch(c, c->wm_small, 64));
    double *sum = (double *)c->wm_small.p;
    if (c->wm_kind[which] == WM_CSR) {
        const WCsrDev &M = c->wm_sp[which][0];
        PairCsrView v{M.indptr, M.idx, M.pv, M.wv, targets ? targets : M.tv, M.rows};
        CHK(ensure_scratch(c, c->wm_part, (size_t)csr_reduce_blocks(c, M.rows) * sizeof(double)));
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
        const float *A = c->F[ps.fa], *B = c->F[ps.fb];
        double *part = (double *)c->wm_part.p;
        CHK(csr_launch_reduce<1>(c, M.rows, part, sum, [&](auto gl, dim3 grid) {
            hipLaunchKernelGGL((wmu_res_csr_kernel<decltype(gl)::value>), grid, dim3(256), 0, c->stream, v, A, B, c->kp, part);
        }));
    } else {
        int64_t S, per;
        wm_plan(c, ps, &S, &per);
        const dim3 grid = pp_grid(c, ps, S);
        CHK(ensure_scratch(c, c->wm_part, (size_t)grid.x * grid.y * sizeof(double)));
        const bool weighted = c->wm_kind[which] == WM_DENSE;
        PairPassArgs a = pp_args(c, ps, per);
        a.img0 = weighted ? c->wm_w[which] : wm_data(c, which);
        a.img1 = wm_data(c, which);
        a.part = (double *)c->wm_part.p;
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)c->frows[ps.fa] * (double)c->frows[ps.fb] * (double)c->k);
        if (weighted) CHK(pp_launch_reduce<WmRes>(c, ps, a, S, sum));
        else CHK(pp_launch_reduce<WmRes1>(c, ps, a, S, sum));
    }
    HIPCHK(hipMemcpyAsync(out, sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_weighted_residual_sq(cmf_ctx *c, double *ex, double *ey) {
    NEED_PROBLEM(c);
    CHK(wm_check(c, "cmf_weighted_residual_sq"));
    if (ex) CHK(wm_side_ok(c, "cmf_weighted_residual_sq", 0));
    if (ey) CHK(wm_side_ok(c, "cmf_weighted_residual_sq", 1));
    DeviceGuard dg(c->device);
    if (ex) CHK(wm_residual_side(c, 0, ex));
    if (ey) CHK(wm_residual_side(c, 1, ey));
    return CMF_OK;
}

extern "C" int cmf_mu_weighted_layout(cmf_ctx *c, int64_t *out4) {
    NEED_PROBLEM(c);
    if (!out4) return fail(CMF_EINVAL, "cmf_mu_weighted_layout: null output");
    CHK(wm_check(c, "cmf_mu_weighted_layout"));
    out4[0] = wm_sweep_slabs(c, CMF_U);
    out4[1] = wm_sweep_slabs(c, CMF_V);
    out4[2] = wm_sweep_slabs(c, CMF_Z);
    out4[3] = (int64_t)(wm_slab_bytes(c, CMF_UPD_U | CMF_UPD_V | CMF_UPD_Z) + 64);
    return CMF_OK;
}

// P = W .* T behind a (re)written dense W image
static int wm_form_p(cmf_ctx *c, int which, int64_t rp, int64_t cp) {
    if (!c->wm_p[which]) CHK(dev_alloc(c, (void **)&c->wm_p[which], (size_t)rp * cp * sizeof(float), false));
    const int64_t n4 = rp * cp / 4;
    Timed tm(c, CMF_K_ELEMWISE);
    const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 8192);
    hipLaunchKernelGGL(wmu_mul_kernel, dim3(blocks), dim3(256), 0, c->stream, c->wm_p[which], (const float *)c->wm_w[which], (const float *)wm_data(c, which), n4);
    HIPCHK(hipGetLastError());
    c->wm_kind[which] = WM_DENSE;
    return CMF_OK;
}
// the relation's dense image must exist; a zeroed W image of its padded shape
static int wm_dense_begin(cmf_ctx *c, const char *what, int which, int64_t *r, int64_t *cc, int64_t *rp, int64_t *cp) {
    float **slot;
    CHK(data_dims(c, which, r, cc, rp, cp, &slot));
    if (!*slot) return fail(CMF_EINVAL, "%s: dense weights need the dense image of %s: set the data first (a native CSR relation takes cmf_set_weighted_csr)",
                            what, which == 0 ? "X" : "Y");
    HIPCHK(hipStreamSynchronize(c->stream));
    wm_free_side(c, which);
    CHK(dev_alloc(c, (void **)&c->wm_w[which], (size_t)*rp * *cp * sizeof(float)));
    return CMF_OK;
}

template <typename T>
static int wm_set_weight(cmf_ctx *c, int which, const T *ptr, int64_t rs, int64_t cs) {
    NEED_PROBLEM(c);
    if (!ptr) return fail(CMF_EINVAL, "null weight pointer");
    DeviceGuard dg(c->device);
    int64_t r, cc, rp, cp;
    CHK(wm_dense_begin(c, "cmf_set_weight", which, &r, &cc, &rp, &cp));
    CHK(upload_strided<T>(c, c->wm_w[which], cp, r, cc, ptr, rs, cs));
    return wm_form_p(c, which, rp, cp);
}
extern "C" int cmf_set_weight_f64(cmf_ctx *c, int which, const double *ptr, int64_t rs, int64_t cs) { return wm_set_weight<double>(c, which, ptr, rs, cs); }
extern "C" int cmf_set_weight_f32(cmf_ctx *c, int which, const float *ptr, int64_t rs, int64_t cs) { return wm_set_weight<float>(c, which, ptr, rs, cs); }

extern "C" int cmf_fill_weight_synthetic(cmf_ctx *c, int which, uint64_t seed, double density) {
    NEED_PROBLEM(c);
    if (!(density >= 0.0 && density <= 1.0)) return fail(CMF_EINVAL, "cmf_fill_weight_synthetic: density must lie in [0, 1]");
    DeviceGuard dg(c->device);
    int64_t r, cc, rp, cp;
    CHK(wm_dense_begin(c, "cmf_fill_weight_synthetic", which, &r, &cc, &rp, &cp));
    CHK(launch_fill(c, c->wm_w[which], cp, r, cc, seed, 0, 0, (float)density, 2));
    return wm_form_p(c, which, rp, cp);
}

extern "C" int cmf_get_weight_block_f32(cmf_ctx *c, int which, int64_t row0, int64_t nrows, int64_t col0, int64_t ncols, float *dst) {
    NEED_PROBLEM(c);
    DeviceGuard dg(c->device);
    int64_t r, cc, rp, cp; float **slot;
    CHK(data_dims(c, which, &r, &cc, &rp, &cp, &slot));
    if (!dst || row0 < 0 || col0 < 0 || nrows < 0 || ncols < 0 || row0 + nrows > r || col0 + ncols > cc) return fail(CMF_EINVAL, "block out of range");
    if (c->wm_kind[which] != WM_DENSE) return fail(CMF_EINVAL, "%s has no dense weight image", which == 0 ? "X" : "Y");
    if (nrows == 0 || ncols == 0) return CMF_OK;
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)ncols * sizeof(float), c->wm_w[which] + row0 * cp + col0, (size_t)cp * sizeof(float), (size_t)ncols * sizeof(float),
                            (size_t)nrows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_clear_weight(cmf_ctx *c, int which) {
    NEED_PROBLEM(c);
    if (which != 0 && which != 1) return fail(CMF_EINVAL, "which must be 0 (X) or 1 (Y)");
    DeviceGuard dg(c->device);
    HIPCHK(hipStreamSynchronize(c->stream));
    wm_free_side(c, which);
    return CMF_OK;
}

static int wm_csr_upload(cmf_ctx *c, WCsrDev &dst, const std::vector<int64_t> &indptr, const std::vector<int32_t> &idx, const std::vector<float> &p,
                         const std::vector<float> &w, const std::vector<float> *t, int64_t rows, int64_t cols) {
    const int64_t nnz = (int64_t)idx.size();
    dst.rows = rows; dst.cols = cols; dst.nnz = nnz;
    auto up = [&](void **dptr, const void *src, size_t bytes) -> int {
        CHK(dev_alloc(c, dptr, std::max<size_t>(bytes, 16), false));
        if (bytes) HIPCHK(hipMemcpyAsync(*dptr, src, bytes, hipMemcpyHostToDevice, c->stream));
        return CMF_OK;
    };
    CHK(up((void **)&dst.indptr, indptr.data(), (size_t)(rows + 1) * sizeof(int64_t)));
    CHK(up((void **)&dst.idx, idx.data(), (size_t)nnz * sizeof(int32_t)));
    CHK(up((void **)&dst.pv, p.data(), (size_t)nnz * sizeof(float)));
    CHK(up((void **)&dst.wv, w.data(), (size_t)nnz * sizeof(float)));
    if (t) CHK(up((void **)&dst.tv, t->data(), (size_t)nnz * sizeof(float)));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vectors may go
    return CMF_OK;
}

extern "C" int cmf_set_weighted_csr(cmf_ctx *c, int which, const int64_t *indptr, const int32_t *indices, const double *t_values, const double *w_values) {
    NEED_PROBLEM(c);
    DeviceGuard dg(c->device);
    int64_t r, cc, rp, cp; float **slot;
    CHK(data_dims(c, which, &r, &cc, &rp, &cp, &slot));
    if (!indptr) return fail(CMF_EINVAL, "null CSR pointer");
    if (indptr[0] != 0) return fail(CMF_EINVAL, "CSR indptr[0] must be 0");
    for (int64_t i = 0; i < r; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(CMF_EINVAL, "CSR indptr is not monotonic at row %lld", (long long)i);
    const int64_t nnz = indptr[r];
    if (nnz > 0 && (!indices || !t_values || !w_values)) return fail(CMF_EINVAL, "null CSR pointer");
    for (int64_t q = 0; q < nnz; ++q) {
        if (indices[q] < 0 || indices[q] >= cc) return fail(CMF_EINVAL, "CSR column index out of range");
        if (!(w_values[q] >= 0.0) || !std::isfinite(w_values[q])) return fail(CMF_EINVAL, "weights must be finite and non-negative");
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    wm_free_side(c, which);
    std::vector<int64_t> ip(indptr, indptr + r + 1), ipt((size_t)cc + 1, 0);
    std::vector<int32_t> ix(indices, indices + nnz), ixt((size_t)nnz);
    std::vector<float> t((size_t)nnz), w((size_t)nnz), p((size_t)nnz), pt((size_t)nnz), wt((size_t)nnz);
    for (int64_t q = 0; q < nnz; ++q) {
        t[q] = (float)t_values[q];
        w[q] = (float)w_values[q];
        p[q] = w[q] * t[q];
    }
    // the transposed image: counting sort by column, rows ascending inside a column (stored order of the transpose)
    for (int64_t q = 0; q < nnz; ++q) ipt[(size_t)ix[q] + 1]++;
    for (int64_t j = 0; j < cc; ++j) ipt[(size_t)j + 1] += ipt[(size_t)j];
    {
        std::vector<int64_t> pos(ipt.begin(), ipt.end() - 1);
        for (int64_t i = 0; i < r; ++i)
            for (int64_t q = ip[i]; q < ip[i + 1]; ++q) {
                const int64_t o = pos[(size_t)ix[q]]++;
                ixt[o] = (int32_t)i; pt[o] = p[q]; wt[o] = w[q];
            }
    }
    CHK(wm_csr_upload(c, c->wm_sp[which][0], ip, ix, p, w, &t, r, cc));
    CHK(wm_csr_upload(c, c->wm_sp[which][1], ipt, ixt, pt, wt, nullptr, cc, r));
    c->wm_kind[which] = WM_CSR;
    return CMF_OK;
}
#endif // CMF_WMU_HOST
