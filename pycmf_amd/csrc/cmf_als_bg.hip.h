// cmf_als_bg.hip.h -- ALS for implicit feedback: a background weight c0 >= 0 on the cells OUTSIDE the stored pattern of a relation
// whose weights are bound as CSR (Hu, Koren, Volinsky: "Collaborative Filtering for Implicit Feedback Datasets").  Its term is
//   1/2 sum_{O} w_ic (t_ic - a_i . b_c)^2  +  1/2 c0 sum_{(i, c) not in O} (a_i . b_c)^2,        w_ic >= c0 on every stored entry
// -- the dense weighted objective with W = c0 and target 0 off the pattern.  With the EXCESS weights e_ic = w_ic - c0 >= 0 a row's
// system is the one of cmf_als.hip.h with two substitutions:
//   H_i = sum_{c in O_i} e_ic b_c b_c^T + c0 B^T B + (Gram of a full side) + l2 I,     g_i = sum_{c in O_i} w_ic t_ic b_c + N_i.
// So the row kernels (als_normal_kernel, als_nnls_kernel, als_cg_kernel) run unchanged: they read the excess array where they read
// wv, keep pv = w t, and the shared matrix S they already take becomes  sum_sides coef Gram(B_side),  coef = c0 for a side with a
// background and 1 for a full side.  What this file adds:
//   als_bg_excess_kernel   ev = wv - c0 (16-byte accesses) and the minimum of wv per workgroup -- the test w >= c0 runs where the
//                          values live; 16 bytes of static LDS
//   als_bg_combine_kernel  S = coef G, or S = S + coef G for the second side of a V sweep: products and sums rounded one by one (no
//                          fma), so the result does not depend on how a compiler pairs them and a repeated call is bit-identical
//   als_bg_res_csr_kernel<GL>  wmu_res_csr_kernel's term with a second sum (policy AlsBgResCsr of csr_reduce, cmf_pairpass.hip.h):
//                          one pass over the row image forms s = a_i . b_c in float32 and accumulates sum w (t - s)^2 AND sum s^2 in
//                          float64, one partial of each per workgroup in fixed slots (summed in slot order by sum_doubles_kernel);
//                          64 bytes of static LDS
//   als_bg_dot64_kernel    <G_a, G_b>_F of two float64 Grams in one workgroup, fixed order; 2 KB of static LDS
// The error of such a relation:  E = sum_O w (t - s)^2 + c0 (<A^T A, B^T B>_F - sum_O s^2),  clamped at 0.
// No atomics; nothing here writes through a scalar path.  c0 = 0 frees the excess arrays: every route is then the code without
// this file, byte for byte.
#pragma once
#include "cmf_kernels.hip.h"
#include "cmf_wmu.hip.h"

namespace cmfk {

__global__ __launch_bounds__(256) void als_bg_excess_kernel(const float *wv, float c0, float *ev, int64_t n, float *minpart) {
    const int64_t n4 = n >> 2;
    float mn = INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f32x4 w = reinterpret_cast<const f32x4 *>(wv)[i];
        mn = fminf(mn, fminf(fminf(w[0], w[1]), fminf(w[2], w[3])));
        reinterpret_cast<f32x4 *>(ev)[i] = f32x4{w[0] - c0, w[1] - c0, w[2] - c0, w[3] - c0};
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) { // the last n mod 4 entries
        const int64_t q = 4 * n4 + threadIdx.x;
        const float w = wv[q];
        mn = fminf(mn, w);
        ev[q] = w - c0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = fminf(mn, __shfl_down(mn, off, 64));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mn;
    __syncthreads();
    if (threadIdx.x == 0) minpart[blockIdx.x] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

__global__ void als_bg_combine_kernel(float *S, const float *G, float coef, int add, int n4) {
#pragma clang fp contract(off)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
        const f32x4 g = reinterpret_cast<const f32x4 *>(G)[i];
        f32x4 v{coef * g[0], coef * g[1], coef * g[2], coef * g[3]};
        if (add) {
            const f32x4 s = reinterpret_cast<const f32x4 *>(S)[i];
            v = f32x4{s[0] + v[0], s[1] + v[1], s[2] + v[2], s[3] + v[3]};
        }
        reinterpret_cast<f32x4 *>(S)[i] = v;
    }
}

// sum w (t - s)^2 AND sum s^2 over the stored entries, s = a_i . b_c in float32
struct AlsBgResCsr {
    enum { NS = 2, NV = 2 };
    static __device__ __forceinline__ void add(const float *tw, float d, double *acc) {
        const float e = tw[0] - d;
        acc[0] += (double)(tw[1] * (e * e));
        acc[1] += (double)(d * d);
    }
};
template <int GL>
__global__ __launch_bounds__(256) void als_bg_res_csr_kernel(PairCsrView T, const float *A, const float *B, int kp, double *partials) {
    csr_reduce<GL, AlsBgResCsr>(T, A, B, kp, partials);
}

__global__ __launch_bounds__(256) void als_bg_dot64_kernel(const double *a, const double *b, int64_t n, double *out) {
    __shared__ double red[256];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) v += a[i] * b[i];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als_bias.hip.h)
#ifdef CMF_ALS_HOST

// the weights the row kernels read for an observed side: the excess w - c0 under a background, w itself otherwise -- or, while a
// sweep has the reweighted arrays of the image bound (AlsReweightGuard, cmf_als_reweight.hip.h), the effective weights hw
static const float *als_side_weights(const WCsrDev &M) { return M.hbound ? M.hw : (M.ev ? M.ev : M.wv); }
// the products w t they read: w times the adjusted targets under biases (cmf_als_bias.hip.h), p = w t otherwise -- or, bound, the
// effective products hp
static const float *als_side_targets(const WCsrDev &M) { return M.hbound ? M.hp : (M.bp ? M.bp : M.pv); }

// does the sweep have a shared term (als_shared_terms sets S): a full relation, or an observed one under a background weight
static bool als_shared_present(const cmf_ctx *c, const AlsSweep &sw) {
    for (int s = 0; s < sw.nrel; ++s)
        if (!sw.observed[s] || c->wm_bg[sw.rel[s].which] > 0.0) return true;
    return false;
}

// The part of a sweep's systems that all its rows share: *S = sum_sides coef Gram(B_side) (coef: c0 of a side with a background,
// 1 of a full side; null when no side has either) and *N = T B of the full side (or null).  Without a background S is the Gram of
// the full side where gram32 leaves it (c->G2): nothing else is launched.
static int als_shared_terms(cmf_ctx *c, const AlsSweep &sw, const float **S, const float **N) {
    *S = *N = nullptr;
    bool bg = false;
    for (int s = 0; s < sw.nrel; ++s) bg = bg || (sw.observed[s] && c->wm_bg[sw.rel[s].which] > 0.0);
    const int n4 = c->kp * c->kp / 4;
    if (bg) CHK(ensure_scratch(c, c->als_bg_s, (size_t)n4 * 16));
    for (int s = 0; s < sw.nrel; ++s) {   // the order of als_rels: the sum of a V sweep is (coef_x G_u) + (coef_y G_z)
        const AlsRel &r = sw.rel[s];
        if (sw.observed[s] && !(c->wm_bg[r.which] > 0.0)) continue;
        CHK(gram32(c, c->F[r.fb], c->frows_pad[r.fb], c->G2));
        if (bg) {
            Timed tm(c, CMF_K_ELEMWISE);
            hipLaunchKernelGGL(cmfk::als_bg_combine_kernel, dim3((unsigned)std::min(64, (n4 + 255) / 256)), dim3(256), 0, c->stream, (float *)c->als_bg_s.p,
                               (const float *)c->G2, sw.observed[s] ? (float)c->wm_bg[r.which] : 1.0f, *S ? 1 : 0, n4);
            HIPCHK(hipGetLastError());
        }
        *S = bg ? (const float *)c->als_bg_s.p : c->G2;
        if (!sw.observed[s]) {
            CHK(data_times(c, r.which, r.data_trans, c->F[r.fb], c->num));
            *N = c->num;
        }
    }
    return CMF_OK;
}

static void als_bg_drop(cmf_ctx *c, int which) {
    for (int t = 0; t < 2; ++t) {
        dev_free(c, c->wm_sp[which][t].ev);
        c->wm_sp[which][t].ev = nullptr;
    }
    c->wm_bg[which] = 0.0;
}

extern "C" int cmf_set_background_weight(cmf_ctx *c, int which, double c0) {
    NEED_PROBLEM(c);
    if (which != 0 && which != 1) return fail(CMF_EINVAL, "cmf_set_background_weight: which must be 0 (X) or 1 (Y)");
    const char *nm = which == 0 ? "X" : "Y";
    if (c->wm_kind[which] != WM_CSR)
        return fail(CMF_EINVAL, "cmf_set_background_weight: %s has no CSR weights bound (cmf_set_weighted_csr first)", nm);
    const float cf = (float)c0;
    if (!(c0 >= 0.0) || !std::isfinite(c0) || !std::isfinite(cf))
        return fail(CMF_EINVAL, "cmf_set_background_weight: the background weight must be finite and >= 0 (in float32), got %g", c0);
    if (cf > 0.f && c->als_bias[which].on)
        return fail(CMF_EUNSUPPORTED, "cmf_set_background_weight: %s has biases bound; biases and a background weight are not built together: "
                                      "clear them with cmf_set_biases(ctx, %d, 0, 0, 0)", nm, which);
    DeviceGuard dg(c->device);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (cf == 0.f) {
        als_bg_drop(c, which);
        return CMF_OK;
    }
    float *ev[2] = {nullptr, nullptr};
    unsigned blocks0 = 1;
    for (int t = 0; t < 2; ++t) {
        const WCsrDev &M = c->wm_sp[which][t];
        const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(1024, ((M.nnz >> 2) + 255) / 256));
        if (t == 0) blocks0 = blocks;
        int rc = dev_alloc(c, (void **)&ev[t], std::max<size_t>((size_t)M.nnz * sizeof(float), 16), false);
        if (rc == CMF_OK) rc = ensure_scratch(c, c->wm_part, 2 * 1024 * sizeof(float));
        if (rc != CMF_OK) {
            dev_free(c, ev[0]); dev_free(c, ev[1]);
            return rc;
        }
        Timed tm(c, CMF_K_ELEMWISE);
        hipLaunchKernelGGL(cmfk::als_bg_excess_kernel, dim3(blocks), dim3(256), 0, c->stream, (const float *)M.wv, cf, ev[t], M.nnz,
                           (float *)c->wm_part.p + 1024 * t);
    }
    float mins[1024];
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(mins, c->wm_part.p, blocks0 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    float mn = INFINITY;
    for (unsigned b = 0; he == hipSuccess && b < blocks0; ++b) mn = std::min(mn, mins[b]);
    if (he != hipSuccess || mn < cf) {
        (void)hipStreamSynchronize(c->stream);
        dev_free(c, ev[0]); dev_free(c, ev[1]);
        if (he != hipSuccess) return fail(CMF_EHIP, "cmf_set_background_weight: %s", hipGetErrorString(he));
        return fail(CMF_EINVAL, "cmf_set_background_weight: a stored weight of %s (%g) lies below the background weight %g: every stored entry must "
                                "count at least as much as an unobserved cell", nm, (double)mn, (double)cf);
    }
    als_bg_drop(c, which);
    c->wm_sp[which][0].ev = ev[0];
    c->wm_sp[which][1].ev = ev[1];
    c->wm_bg[which] = (double)cf;
    return CMF_OK;
}

extern "C" int cmf_get_background_weight(cmf_ctx *c, int which, double *c0) {
    NEED_PROBLEM(c);
    if ((which != 0 && which != 1) || !c0) return fail(CMF_EINVAL, "cmf_get_background_weight: which must be 0 (X) or 1 (Y) and the output non-null");
    *c0 = c->wm_bg[which];
    return CMF_OK;
}

// E of one relation with CSR weights into *out (file header); without a background: the weighted residual, the same launches
static int als_bg_residual_side(cmf_ctx *c, int which, double *out) {
    if (c->als_bias[which].on) {   // (never together with a background) the residual of the biased model: bt where the pass reads t
        CHK(als_bias_refresh(c, which));
        return wm_residual_side(c, which, out, c->wm_sp[which][0].bt);
    }
    if (!(c->wm_bg[which] > 0.0)) return wm_residual_side(c, which, out);
    const int fa = which == 0 ? CMF_U : CMF_V, fb = which == 0 ? CMF_V : CMF_Z;
    const float *A = c->F[fa], *B = c->F[fb];
    const int64_t kk = (int64_t)c->kp * c->kp;
    CHK(ensure_scratch(c, c->wm_small, 64));
    CHK(ensure_scratch(c, c->als_bg64, (size_t)2 * kk * sizeof(double)));
    double *sum = (double *)c->wm_small.p, *Ga = (double *)c->als_bg64.p, *Gb = Ga + kk;
    const WCsrDev &M = c->wm_sp[which][0];
    cmfk::PairCsrView v{M.indptr, M.idx, M.pv, M.wv, M.tv, M.rows};
    CHK(ensure_scratch(c, c->wm_part, (size_t)2 * csr_reduce_blocks(c, M.rows) * sizeof(double)));
    {
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
        double *part = (double *)c->wm_part.p;
        CHK(csr_launch_reduce<2>(c, M.rows, part, sum, [&](auto gl, dim3 grid) {
            hipLaunchKernelGGL((cmfk::als_bg_res_csr_kernel<decltype(gl)::value>), grid, dim3(256), 0, c->stream, v, A, B, c->kp, part);
        }));
    }
    CHK(gram64(c, A, c->frows_pad[fa], Ga, nullptr));
    CHK(gram64(c, B, c->frows_pad[fb], Gb, nullptr));
    {
        Timed tm(c, CMF_K_GEMM_SMALL, 2.0 * (double)kk);
        hipLaunchKernelGGL(cmfk::als_bg_dot64_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)Ga, (const double *)Gb, kk, sum + 2);
        HIPCHK(hipGetLastError());
    }
    double h[3];
    HIPCHK(hipMemcpyAsync(h, sum, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = std::max(0.0, h[0] + c->wm_bg[which] * (h[2] - h[1]));
    return CMF_OK;
}

extern "C" int cmf_als_residual_sq(cmf_ctx *c, double *ex, double *ey) {
    NEED_PROBLEM(c);
    CHK(wm_check(c, "cmf_als_residual_sq"));
    double *want[2] = {ex, ey};
    for (int w = 0; w < 2; ++w)
        if (want[w] && c->wm_kind[w] != WM_CSR)
            return fail(CMF_EINVAL, "cmf_als_residual_sq: %s has no CSR weights bound (cmf_set_weighted_csr); a full relation's error is cmf_residual_sq",
                        w == 0 ? "X" : "Y");
    DeviceGuard dg(c->device);
    for (int w = 0; w < 2; ++w)
        if (want[w]) CHK(als_bg_residual_side(c, w, want[w]));
    return CMF_OK;
}

#endif // CMF_ALS_HOST
