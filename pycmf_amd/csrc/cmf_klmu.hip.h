// cmf_klmu.hip.h -- multiplicative updates for the generalised Kullback-Leibler objective  D(X || U V^T) + D(Y || V Z^T).
//
// The KL update of a factor needs  N = (T ./ max(A B^T, EPS)) B : an element-wise quotient BETWEEN two products over the same tiles
// (sklearn's _multiplicative_update_w / _h with beta_loss = 1, applied to each block of the collective model).  The quotient tile
// is never written to memory: the fused two-product pass of cmf_pairpass.hip.h runs with the two policies of this file.
//   KlQuotient    the 16 registers of a sub-tile become quotients in place, q = t * rcp(max(s, EPS)), against the matching elements
//                 of T.  A zero of T gives an exact zero; so do the padded rows and columns (0 * rcp(EPS)).
//   KlDivergence  t log(t / s) - t + s  (t = 0: s; s = 0: EPS in the quotient) over the valid rows and columns.
// kl_quotient_csr_kernel<GL> / kl_div_csr_kernel<GL> (policy KlDivCsr of csr_reduce): the same for a native CSR T -- a group of GL lanes owns an output row and uses the
// gathered row of B twice per stored entry: for the dot with its own row (DPP group_sum) and for the update.
// kl_colsum_*: column sums of a factor in a fixed order (partials per row chunk, then one pass over the partials).
// The update: F <- F * (sum of the numerator slabs) / reg(colsum, F)   (pairpass_update_kernel<DEN_COLSUM>; cmf_solvers.py:212-228 with
// gamma = 1).
//
// Reference counterpart: none -- pycmf/cmf.py:245-247 documents beta_loss='kullback-leibler' and states that it is not implemented.
#pragma once
#include "cmf_pairpass.hip.h"

namespace cmfk {

struct KlQuotient { // img0 = T
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static constexpr bool ADDS = false; // the passes of a V sweep keep slabs of their own
    static __device__ __forceinline__ float map(float s, float t, float) { return t * __builtin_amdgcn_rcpf(fmaxf(s, CMF_MU_EPS)); }
};
struct KlDivergence { // img0 = T
    static constexpr bool DOT = true;
    static constexpr int IMAGES = 1;
    static __device__ __forceinline__ double term(float s, float tt, float) {
        double e = (double)s;
        if (tt > 0.f) e += (double)(tt * logf(tt / (s > 0.f ? s : CMF_MU_EPS))) - (double)tt; // s = 0: EPS, as sklearn's _beta_divergence
        return e;
    }
};

// ------------------------------------------------------------------ native CSR
// out[r, :] = sum over the stored (r, c, t) of  t / max(A_r . B_c, EPS)  B_c ; rows beyond T.rows (padding) are written as zeros.
template <int GL>
__global__ __launch_bounds__(256) void kl_quotient_csr_kernel(CsrView T, const float *A, const float *B, int kp, int64_t rows_pad, float *out) {
    int gl;
    const int64_t row = csr_group_row<GL>(&gl);
    if (row >= rows_pad) return;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *val[1] = {T.val};
    if (row < T.rows)
        csr_row_pairs<GL, 1>(T.indptr, T.idx, val, A, B, kp, row, gl, [&](const float *v, float d, const f32x4 &b) {
            const float w = v[0] * __builtin_amdgcn_rcpf(fmaxf(d, CMF_MU_EPS));
            acc += w * b;
        });
    *reinterpret_cast<f32x4 *>(out + row * kp + 4 * gl) = acc;
}

// sum over the stored entries of  t log(t / (A_r . B_c)) - t  (t > 0; a zero product counts as EPS)
struct KlDivCsr {
    enum { NS = 1, NV = 1 };
    static __device__ __forceinline__ void add(const float *tw, float d, double *acc) {
        const float v = tw[0];
        if (v > 0.f) acc[0] += (double)(v * logf(v / (d > 0.f ? d : CMF_MU_EPS))) - (double)v;
    }
};
template <int GL>
__global__ __launch_bounds__(256) void kl_div_csr_kernel(PairCsrView T, const float *A, const float *B, int kp, double *partials) {
    csr_reduce<GL, KlDivCsr>(T, A, B, kp, partials);
}

// ------------------------------------------------------------------ column sums and the update
// part[b][col] = sum of F[r][col] over the rows of chunk b: thread (sub, col) walks every (256 / kp)-th row, the subs are added in order
template <typename ACC>
__global__ __launch_bounds__(256) void kl_colsum_partial_kernel(const float *F, int kp, int64_t rows, int64_t chunk, ACC *part) {
    __shared__ ACC red[256];
    const int tid = threadIdx.x, col = tid % kp, sub = tid / kp, nsub = 256 / kp;
    const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = min(rows, r0 + chunk);
    ACC s = 0;
    for (int64_t r = r0 + sub; r < r1; r += nsub) s += (ACC)F[r * kp + col];
    red[tid] = s;
    __syncthreads();
    if (tid < kp) {
        ACC t = 0;
        for (int u = 0; u < nsub; ++u) t += red[u * kp + tid];
        part[(int64_t)blockIdx.x * kp + tid] = t;
    }
}
template <typename ACC>
__global__ __launch_bounds__(256) void kl_colsum_reduce_kernel(const ACC *part, int kp, int nblk, ACC *out) {
    const int col = threadIdx.x;
    if (col >= kp) return;
    ACC s = 0;
    for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * kp + col];
    out[col] = s;
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx)
#ifdef CMF_KLMU_HOST

static bool kl_native(const cmf_ctx *c, int which) { return c->sparse[which] && !(which == 0 ? c->X : c->Y); }

// pp_plan's share rule (option "kl_split" forces the count); S = 1 for a native CSR relation
static void kl_plan(const cmf_ctx *c, const PairPass &ps, int64_t *S, int64_t *per) { pp_plan(c, ps, c->opt_kl_split, kl_native(c, ps.which), S, per); }

static int64_t kl_colsum_blocks(int64_t rows) { return (rows + 511) / 512; }

// scratch of a step: the numerator slabs of the widest sweep + column-sum partials and sums
static size_t kl_small_bytes(const cmf_ctx *c) {
    const int64_t rmax = std::max(c->mp + c->pp, c->dp);
    return (size_t)(2 * kl_colsum_blocks(rmax) + 4) * c->kp * sizeof(double) + 64;
}
static size_t kl_slab_bytes(const cmf_ctx *c, int mask) {
    int64_t S, per, S2;
    size_t need = 0;
    const size_t kp4 = (size_t)c->kp * sizeof(float);
    if (mask & CMF_UPD_V) { kl_plan(c, PP_VX, &S, &per); kl_plan(c, PP_VY, &S2, &per); need = std::max(need, (size_t)(S + S2) * c->dp * kp4); }
    if (mask & CMF_UPD_U) { kl_plan(c, PP_U, &S, &per); need = std::max(need, (size_t)S * c->mp * kp4); }
    if (mask & CMF_UPD_Z) { kl_plan(c, PP_Z, &S, &per); need = std::max(need, (size_t)S * c->pp * kp4); }
    return need;
}

static int kl_check(cmf_ctx *c, const char *what) {
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: k_pad = %d (n_components above 256) is not supported by the Kullback-Leibler passes", what, c->kp);
    return CMF_OK;
}

// numerator slabs of one pass into `slabs` (slab stride = rows_pad * k_pad); *nslab = how many it wrote
static int kl_quotient_pass(cmf_ctx *c, const PairPass &ps, float *slabs, int *nslab) {
    if (!have_data(c, ps.which)) return fail(CMF_EINVAL, "cmf_mu_kl_step: %s has not been set", ps.which == 0 ? "X" : "Y");
    if (kl_native(c, ps.which)) {
        const int64_t rows_pad = c->frows_pad[ps.fa];
        const float *A = c->F[ps.fa], *B = c->F[ps.fb];
        const CsrDev &M = c->sp[ps.which][ps.trans ? 1 : 0];
        CsrView v{M.indptr, M.idx, M.val, M.rows};
        Timed tm(c, CMF_K_KLMU, 4.0 * (double)M.nnz * (double)c->kp);
        const int gl = c->kp / 4, rpw = 64 / gl;
        const unsigned blocks = (unsigned)(rows_pad / (4 * rpw));
        with_kp(c->kp, [&](auto kp) {
            hipLaunchKernelGGL((kl_quotient_csr_kernel<decltype(kp)::value / 4>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, slabs);
        });
        HIPCHK(hipGetLastError());
        *nslab = 1;
        return CMF_OK;
    }
    int64_t S, per;
    kl_plan(c, ps, &S, &per);
    PairPassArgs a = pp_args(c, ps, per);
    a.img0 = ps.which == 0 ? c->X : c->Y;
    a.out = slabs;
    Timed tm(c, CMF_K_KLMU, 4.0 * (double)c->frows[ps.fa] * (double)c->frows[ps.fb] * (double)c->k);
    CHK(pp_launch_pass<KlQuotient>(c, ps, a, S));
    *nslab = (int)S;
    return CMF_OK;
}

// out[k_pad] = column sums of F (rows x k_pad); `part` holds the partials
template <typename ACC>
static int kl_colsum(cmf_ctx *c, const float *F, int64_t rows, ACC *part, ACC *out) {
    const int64_t nblk = kl_colsum_blocks(rows);
    Timed tm(c, CMF_K_ELEMWISE);
    hipLaunchKernelGGL((kl_colsum_partial_kernel<ACC>), dim3((unsigned)nblk), dim3(256), 0, c->stream, F, c->kp, rows, (int64_t)512, part);
    hipLaunchKernelGGL((kl_colsum_reduce_kernel<ACC>), dim3(1), dim3(256), 0, c->stream, (const ACC *)part, c->kp, (int)nblk, out);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

extern "C" int cmf_mu_kl_step(cmf_ctx *c, double l1, double l2, int mask) {
    NEED_PROBLEM(c);
    CHK(kl_check(c, "cmf_mu_kl_step"));
    if ((mask & (CMF_UPD_U | CMF_UPD_V)) && !have_data(c, 0)) return fail(CMF_EINVAL, "cmf_mu_kl_step: X has not been set");
    if ((mask & (CMF_UPD_Z | CMF_UPD_V)) && !have_data(c, 1)) return fail(CMF_EINVAL, "cmf_mu_kl_step: Y has not been set");
    DeviceGuard dg(c->device);
    CHK(ensure_scratch(c, c->kl_slab, kl_slab_bytes(c, mask)));
    CHK(ensure_scratch(c, c->kl_small, kl_small_bytes(c)));
    float *slabs = (float *)c->kl_slab.p;
    float *cs = (float *)c->kl_small.p, *cpart = cs + c->kp;
    int n1 = 0, n2 = 0;
    if (mask & CMF_UPD_V) { // V <- V .* [Q(X,U,V)^T U + Q(Y,V,Z) Z] ./ reg(colsum U + colsum Z, V): U and Z are one stacked block
        CHK(kl_quotient_pass(c, PP_VX, slabs, &n1));
        CHK(kl_quotient_pass(c, PP_VY, slabs + (int64_t)n1 * c->dp * c->kp, &n2));
        CHK(kl_colsum<float>(c, c->F[CMF_U], c->mp + c->pp, cpart, cs));
        CHK(pp_update<DEN_COLSUM>(c, CMF_V, slabs, cs, n1 + n2, l1, l2));
    }
    if (mask & (CMF_UPD_U | CMF_UPD_Z)) CHK(kl_colsum<float>(c, c->F[CMF_V], c->dp, cpart, cs));
    if (mask & CMF_UPD_U) {
        CHK(kl_quotient_pass(c, PP_U, slabs, &n1));
        CHK(pp_update<DEN_COLSUM>(c, CMF_U, slabs, cs, n1, l1, l2));
    }
    if (mask & CMF_UPD_Z) {
        CHK(kl_quotient_pass(c, PP_Z, slabs, &n1));
        CHK(pp_update<DEN_COLSUM>(c, CMF_Z, slabs, cs, n1, l1, l2));
    }
    return CMF_OK;
}

// D(T || A B^T) of one side into *out
static int kl_divergence_side(cmf_ctx *c, int which, double *out) {
    const PairPass ps = which == 0 ? PP_U : PP_VY;
    const float *A = c->F[ps.fa], *B = c->F[ps.fb];
    double *small = (double *)c->kl_small.p; // [0] the sum, [1 .. 1 + 2 k_pad) column sums, then partials
    if (kl_native(c, which)) { // sum over the stored entries + sum of all s = colsum(A) . colsum(B): no dense image
        const CsrDev &M = c->sp[which][0];
        PairCsrView v{M.indptr, M.idx, nullptr, nullptr, M.val, M.rows};
        CHK(ensure_scratch(c, c->kl_part, (size_t)csr_reduce_blocks(c, M.rows) * sizeof(double)));
        {
            Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
            double *part = (double *)c->kl_part.p;
            CHK(csr_launch_reduce<1>(c, M.rows, part, small, [&](auto gl, dim3 grid) {
                hipLaunchKernelGGL((kl_div_csr_kernel<decltype(gl)::value>), grid, dim3(256), 0, c->stream, v, A, B, c->kp, part);
            }));
        }
        double *cpart = small + 1 + 2 * c->kp;
        CHK(kl_colsum<double>(c, A, c->frows_pad[ps.fa], cpart, small + 1));
        CHK(kl_colsum<double>(c, B, c->frows_pad[ps.fb], cpart, small + 1 + c->kp));
        std::vector<double> h(1 + 2 * (size_t)c->kp);
        HIPCHK(hipMemcpyAsync(h.data(), small, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        double d = h[0];
        for (int t = 0; t < c->kp; ++t) d += h[1 + t] * h[1 + c->kp + t];
        *out = d;
        return CMF_OK;
    }
    int64_t S, per;
    kl_plan(c, ps, &S, &per);
    const dim3 grid = pp_grid(c, ps, S);
    CHK(ensure_scratch(c, c->kl_part, (size_t)grid.x * grid.y * sizeof(double)));
    PairPassArgs a = pp_args(c, ps, per);
    a.img0 = which == 0 ? c->X : c->Y;
    a.part = (double *)c->kl_part.p;
    {
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)c->frows[ps.fa] * (double)c->frows[ps.fb] * (double)c->k);
        CHK(pp_launch_reduce<KlDivergence>(c, ps, a, S, small));
    }
    HIPCHK(hipMemcpyAsync(out, small, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_kl_divergence(cmf_ctx *c, double *dx, double *dy) {
    NEED_PROBLEM(c);
    CHK(kl_check(c, "cmf_kl_divergence"));
    if (dx && !have_data(c, 0)) return fail(CMF_EINVAL, "cmf_kl_divergence: X has not been set");
    if (dy && !have_data(c, 1)) return fail(CMF_EINVAL, "cmf_kl_divergence: Y has not been set");
    DeviceGuard dg(c->device);
    CHK(ensure_scratch(c, c->kl_small, kl_small_bytes(c)));
    if (dx) CHK(kl_divergence_side(c, 0, dx));
    if (dy) CHK(kl_divergence_side(c, 1, dy));
    return CMF_OK;
}

extern "C" int cmf_mu_kl_layout(cmf_ctx *c, int64_t *out4) {
    NEED_PROBLEM(c);
    if (!out4) return fail(CMF_EINVAL, "cmf_mu_kl_layout: null output");
    CHK(kl_check(c, "cmf_mu_kl_layout"));
    int64_t S, S2, per;
    kl_plan(c, PP_U, &S, &per);
    out4[0] = S;
    kl_plan(c, PP_VX, &S, &per);
    kl_plan(c, PP_VY, &S2, &per);
    out4[1] = std::max(S, S2);
    kl_plan(c, PP_Z, &S, &per);
    out4[2] = S;
    out4[3] = (int64_t)(kl_slab_bytes(c, CMF_UPD_U | CMF_UPD_V | CMF_UPD_Z) + kl_small_bytes(c));
    return CMF_OK;
}
#endif // CMF_KLMU_HOST
