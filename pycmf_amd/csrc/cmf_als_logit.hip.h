// cmf_als_logit.hip.h -- a logistic loss for the ALS solver: a relation with CSR weights may be fitted as sigmoid(a . b), its term of
// the objective the weighted cross-entropy over the stored pattern
//   sum_O w [softplus(a . b) - t (a . b)],      t in [0, 1], w >= 0,
// next to Frobenius relations (observed or full) in the same sweep.  The Jaakkola-Jordan bound of the logistic loss is quadratic in
// the score s = a . b and tight at s = +-xi:
//   w [softplus(s) - t s]  <=  1/2 w kappa(xi) s^2 - w (t - 1/2) s + const,      kappa(xi) = tanh(xi / 2) / (2 xi) in (0, 1/4].
// With xi the score under the CURRENT row f_i, the exact minimiser of the bound for row i solves the system of cmf_als.hip.h with
// w kappa in place of w and w (t - 1/2) in place of w t:
//   (sum_{e in O_i} w_e kappa_e b_e b_e^T + S + l2 I) f_i = sum_{e in O_i} w_e (t_e - 1/2) b_e + N_i
// (S, N of a full Frobenius side as there).  The bound touches the loss at the current row, so every row solve -- the Cholesky
// route, and the coordinate descent of als_nnls_kernel, which starts from the current row and never raises the quadratic -- lowers
// the true objective: monotone descent without a step size or a clamp, signed or non-negative (sweeps > 0).
//   als_normal_kernel<KP, true>  (cmf_als.hip.h) the normal-equation kernel with the current row in registers: the reweighting
//                          w kappa, w (t - 1/2) where a staged tile leaves them.  A sweep without a logistic relation launches the
//                          LG = false instance, which carries none of it.
//   als_logit_loss_kernel<GL>     sum_O w [max(s, 0) + log1p(exp(-|s|)) - t s]: one 256-thread workgroup per piece of at most 2048
//                          stored entries of one row (AlsBiasPiece, the lane layout of als_bias_piece_kernel), s in float32, the
//                          terms added in float64 per lane group, the groups in group order; the pieces are added in piece order
//                          behind the kernel boundary (als_logit_sum_kernel, one thread).
// No atomics anywhere, vector stores only: a repeated call from the same state is bit-identical.
#pragma once
#include "cmf_kernels.hip.h"   // (AlsBiasPiece: cmf_als_bias.hip.h, which cmf_api.hip includes before this file)

namespace cmfk {

struct AlsLogitLossArgs {
    const AlsBiasPiece *pieces;
    const int32_t *idx;
    const float *tv, *wv;
    const float *A, *B;      // the factor of the image's rows, the gathered factor; pitch kp
    int kp;
    double *part;            // [pieces]
};

template <int GL>
__global__ __launch_bounds__(256) void als_logit_loss_kernel(AlsLogitLossArgs g) {
#pragma clang fp contract(off)
    constexpr int NG = 256 / GL;
    const AlsBiasPiece pc = g.pieces[blockIdx.x];
    const int gl = threadIdx.x % GL, grp = threadIdx.x / GL;
    const f32x4 a = *reinterpret_cast<const f32x4 *>(g.A + (int64_t)pc.row * g.kp + 4 * gl);
    const int32_t *idx = g.idx + pc.beg;
    const float *tv = g.tv + pc.beg, *wv = g.wv + pc.beg;
    double sum = 0.0;
    // every group runs the same number of rounds (a round past the piece's end reads its last entry again and adds nothing)
    for (int base = 0; base < pc.len; base += NG) {
        const int e = base + grp, q = min(e, pc.len - 1);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(g.B + (int64_t)idx[q] * g.kp + 4 * gl);
        float s = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
        s = group_sum<GL>(s);
        const float term = wv[q] * ((fmaxf(s, 0.f) + log1pf(expf(-fabsf(s)))) - tv[q] * s);
        if (e < pc.len) sum += (double)term;
    }
    __shared__ double red[NG];
    if (gl == 0) red[grp] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = red[0];
        for (int q = 1; q < NG; ++q) v += red[q];
        g.part[blockIdx.x] = v;
    }
}

// the pieces in piece order
__global__ void als_logit_sum_kernel(const double *part, int64_t n, double *out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double v = 0.0;
    for (int64_t p = 0; p < n; ++p) v += part[p];
    *out = v;
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als_bg.hip.h)
#ifdef CMF_ALS_HOST
enum { ALS_LOGIT_LOSS_PIECE = 2048 };

static bool als_logit_rel(const cmf_ctx *c, int which) { return c->rel_loss[which] == CMF_LOSS_LOGISTIC; }
// A logistic relation is reweighted in one of two places: inside als_normal_kernel<KP, true> (FUSED, the default: the formed routes
// only), or by a pass of its own in front of every sweep (PASSED, cmf_set_logit_pass, cmf_als_logit_pass.hip.h), after which every
// route reads it as a Frobenius relation under w kappa and w (t - 1/2).  For routing and for the refusals of the routes without
// formed systems a passed relation is therefore not a logistic one.
static bool als_logit_passed(const cmf_ctx *c, int which) { return als_logit_rel(c, which) && c->als_logit_pass[which]; }
static bool als_logit_fused(const cmf_ctx *c, int which) { return als_logit_rel(c, which) && !c->als_logit_pass[which]; }

// does the sweep of factor f read a fused logistic relation?
static bool als_logit_sweep(const cmf_ctx *c, const AlsSweep &sw) {
    for (int s = 0; s < sw.nrel; ++s)
        if (als_logit_fused(c, sw.rel[s].which)) return true;
    return false;
}

// the relations X (U, V sweeps) / Y (V, Z sweeps) a step with this mask reads
static bool als_logit_swept(const cmf_ctx *c, int mask) {
    return ((mask & (CMF_UPD_U | CMF_UPD_V)) && als_logit_rel(c, 0)) || ((mask & (CMF_UPD_Z | CMF_UPD_V)) && als_logit_rel(c, 1));
}

// What a step that sweeps a logistic relation cannot do: the relation must be observed (CSR weights), without a background weight and
// without biases, fused or passed.  cg: the entry point asked for the conjugate-gradient route, which has no reweighting pass of its
// own: a fused relation is refused there.
static int als_logit_check(cmf_ctx *c, const char *what, int mask, bool cg = false) {
    for (int w = 0; w < 2; ++w) {
        const bool swept = w == 0 ? (mask & (CMF_UPD_U | CMF_UPD_V)) != 0 : (mask & (CMF_UPD_Z | CMF_UPD_V)) != 0;
        if (!swept || !als_logit_rel(c, w)) continue;
        const char *nm = w == 0 ? "X" : "Y";
        if (c->wm_kind[w] != WM_CSR)
            return fail(CMF_EUNSUPPORTED, "%s: %s has a logistic loss (cmf_set_relation_loss) and no CSR weights bound; the logistic loss is built over an "
                                          "observed pattern only (cmf_set_weighted_csr), not over every cell", what, nm);
        if (c->wm_bg[w] > 0.0)
            return fail(CMF_EUNSUPPORTED, "%s: %s has a logistic loss and a background weight; the logistic loss over the cells outside the pattern is not built", what, nm);
        if (c->als_bias[w].on) return fail(CMF_EUNSUPPORTED, "%s: %s has a logistic loss and biases; biases under a logit link are not built", what, nm);
        if (cg && als_logit_fused(c, w))
            return fail(CMF_EUNSUPPORTED, "%s: %s has a logistic loss; the conjugate-gradient rows have no reweighting pass: use cmf_als_step or cmf_als_nnls_step", what, nm);
    }
    return CMF_OK;
}

extern "C" int cmf_set_relation_loss(cmf_ctx *c, int which, int kind) {
    NEED_PROBLEM(c);
    if (which != 0 && which != 1) return fail(CMF_EINVAL, "cmf_set_relation_loss: which must be 0 (X) or 1 (Y)");
    if (kind != CMF_LOSS_FROBENIUS && kind != CMF_LOSS_LOGISTIC)
        return fail(CMF_EINVAL, "cmf_set_relation_loss: kind must be CMF_LOSS_FROBENIUS (0) or CMF_LOSS_LOGISTIC (1), got %d", kind);
    c->rel_loss[which] = kind;
    return CMF_OK;
}

extern "C" int cmf_get_relation_loss(cmf_ctx *c, int which, int *kind) {
    NEED_PROBLEM(c);
    if ((which != 0 && which != 1) || !kind) return fail(CMF_EINVAL, "cmf_get_relation_loss: which must be 0 (X) or 1 (Y) and the output non-null");
    *kind = c->rel_loss[which];
    return CMF_OK;
}

// sum_O w [softplus(s) - t s] of one logistic relation into *out
static int als_logit_loss_side(cmf_ctx *c, int which, double *out) {
    const WCsrDev &M = c->wm_sp[which][0];
    *out = 0.0;
    if (M.nnz <= 0) return CMF_OK;
    std::vector<int64_t> ip((size_t)M.rows + 1, 0);
    HIPCHK(hipMemcpyAsync(ip.data(), M.indptr, ip.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<cmfk::AlsBiasPiece> pieces;
    als_cut_rows(&ip, 1, M.rows, ALS_LOGIT_LOSS_PIECE, [&](int64_t r, int, int64_t beg, int32_t len) {
        pieces.push_back(cmfk::AlsBiasPiece{beg, len, (int32_t)r});
    });
    if ((int64_t)pieces.size() > INT32_MAX) return fail(CMF_EUNSUPPORTED, "cmf_als_logistic_loss: more than 2^31 - 1 pieces");
    const size_t pbytes = rup((int64_t)(pieces.size() * sizeof(cmfk::AlsBiasPiece)), 16);
    CHK(ensure_scratch(c, c->als_desc, pbytes));
    CHK(ensure_scratch(c, c->als_bias_part, (pieces.size() + 1) * sizeof(double)));
    HIPCHK(hipMemcpyAsync(c->als_desc.p, pieces.data(), pieces.size() * sizeof(cmfk::AlsBiasPiece), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vector may go
    cmfk::AlsLogitLossArgs a;
    a.pieces = (const cmfk::AlsBiasPiece *)c->als_desc.p;
    a.idx = M.idx; a.tv = M.tv; a.wv = M.wv;
    a.A = c->F[which == 0 ? CMF_U : CMF_V];
    a.B = c->F[which == 0 ? CMF_V : CMF_Z];
    a.kp = c->kp;
    a.part = (double *)c->als_bias_part.p;
    double *sum = a.part + pieces.size();
    {
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
        const dim3 grid((unsigned)pieces.size()), block(256);
        ALS_LAUNCH_GL(c, als_logit_loss_kernel, grid, block, 0, c->stream, a);
        hipLaunchKernelGGL(cmfk::als_logit_sum_kernel, dim3(1), dim3(64), 0, c->stream, (const double *)a.part, (int64_t)pieces.size(), sum);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_als_logistic_loss(cmf_ctx *c, double *lx, double *ly) {
    NEED_PROBLEM(c);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_als_logistic_loss: n_components <= 256 only (k_pad = %d)", c->kp);
    double *want[2] = {lx, ly};
    for (int w = 0; w < 2; ++w)
        if (want[w] && als_logit_rel(c, w)) CHK(als_logit_check(c, "cmf_als_logistic_loss", w == 0 ? CMF_UPD_U : CMF_UPD_Z));
    DeviceGuard dg(c->device);
    for (int w = 0; w < 2; ++w) {
        if (!want[w]) continue;
        *want[w] = 0.0;
        if (als_logit_rel(c, w)) CHK(als_logit_loss_side(c, w, want[w]));
    }
    return CMF_OK;
}

#endif // CMF_ALS_HOST
