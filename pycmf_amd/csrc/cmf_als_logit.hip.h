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
//                          stored entries of one row (the walk of cmf_als_entries.hip.h, one gather in flight), s in float32, the
//                          terms added in float64 per lane group, the groups in group order; the pieces are added in piece order
//                          behind the kernel boundary (als_piece_sum_kernel, one thread).
// No atomics anywhere, vector stores only: a repeated call from the same state is bit-identical.
#pragma once
#include "cmf_als_entries.hip.h"

namespace cmfk {

struct AlsLogitLossArgs : AlsEntryArgs {
    const float *tv, *wv;
    double *part;            // [pieces]
};

struct AlsLogitLossBody {
    const AlsLogitLossArgs &g;
    const float *tv, *wv;    // of the piece
    float t[1], w[1];
    double sum[1] = {0.0};
    __device__ __forceinline__ void begin(int64_t beg) { tv = g.tv + beg, wv = g.wv + beg; }
    __device__ __forceinline__ void load(int j, int q, int32_t) {
        t[j] = tv[q];
        w[j] = wv[q];
    }
    __device__ __forceinline__ void use(int j, float s, int, bool real) {
#pragma clang fp contract(off)
        const float term = w[j] * ((fmaxf(s, 0.f) + log1pf(expf(-fabsf(s)))) - t[j] * s);
        if (real) sum[0] += (double)term;
    }
};

template <int GL>
__global__ __launch_bounds__(256) void als_logit_loss_kernel(AlsLogitLossArgs g) {
    AlsLogitLossBody body{g};
    als_entry_walk<GL, 1>(g, body);
    als_group_reduce<GL>(body.sum, g.part + blockIdx.x);
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als_bg.hip.h)
#ifdef CMF_ALS_HOST
static bool als_logit_rel(const cmf_ctx *c, int which) { return c->rel_loss[which] == CMF_LOSS_LOGISTIC; }
// A logistic relation is reweighted in one of two places: inside als_normal_kernel<KP, true> (FUSED, the default: the formed routes
// only), or by a pass of its own in front of every sweep (PASSED, cmf_set_logit_pass, cmf_als_reweight.hip.h), after which every
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
    CHK(als_entry_pieces(c, which, 0, "cmf_als_logistic_loss"));
    const AlsReweight &h = c->als_reweight[which];
    cmfk::AlsLogitLossArgs a{};
    als_entry_args(c, which, 0, h.pieces[0], a);
    a.tv = M.tv; a.wv = M.wv;
    return als_pieces_loss(c, h.npieces[0], M.nnz, [&](double *part) {
        a.part = part;
        const dim3 grid((unsigned)h.npieces[0]), block(256);
        ALS_LAUNCH_GL(c, als_logit_loss_kernel, grid, block, 0, c->stream, a);
    }, out);
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
