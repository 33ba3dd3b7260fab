// cmf_als_reweight.hip.h -- the losses of the ALS solver that are fitted by REWEIGHTING: with the residual or score under the CURRENT
// row a majoriser of the loss makes row i the row problem of cmf_als.hip.h under effective weights hw in place of w and effective
// products hp in place of w t.  So no row kernel changes: ONE pass of its own in front of every sweep writes hw (and hp) per stored
// entry of the image the sweep reads, and the row routes read them through als_side_weights / als_side_targets while the sweep has
// them bound (AlsReweightGuard).  Every route starts at the current row and never raises its quadratic, so the exact,
// coordinate-descent, CG, projected-CG and dual rows all lower the true objective.  A relation takes one of the two:
//
// A HUBER loss (cmf_set_huber_delta, d > 0) on a relation with CSR weights, next to the other relation as it is:
//   sum_O w rho_d(t - a . b),      rho_d(r) = 1/2 r^2 if |r| <= d,  d (|r| - 1/2 d) otherwise
// The half-quadratic majoriser
//   rho_d(r) <= rho_d(r0) + 1/2 omega(r0) (r^2 - r0^2),      omega(r) = 1 if |r| <= d,  d / |r| otherwise,      tight at r = +-r0
// gives
//   r = tt - s,   omega = |r| <= d ? 1 : d / |r|,   hw = w omega,   hp = pp omega
// (tt: the adjusted targets under biases, else t; pp: bp under biases, else pv = w t; s = a . b in float32).  omega == 1 leaves w and
// pp with their bits: under a delta no residual reaches, every route gives the bits it gives without one.
//
// The LOGISTIC loss of cmf_als_logit.hip.h on every route (cmf_set_logit_pass, opt-in per relation).  With xi the score under the
// current row the Jaakkola-Jordan bound gives
//   hw = w kappa(xi),      hp = w t - 1/2 w,      kappa(s) = |s| < 1e-4 ? 1/4 : tanh(s / 2) / (2 s)
// hp does not depend on the factors: it is written once, when the arrays are built.  Without the flag a logistic relation is
// reweighted inside als_normal_kernel<KP, true>, which costs less on the formed routes and is all the other routes refuse.
//
// The kernels are the walk of cmf_als_entries.hip.h over pieces of at most 2048 stored entries, FOUR gathered rows in flight per lane
// group (indices, then the rows, then the body's scalars):
//   als_huber_pass_kernel<GL, LOSS>  LOSS = false: hw and hp leave through lane 0 of the group; an entry past the piece's end writes
//                          nothing.  LOSS = true: sum w rho_d(r), the terms in float32, added in float64 per lane group, the groups
//                          in group order; the pieces in piece order behind the kernel boundary (als_piece_sum_kernel).
//   als_logit_pass_kernel<GL>  hw leaves through lane 0 of the group.  It reads idx, w and the gathered rows and writes hw:
//                          nnz (4 k_pad + 12) bytes.
//   als_logit_hp_kernel    hp = pv - 0.5f w, elementwise, once per image and bound pattern.
// No atomics, vector stores only: a repeated call from the same state is bit-identical.
#pragma once
#include "cmf_als_entries.hip.h"

namespace cmfk {

enum { ALS_REWEIGHT_FLIGHT = 4 };   // gathered rows in flight per lane group

struct AlsHuberArgs : AlsEntryArgs {
    const float *tt, *wv, *pp;   // targets (adjusted under biases), weights, products w tt
    float delta;
    float *hw, *hp;              // LOSS = false: [nnz] each
    double *part;                // LOSS = true: [pieces]
};

template <int GL, bool LOSS>
struct AlsHuberBody {
    const AlsHuberArgs &g;
    const bool lane0 = threadIdx.x % GL == 0;
    int64_t beg;                 // the piece's first entry; tt, wv: of the piece
    const float *tt, *wv;
    float t[ALS_REWEIGHT_FLIGHT], w[ALS_REWEIGHT_FLIGHT];
    double sum[1] = {0.0};
    __device__ __forceinline__ void begin(int64_t first) { beg = first, tt = g.tt + first, wv = g.wv + first; }
    __device__ __forceinline__ void load(int j, int q, int32_t) {
        t[j] = tt[q];
        w[j] = wv[q];
    }
    __device__ __forceinline__ void use(int j, float s, int e, bool real) {
#pragma clang fp contract(off)
        const float d = g.delta, r = t[j] - s, ar = fabsf(r);
        if constexpr (LOSS) {
            const float term = w[j] * (ar <= d ? 0.5f * (r * r) : d * (ar - 0.5f * d));
            if (lane0 && real) sum[0] += (double)term;   // (every lane of the group holds the term; lane 0 keeps the sum)
        } else {
            const float om = ar <= d ? 1.0f : d / ar;
            if (lane0 && real) {
                g.hw[beg + e] = w[j] * om;
                g.hp[beg + e] = g.pp[beg + e] * om;
            }
        }
    }
};

template <int GL, bool LOSS>
__global__ __launch_bounds__(256) void als_huber_pass_kernel(AlsHuberArgs g) {
    AlsHuberBody<GL, LOSS> body{g};
    als_entry_walk<GL, ALS_REWEIGHT_FLIGHT>(g, body);
    if constexpr (LOSS) als_group_reduce<GL>(body.sum, g.part + blockIdx.x);
}

struct AlsLogitPassArgs : AlsEntryArgs {
    const float *wv;
    float *hw;                   // [nnz]
};

template <int GL>
struct AlsLogitPassBody {
    const AlsLogitPassArgs &g;
    const bool lane0 = threadIdx.x % GL == 0;
    const float *wv;             // of the piece, like hw
    float *hw;
    float w[ALS_REWEIGHT_FLIGHT];
    __device__ __forceinline__ void begin(int64_t beg) { wv = g.wv + beg, hw = g.hw + beg; }
    __device__ __forceinline__ void load(int j, int q, int32_t) { w[j] = wv[q]; }
    __device__ __forceinline__ void use(int j, float s, int e, bool real) {
#pragma clang fp contract(off)
        const float kap = fabsf(s) < 1e-4f ? 0.25f : tanhf(0.5f * s) / (2.0f * s);   // (als_logit_kappa's expression)
        if (lane0 && real) hw[e] = w[j] * kap;
    }
};

template <int GL>
__global__ __launch_bounds__(256) void als_logit_pass_kernel(AlsLogitPassArgs g) {
    AlsLogitPassBody<GL> body{g};
    als_entry_walk<GL, ALS_REWEIGHT_FLIGHT>(g, body);
}

__global__ void als_logit_hp_kernel(const float *pv, const float *wv, int64_t n, float *hp) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) hp[i] = pv[i] - 0.5f * wv[i];
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als_logit.hip.h)
#ifdef CMF_ALS_HOST

static bool als_huber_rel(const cmf_ctx *c, int which) { return c->als_reweight[which].delta > 0.0; }

// What a step, a row entry or a Huber entry point that reads Huber relation `which` cannot do: the relation must be observed (CSR
// weights), without a background weight and without a logistic loss.
static int als_huber_rel_ok(cmf_ctx *c, const char *what, int which) {
    if (!als_huber_rel(c, which)) return CMF_OK;
    const char *nm = which == 0 ? "X" : "Y";
    if (c->wm_kind[which] != WM_CSR)
        return fail(CMF_EUNSUPPORTED, "%s: %s has a Huber loss (cmf_set_huber_delta) and no CSR weights bound; the Huber loss is built over an observed "
                                      "pattern only (cmf_set_weighted_csr), not over every cell", what, nm);
    if (c->wm_bg[which] > 0.0)
        return fail(CMF_EUNSUPPORTED, "%s: %s has a Huber loss and a background weight; the Huber loss over the cells outside the pattern is not built", what, nm);
    if (als_logit_rel(c, which))
        return fail(CMF_EUNSUPPORTED, "%s: %s has a Huber loss and a logistic loss; a relation takes one of them: clear one with cmf_set_huber_delta(ctx, %d, 0) "
                                      "or cmf_set_relation_loss(ctx, %d, CMF_LOSS_FROBENIUS)", what, nm, which, which);
    return CMF_OK;
}
// ... for the relations X (U, V sweeps) / Y (V, Z sweeps) a step with this mask reads
static int als_huber_check(cmf_ctx *c, const char *what, int mask) {
    if (mask & (CMF_UPD_U | CMF_UPD_V)) CHK(als_huber_rel_ok(c, what, 0));
    if (mask & (CMF_UPD_Z | CMF_UPD_V)) CHK(als_huber_rel_ok(c, what, 1));
    return CMF_OK;
}

// What a pass of this kind needs beyond the images and their piece lists: hw / hp of both images and, HUBER, t in the stored order of
// the transpose; LOGIT, hp of both images, which no sweep changes.  Built once per bound pattern (als_reweight_free drops it with the
// weights).  A relation takes a Huber loss or a logistic one, never both at once: what the other kind built is dropped first.
static int als_reweight_build(cmf_ctx *c, int which, AlsReweightKind kind) {
    AlsReweight &h = c->als_reweight[which];
    const int64_t nnz = c->wm_sp[which][0].nnz;
    const size_t vbytes = std::max<size_t>(16, (size_t)nnz * sizeof(float));
    if (kind == ALS_REWEIGHT_HUBER) {
        std::vector<float> tt;
        CHK(als_transposed_targets(c, which, tt));
        CHK(dev_alloc(c, (void **)&h.tt1, vbytes, false));
        if (nnz) HIPCHK(hipMemcpyAsync(h.tt1, tt.data(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream)); // the host vector may go
    }
    for (int t = 0; t < 2; ++t) {
        WCsrDev &M = c->wm_sp[which][t];
        CHK(dev_alloc(c, (void **)&M.hw, vbytes));
        CHK(dev_alloc(c, (void **)&M.hp, vbytes));
        CHK(als_entry_pieces(c, which, t, "the Huber pass"));
        if (kind == ALS_REWEIGHT_LOGIT) CHK(launch_ew(c, cmfk::als_logit_hp_kernel, M.nnz, (const float *)M.pv, (const float *)M.wv, M.nnz, M.hp));
    }
    return CMF_OK;
}
static int als_reweight_ensure(cmf_ctx *c, int which, AlsReweightKind kind) {
    AlsReweight &h = c->als_reweight[which];
    if (h.kind == kind) return CMF_OK;
    if (h.kind != ALS_REWEIGHT_NONE) {
        HIPCHK(hipStreamSynchronize(c->stream));
        als_reweight_free(c, which);
    }
    const int rc = als_reweight_build(c, which, kind);
    if (rc != CMF_OK) {
        (void)hipStreamSynchronize(c->stream);
        als_reweight_free(c, which);
        return rc;
    }
    h.kind = kind;
    return CMF_OK;
}

// the arguments of a Huber pass over image t of relation `which` at the current factors (and, under biases, the current adjusted targets)
static int als_huber_args(cmf_ctx *c, int which, int t, cmfk::AlsHuberArgs &a) {
    CHK(als_reweight_ensure(c, which, ALS_REWEIGHT_HUBER));
    CHK(als_bias_refresh(c, which));   // (written when the biases last changed: nothing to do)
    const AlsReweight &h = c->als_reweight[which];
    const WCsrDev &M = c->wm_sp[which][t];
    a = cmfk::AlsHuberArgs{};
    als_entry_args(c, which, t, h.pieces[t], a);
    a.tt = M.bt ? M.bt : (t == 0 ? M.tv : h.tt1);
    a.wv = M.wv;
    a.pp = M.bp ? M.bp : M.pv;
    a.delta = (float)h.delta;
    a.hw = M.hw;
    a.hp = M.hp;
    return CMF_OK;
}

// hw, hp of image t of Huber relation `which` from the current factors
static int als_huber_refresh(cmf_ctx *c, int which, int t) {
    cmfk::AlsHuberArgs a;
    CHK(als_huber_args(c, which, t, a));
    const int64_t np = c->als_reweight[which].npieces[t];
    if (np <= 0) return CMF_OK;
    Timed tm(c, CMF_K_KLMU, 2.0 * (double)c->wm_sp[which][t].nnz * (double)c->kp);
    const dim3 grid((unsigned)np), block(256);
    ALS_LAUNCH_GL_T(c, als_huber_pass_kernel, false, grid, block, 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// sum_O w rho_d(tt - a . b) of one Huber relation into *out
static int als_huber_loss_side(cmf_ctx *c, int which, double *out) {
    cmfk::AlsHuberArgs a;
    CHK(als_huber_args(c, which, 0, a));
    const int64_t np = c->als_reweight[which].npieces[0];
    *out = 0.0;
    if (np <= 0) return CMF_OK;
    return als_pieces_loss(c, np, c->wm_sp[which][0].nnz, [&](double *part) {
        a.part = part;
        const dim3 grid((unsigned)np), block(256);
        ALS_LAUNCH_GL_T(c, als_huber_pass_kernel, true, grid, block, 0, c->stream, a);
    }, out);
}

// hw of image t of the passed logistic relation `which` from the current factors
static int als_logit_pass_refresh(cmf_ctx *c, int which, int t) {
    CHK(als_reweight_ensure(c, which, ALS_REWEIGHT_LOGIT));
    const AlsReweight &h = c->als_reweight[which];
    const WCsrDev &M = c->wm_sp[which][t];
    const int64_t np = h.npieces[t];
    if (np <= 0) return CMF_OK;
    cmfk::AlsLogitPassArgs a{};
    als_entry_args(c, which, t, h.pieces[t], a);
    a.wv = M.wv;
    a.hw = M.hw;
    Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
    const dim3 grid((unsigned)np), block(256);
    ALS_LAUNCH_GL(c, als_logit_pass_kernel, grid, block, 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// The reweighted sides of one sweep, bound for its duration: bind() refreshes hw / hp of every Huber or passed-logistic image the
// sweep reads, in the sweep's orientation, from the current factors, and als_side_weights / als_side_targets return them until the
// scope ends.  Nothing outside a sweep ever sees them: the residual, the bias targets and the losses read the images as they were
// bound.
struct AlsReweightGuard {
    cmf_ctx *const c;
    WCsrDev *bound[2] = {nullptr, nullptr};
    explicit AlsReweightGuard(cmf_ctx *ctx) : c(ctx) {}
    int bind(const AlsSweep &sw) {
        for (int s = 0; s < sw.nrel; ++s) {
            const AlsRel &r = sw.rel[s];
            if (!sw.observed[s]) continue;
            if (als_huber_rel(c, r.which)) CHK(als_huber_refresh(c, r.which, r.t));
            else if (als_logit_passed(c, r.which)) CHK(als_logit_pass_refresh(c, r.which, r.t));
            else continue;
            bound[s] = &c->wm_sp[r.which][r.t];
            bound[s]->hbound = true;
        }
        return CMF_OK;
    }
    ~AlsReweightGuard() {
        for (int s = 0; s < 2; ++s)
            if (bound[s]) bound[s]->hbound = false;
    }
    AlsReweightGuard(const AlsReweightGuard &) = delete;
    AlsReweightGuard &operator=(const AlsReweightGuard &) = delete;
};

static int als_huber_which_ok(const char *what, int which) {
    if (which != 0 && which != 1) return fail(CMF_EINVAL, "%s: which must be 0 (X) or 1 (Y)", what);
    return CMF_OK;
}

extern "C" int cmf_set_huber_delta(cmf_ctx *c, int which, double delta) {
    NEED_PROBLEM(c);
    CHK(als_huber_which_ok("cmf_set_huber_delta", which));
    const float df = (float)delta;
    if (!(delta >= 0.0) || !std::isfinite(delta) || !std::isfinite(df) || (delta > 0.0 && !(df > 0.f)))
        return fail(CMF_EINVAL, "cmf_set_huber_delta: delta must be finite and > 0 (in float32), or 0 for no Huber loss, got %g", delta);
    DeviceGuard dg(c->device);
    if (delta == 0.0) {
        HIPCHK(hipStreamSynchronize(c->stream));
        als_reweight_free(c, which);
    }
    c->als_reweight[which].delta = (double)df;
    return CMF_OK;
}

extern "C" int cmf_get_huber_delta(cmf_ctx *c, int which, double *delta) {
    NEED_PROBLEM(c);
    CHK(als_huber_which_ok("cmf_get_huber_delta", which));
    if (!delta) return fail(CMF_EINVAL, "cmf_get_huber_delta: null output");
    *delta = c->als_reweight[which].delta;
    return CMF_OK;
}

extern "C" int cmf_als_huber_loss(cmf_ctx *c, double *lx, double *ly) {
    NEED_PROBLEM(c);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_als_huber_loss: n_components <= 256 only (k_pad = %d)", c->kp);
    double *want[2] = {lx, ly};
    for (int w = 0; w < 2; ++w)
        if (want[w]) CHK(als_huber_rel_ok(c, "cmf_als_huber_loss", w));
    DeviceGuard dg(c->device);
    for (int w = 0; w < 2; ++w) {
        if (!want[w]) continue;
        *want[w] = 0.0;
        if (als_huber_rel(c, w)) CHK(als_huber_loss_side(c, w, want[w]));
    }
    return CMF_OK;
}

extern "C" int cmf_set_logit_pass(cmf_ctx *c, int which, int enable) {
    NEED_PROBLEM(c);
    CHK(als_huber_which_ok("cmf_set_logit_pass", which));
    if (!enable && c->als_reweight[which].kind == ALS_REWEIGHT_LOGIT) {   // what the pass built for the pattern goes with the flag
        DeviceGuard dg(c->device);
        HIPCHK(hipStreamSynchronize(c->stream));
        als_reweight_free(c, which);
    }
    c->als_logit_pass[which] = enable != 0;
    return CMF_OK;
}

extern "C" int cmf_get_logit_pass(cmf_ctx *c, int which, int *enabled) {
    NEED_PROBLEM(c);
    CHK(als_huber_which_ok("cmf_get_logit_pass", which));
    if (!enabled) return fail(CMF_EINVAL, "cmf_get_logit_pass: null output");
    *enabled = c->als_logit_pass[which] ? 1 : 0;
    return CMF_OK;
}

// The test entries: hw and hp of image t (0 the pattern, 1 its transpose) of a Huber / a passed logistic relation at the current
// factors; nnz: the entries the caller's buffers hold, which must be the stored entries of the pattern.  The checks both share:
static int als_weights_args_ok(cmf_ctx *c, const char *what, int which, int t) {
    CHK(als_huber_which_ok(what, which));
    if (t != 0 && t != 1) return fail(CMF_EINVAL, "%s: the image must be 0 (the pattern) or 1 (its transpose)", what);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: n_components <= 256 only (k_pad = %d)", what, c->kp);
    return CMF_OK;
}
static int als_weights_nnz_ok(cmf_ctx *c, const char *what, int which, int t, int64_t nnz) {
    const WCsrDev &M = c->wm_sp[which][t];
    if (nnz != M.nnz) return fail(CMF_EINVAL, "%s: the caller's buffers hold %lld entries, the pattern stores %lld", what, (long long)nnz, (long long)M.nnz);
    return CMF_OK;
}

extern "C" int cmf_als_huber_weights(cmf_ctx *c, int which, int t, int64_t nnz, float *w_eff, float *p_eff) {
    NEED_PROBLEM(c);
    const char *what = "cmf_als_huber_weights";
    CHK(als_weights_args_ok(c, what, which, t));
    if (!als_huber_rel(c, which)) return fail(CMF_EINVAL, "%s: %s has no Huber loss (cmf_set_huber_delta first)", what, which == 0 ? "X" : "Y");
    CHK(als_huber_rel_ok(c, what, which));
    CHK(als_weights_nnz_ok(c, what, which, t, nnz));
    DeviceGuard dg(c->device);
    CHK(als_huber_refresh(c, which, t));
    return als_weights_out(c, c->wm_sp[which][t], w_eff, p_eff);
}

extern "C" int cmf_als_logit_weights(cmf_ctx *c, int which, int t, int64_t nnz, float *w_eff, float *p_eff) {
    NEED_PROBLEM(c);
    const char *what = "cmf_als_logit_weights";
    CHK(als_weights_args_ok(c, what, which, t));
    const char *nm = which == 0 ? "X" : "Y";
    if (!als_logit_rel(c, which)) return fail(CMF_EINVAL, "%s: %s has no logistic loss (cmf_set_relation_loss first)", what, nm);
    if (!c->als_logit_pass[which]) return fail(CMF_EINVAL, "%s: %s is reweighted inside the normal-equation kernel (cmf_set_logit_pass first)", what, nm);
    CHK(als_logit_check(c, what, which == 0 ? CMF_UPD_U : CMF_UPD_Z));
    CHK(als_huber_rel_ok(c, what, which));
    CHK(als_weights_nnz_ok(c, what, which, t, nnz));
    DeviceGuard dg(c->device);
    CHK(als_logit_pass_refresh(c, which, t));
    return als_weights_out(c, c->wm_sp[which][t], w_eff, p_eff);
}

#endif // CMF_ALS_HOST
