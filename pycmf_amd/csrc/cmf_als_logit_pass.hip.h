// cmf_als_logit_pass.hip.h -- the logistic loss of the ALS solver (cmf_als_logit.hip.h) on every route, by a reweighting pass of its
// own in front of every sweep (cmf_set_logit_pass, opt-in per relation).  With xi the score under the CURRENT row the
// Jaakkola-Jordan bound makes the majoriser of row i the row problem of cmf_als.hip.h under
//   hw = w kappa(xi),      hp = w t - 1/2 w,      kappa(s) = |s| < 1e-4 ? 1/4 : tanh(s / 2) / (2 s)
// in place of w and w t.  hp does not depend on the factors: it is written once, when the arrays are built.  ONE pass per sweep writes
// hw per stored entry of the image the sweep reads, and the row routes read hw / hp through als_side_weights / als_side_targets
// while the sweep has them bound (AlsHuberGuard, cmf_als_huber.hip.h, whose arrays and piece lists this pass shares: a relation never
// carries a Huber delta and a logistic loss at once).  Every route starts at the current row and never raises its quadratic, so the
// exact, coordinate-descent, CG, projected-CG and dual rows all lower the true objective.  Without the flag a logistic relation is
// reweighted inside als_normal_kernel<KP, true>, which costs less on the formed routes and is all the other routes refuse.
//   als_logit_pass_kernel<GL>  the layout of als_huber_pass_kernel<GL, false>: one 256-thread workgroup per piece of at most 2048
//                          stored entries of one row (AlsBiasPiece), the row a in registers, GL = k_pad / 4 lanes x f32x4 per
//                          gathered row, the 256 / GL lane groups deal the piece's entries round-robin, FOUR gathered rows in flight
//                          per group (indices, then the rows, then w); hw leaves through lane 0 of the group; an entry past the
//                          piece's end reads the last one again and writes nothing.  It reads idx, w and the gathered rows and
//                          writes hw: nnz (4 k_pad + 12) bytes.
//   als_logit_hp_kernel    hp = pv - 0.5f w, elementwise, once per image and bound pattern.
// No atomics, no LDS, vector stores only: a repeated call from the same state is bit-identical.
#pragma once
#include "cmf_kernels.hip.h"   // (AlsBiasPiece: cmf_als_bias.hip.h; als_logit_kappa: cmf_als.hip.h; both stand above)

namespace cmfk {

struct AlsLogitPassArgs {
    const AlsBiasPiece *pieces;
    const int32_t *idx;
    const float *wv;
    const float *A, *B;          // the factor of the image's rows, the gathered factor; pitch kp
    int kp;
    float *hw;                   // [nnz]
};

enum { ALS_LOGIT_PASS_FLIGHT = 4 };   // gathered rows in flight per lane group

template <int GL>
__global__ __launch_bounds__(256) void als_logit_pass_kernel(AlsLogitPassArgs g) {
#pragma clang fp contract(off)
    constexpr int NG = 256 / GL, NF = ALS_LOGIT_PASS_FLIGHT;
    const AlsBiasPiece pc = g.pieces[blockIdx.x];
    const int gl = threadIdx.x % GL, grp = threadIdx.x / GL;
    const f32x4 a = *reinterpret_cast<const f32x4 *>(g.A + (int64_t)pc.row * g.kp + 4 * gl);
    const int32_t *idx = g.idx + pc.beg;
    const float *wv = g.wv + pc.beg;
    float *hw = g.hw + pc.beg;
    // every group runs the same number of rounds (an entry past the piece's end reads the piece's last entry again and stores
    // nothing): the lanes of a wave stay together through group_sum
    for (int base = 0; base < pc.len; base += NF * NG) {
        int e[NF], q[NF];
        f32x4 b[NF];
        float w[NF], s[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            e[j] = base + grp + j * NG;
            q[j] = min(e[j], pc.len - 1);
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) b[j] = *reinterpret_cast<const f32x4 *>(g.B + (int64_t)idx[q[j]] * g.kp + 4 * gl);
#pragma unroll
        for (int j = 0; j < NF; ++j) w[j] = wv[q[j]];
#pragma unroll
        for (int j = 0; j < NF; ++j) s[j] = group_sum<GL>(a[0] * b[j][0] + a[1] * b[j][1] + a[2] * b[j][2] + a[3] * b[j][3]);
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const float kap = fabsf(s[j]) < 1e-4f ? 0.25f : tanhf(0.5f * s[j]) / (2.0f * s[j]);   // (als_logit_kappa's expression)
            if (gl == 0 && e[j] < pc.len) hw[e[j]] = w[j] * kap;
        }
    }
}

__global__ void als_logit_hp_kernel(const float *pv, const float *wv, int64_t n, float *hp) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) hp[i] = pv[i] - 0.5f * wv[i];
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als_huber.hip.h)
#ifdef CMF_ALS_HOST
// hw / hp and the piece lists of both images of a passed logistic relation (als_huber_build, without the transposed targets), and hp
// of both images, which no sweep changes
static int als_logit_pass_ensure(cmf_ctx *c, int which) {
    const AlsHuber &h = c->als_huber[which];
    if (h.ready && h.logit) return CMF_OK;
    CHK(als_huber_ensure(c, which, true));
    for (int t = 0; t < 2; ++t) {
        const WCsrDev &M = c->wm_sp[which][t];
        CHK(launch_ew(c, cmfk::als_logit_hp_kernel, M.nnz, (const float *)M.pv, (const float *)M.wv, M.nnz, M.hp));
    }
    return CMF_OK;
}

// hw of image t of the passed logistic relation `which` from the current factors
static int als_logit_pass_refresh(cmf_ctx *c, int which, int t) {
    CHK(als_logit_pass_ensure(c, which));
    const AlsHuber &h = c->als_huber[which];
    const WCsrDev &M = c->wm_sp[which][t];
    const int64_t np = h.npieces[t];
    if (np <= 0) return CMF_OK;
    cmfk::AlsLogitPassArgs a;
    memset(&a, 0, sizeof a);
    a.pieces = h.pieces[t];
    a.idx = M.idx;
    a.wv = M.wv;
    a.A = c->F[which == 0 ? (t == 0 ? CMF_U : CMF_V) : (t == 0 ? CMF_V : CMF_Z)];
    a.B = c->F[which == 0 ? (t == 0 ? CMF_V : CMF_U) : (t == 0 ? CMF_Z : CMF_V)];
    a.kp = c->kp;
    a.hw = M.hw;
    Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
    const dim3 grid((unsigned)np), block(256);
    ALS_LAUNCH_GL(c, als_logit_pass_kernel, grid, block, 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

extern "C" int cmf_set_logit_pass(cmf_ctx *c, int which, int enable) {
    NEED_PROBLEM(c);
    CHK(als_huber_which_ok("cmf_set_logit_pass", which));
    if (!enable && c->als_huber[which].ready && c->als_huber[which].logit) {   // what the pass built for the pattern goes with the flag
        DeviceGuard dg(c->device);
        HIPCHK(hipStreamSynchronize(c->stream));
        als_huber_free(c, which);
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

// test entry: hw and hp of image t (0 the pattern, 1 its transpose) of a passed logistic relation at the current factors; nnz: the
// entries the caller's buffers hold, which must be the stored entries of the pattern
extern "C" int cmf_als_logit_weights(cmf_ctx *c, int which, int t, int64_t nnz, float *w_eff, float *p_eff) {
    NEED_PROBLEM(c);
    const char *what = "cmf_als_logit_weights";
    CHK(als_huber_which_ok(what, which));
    if (t != 0 && t != 1) return fail(CMF_EINVAL, "%s: the image must be 0 (the pattern) or 1 (its transpose)", what);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: n_components <= 256 only (k_pad = %d)", what, c->kp);
    const char *nm = which == 0 ? "X" : "Y";
    if (!als_logit_rel(c, which)) return fail(CMF_EINVAL, "%s: %s has no logistic loss (cmf_set_relation_loss first)", what, nm);
    if (!c->als_logit_pass[which]) return fail(CMF_EINVAL, "%s: %s is reweighted inside the normal-equation kernel (cmf_set_logit_pass first)", what, nm);
    CHK(als_logit_check(c, what, which == 0 ? CMF_UPD_U : CMF_UPD_Z));
    CHK(als_huber_rel_ok(c, what, which));
    const WCsrDev &M = c->wm_sp[which][t];
    if (nnz != M.nnz) return fail(CMF_EINVAL, "%s: the caller's buffers hold %lld entries, the pattern stores %lld", what, (long long)nnz, (long long)M.nnz);
    DeviceGuard dg(c->device);
    CHK(als_logit_pass_refresh(c, which, t));
    if (M.nnz && w_eff) HIPCHK(hipMemcpyAsync(w_eff, M.hw, (size_t)M.nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (M.nnz && p_eff) HIPCHK(hipMemcpyAsync(p_eff, M.hp, (size_t)M.nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

#endif // CMF_ALS_HOST
