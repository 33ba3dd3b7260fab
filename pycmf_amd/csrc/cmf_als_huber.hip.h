// cmf_als_huber.hip.h -- a Huber loss for the ALS solver: a relation with CSR weights may be fitted under
//   sum_O w rho_d(t - a . b),      rho_d(r) = 1/2 r^2 if |r| <= d,  d (|r| - 1/2 d) otherwise      (cmf_set_huber_delta, d > 0)
// next to the other relation as it is today.  The half-quadratic majoriser
//   rho_d(r) <= rho_d(r0) + 1/2 omega(r0) (r^2 - r0^2),      omega(r) = 1 if |r| <= d,  d / |r| otherwise,      tight at r = +-r0
// with r0 the residual under the CURRENT row makes the majoriser of row i the row problem of cmf_als.hip.h under w omega in place of
// w, on the same targets.  So no row kernel changes: ONE pass of its own in front of every sweep writes, per stored entry of the
// image the sweep reads, the effective weight and the effective product
//   r = tt - s,   omega = |r| <= d ? 1 : d / |r|,   hw = w omega,   hp = pp omega
// (tt: the adjusted targets under biases, else t; pp: bp under biases, else pv = w t; s = a . b in float32 from group_sum), and the
// row routes read hw / hp through als_side_weights / als_side_targets while the sweep has them bound (AlsHuberGuard,
// cmf_als_steps.hip.h).  Every route starts at the current row and never raises its quadratic, so every sweep lowers the true
// objective.  omega == 1 leaves w and pp with their bits: under a delta no residual reaches, every route gives the bits it gives
// without one.
//   als_huber_pass_kernel<GL, LOSS>  one 256-thread workgroup per piece of at most 2048 stored entries of one row (AlsBiasPiece, the
//                          lane layout of als_logit_loss_kernel): the row a in registers, GL = k_pad / 4 lanes x f32x4 per gathered
//                          row, the 256 / GL lane groups deal the piece's entries round-robin, FOUR gathered rows in flight per
//                          group.  LOSS = false: hw and hp leave through lane 0 of the group; an entry past the piece's end writes
//                          nothing.  LOSS = true: sum w rho_d(r), the terms in float32, added in float64 per lane group, the groups
//                          in group order; the pieces in piece order behind the kernel boundary (als_logit_sum_kernel).
// No atomics, vector stores only: a repeated call from the same state is bit-identical.
#pragma once
#include "cmf_kernels.hip.h"   // (AlsBiasPiece: cmf_als_bias.hip.h; als_logit_sum_kernel: cmf_als_logit.hip.h; both stand above)

namespace cmfk {

struct AlsHuberArgs {
    const AlsBiasPiece *pieces;
    const int32_t *idx;
    const float *tt, *wv, *pp;   // targets (adjusted under biases), weights, products w tt
    const float *A, *B;          // the factor of the image's rows, the gathered factor; pitch kp
    int kp;
    float delta;
    float *hw, *hp;              // LOSS = false: [nnz] each
    double *part;                // LOSS = true: [pieces]
};

enum { ALS_HUBER_FLIGHT = 4 };   // gathered rows in flight per lane group

template <int GL, bool LOSS>
__global__ __launch_bounds__(256) void als_huber_pass_kernel(AlsHuberArgs g) {
#pragma clang fp contract(off)
    constexpr int NG = 256 / GL, NF = ALS_HUBER_FLIGHT;
    const AlsBiasPiece pc = g.pieces[blockIdx.x];
    const int gl = threadIdx.x % GL, grp = threadIdx.x / GL;
    const f32x4 a = *reinterpret_cast<const f32x4 *>(g.A + (int64_t)pc.row * g.kp + 4 * gl);
    const int32_t *idx = g.idx + pc.beg;
    const float *tt = g.tt + pc.beg, *wv = g.wv + pc.beg;
    const float d = g.delta;
    [[maybe_unused]] double sum = 0.0;
    // every group runs the same number of rounds (an entry past the piece's end reads the piece's last entry again, and neither
    // stores nor adds): the lanes of a wave stay together through group_sum
    for (int base = 0; base < pc.len; base += NF * NG) {
        int e[NF], q[NF];
        f32x4 b[NF];
        float t[NF], w[NF], s[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            e[j] = base + grp + j * NG;
            q[j] = min(e[j], pc.len - 1);
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) b[j] = *reinterpret_cast<const f32x4 *>(g.B + (int64_t)idx[q[j]] * g.kp + 4 * gl);
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            t[j] = tt[q[j]];
            w[j] = wv[q[j]];
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) s[j] = group_sum<GL>(a[0] * b[j][0] + a[1] * b[j][1] + a[2] * b[j][2] + a[3] * b[j][3]);
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const float r = t[j] - s[j], ar = fabsf(r);
            if constexpr (LOSS) {
                const float term = w[j] * (ar <= d ? 0.5f * (r * r) : d * (ar - 0.5f * d));
                if (gl == 0 && e[j] < pc.len) sum += (double)term;   // (every lane of the group holds the term; lane 0 keeps the sum)
            } else {
                const float om = ar <= d ? 1.0f : d / ar;
                if (gl == 0 && e[j] < pc.len) {
                    g.hw[pc.beg + e[j]] = w[j] * om;
                    g.hp[pc.beg + e[j]] = g.pp[pc.beg + e[j]] * om;
                }
            }
        }
    }
    if constexpr (LOSS) {
        __shared__ double red[NG];
        if (gl == 0) red[grp] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            double v = red[0];
            for (int x = 1; x < NG; ++x) v += red[x];
            g.part[blockIdx.x] = v;
        }
    }
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als_logit.hip.h)
#ifdef CMF_ALS_HOST
enum { ALS_HUBER_PIECE = 2048 };

static bool als_huber_rel(const cmf_ctx *c, int which) { return c->als_huber[which].delta > 0.0; }

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

// What the pass needs beyond the images: hw / hp of both images, t in the stored order of the transpose, and the piece lists of both
// images -- built once per bound pattern (als_huber_free drops them with the weights), like AlsBias::pieces.  logit: for the logistic
// pass (cmf_als_logit_pass.hip.h), which shares the arrays and the piece lists and reads no targets.
static int als_huber_build(cmf_ctx *c, int which, bool logit) {
    AlsHuber &h = c->als_huber[which];
    const int64_t nnz = c->wm_sp[which][0].nnz;
    const size_t vbytes = std::max<size_t>(16, (size_t)nnz * sizeof(float));
    h.logit = logit;
    if (!logit) {
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
        std::vector<int64_t> ip((size_t)M.rows + 1, 0);
        HIPCHK(hipMemcpyAsync(ip.data(), M.indptr, ip.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        std::vector<cmfk::AlsBiasPiece> pieces;
        als_cut_rows(&ip, 1, M.rows, ALS_HUBER_PIECE, [&](int64_t r, int, int64_t beg, int32_t len) {
            pieces.push_back(cmfk::AlsBiasPiece{beg, len, (int32_t)r});
        });
        if ((int64_t)pieces.size() > INT32_MAX) return fail(CMF_EUNSUPPORTED, "the Huber pass: more than 2^31 - 1 pieces");
        CHK(dev_alloc(c, (void **)&h.pieces[t], std::max<size_t>(16, pieces.size() * sizeof(cmfk::AlsBiasPiece)), false));
        if (!pieces.empty()) HIPCHK(hipMemcpyAsync(h.pieces[t], pieces.data(), pieces.size() * sizeof(cmfk::AlsBiasPiece), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream)); // the host vector may go
        h.npieces[t] = (int64_t)pieces.size();
    }
    return CMF_OK;
}
// (a relation takes a Huber loss or a logistic one, never both at once: what the other loss built for the pattern is dropped first)
static int als_huber_ensure(cmf_ctx *c, int which, bool logit = false) {
    if (c->als_huber[which].ready && c->als_huber[which].logit == logit) return CMF_OK;
    if (c->als_huber[which].ready) {
        HIPCHK(hipStreamSynchronize(c->stream));
        als_huber_free(c, which);
    }
    const int rc = als_huber_build(c, which, logit);
    if (rc != CMF_OK) {
        (void)hipStreamSynchronize(c->stream);
        als_huber_free(c, which);
        return rc;
    }
    c->als_huber[which].ready = true;
    return CMF_OK;
}

// the arguments of a pass over image t of relation `which` at the current factors (and, under biases, the current adjusted targets)
static int als_huber_args(cmf_ctx *c, int which, int t, cmfk::AlsHuberArgs &a) {
    CHK(als_huber_ensure(c, which));
    CHK(als_bias_refresh(c, which));   // (written when the biases last changed: nothing to do)
    const AlsHuber &h = c->als_huber[which];
    const WCsrDev &M = c->wm_sp[which][t];
    memset(&a, 0, sizeof a);
    a.pieces = h.pieces[t];
    a.idx = M.idx;
    a.tt = M.bt ? M.bt : (t == 0 ? M.tv : h.tt1);
    a.wv = M.wv;
    a.pp = M.bp ? M.bp : M.pv;
    a.A = c->F[which == 0 ? (t == 0 ? CMF_U : CMF_V) : (t == 0 ? CMF_V : CMF_Z)];
    a.B = c->F[which == 0 ? (t == 0 ? CMF_V : CMF_U) : (t == 0 ? CMF_Z : CMF_V)];
    a.kp = c->kp;
    a.delta = (float)h.delta;
    a.hw = M.hw;
    a.hp = M.hp;
    return CMF_OK;
}

// hw, hp of image t of Huber relation `which` from the current factors
static int als_huber_refresh(cmf_ctx *c, int which, int t) {
    cmfk::AlsHuberArgs a;
    CHK(als_huber_args(c, which, t, a));
    const int64_t np = c->als_huber[which].npieces[t];
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
    const int64_t np = c->als_huber[which].npieces[0];
    *out = 0.0;
    if (np <= 0) return CMF_OK;
    CHK(ensure_scratch(c, c->als_bias_part, (size_t)(np + 1) * sizeof(double)));
    a.part = (double *)c->als_bias_part.p;
    double *sum = a.part + np;
    {
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)c->wm_sp[which][0].nnz * (double)c->kp);
        const dim3 grid((unsigned)np), block(256);
        ALS_LAUNCH_GL_T(c, als_huber_pass_kernel, true, grid, block, 0, c->stream, a);
        hipLaunchKernelGGL(cmfk::als_logit_sum_kernel, dim3(1), dim3(64), 0, c->stream, (const double *)a.part, np, sum);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

// (cmf_als_logit_pass.hip.h, which stands below: hw of one image of a passed logistic relation from the current factors)
static int als_logit_pass_refresh(cmf_ctx *c, int which, int t);

// The Huber sides of one sweep, bound for its duration: bind() refreshes hw / hp of every Huber image the sweep reads, in the
// sweep's orientation, from the current factors, and als_side_weights / als_side_targets return them until the scope ends.  Nothing
// outside a sweep ever sees them: the residual, the bias targets and the losses read the images as they were bound.  A logistic
// relation under cmf_set_logit_pass is bound in the same way, behind its own pass.
struct AlsHuberGuard {
    cmf_ctx *const c;
    WCsrDev *bound[2] = {nullptr, nullptr};
    explicit AlsHuberGuard(cmf_ctx *ctx) : c(ctx) {}
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
    ~AlsHuberGuard() {
        for (int s = 0; s < 2; ++s)
            if (bound[s]) bound[s]->hbound = false;
    }
    AlsHuberGuard(const AlsHuberGuard &) = delete;
    AlsHuberGuard &operator=(const AlsHuberGuard &) = delete;
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
        als_huber_free(c, which);
    }
    c->als_huber[which].delta = (double)df;
    return CMF_OK;
}

extern "C" int cmf_get_huber_delta(cmf_ctx *c, int which, double *delta) {
    NEED_PROBLEM(c);
    CHK(als_huber_which_ok("cmf_get_huber_delta", which));
    if (!delta) return fail(CMF_EINVAL, "cmf_get_huber_delta: null output");
    *delta = c->als_huber[which].delta;
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

// test entry: hw and hp of image t (0 the pattern, 1 its transpose) of a Huber relation at the current factors; nnz: the entries the
// caller's buffers hold, which must be the stored entries of the pattern
extern "C" int cmf_als_huber_weights(cmf_ctx *c, int which, int t, int64_t nnz, float *w_eff, float *p_eff) {
    NEED_PROBLEM(c);
    const char *what = "cmf_als_huber_weights";
    CHK(als_huber_which_ok(what, which));
    if (t != 0 && t != 1) return fail(CMF_EINVAL, "%s: the image must be 0 (the pattern) or 1 (its transpose)", what);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: n_components <= 256 only (k_pad = %d)", what, c->kp);
    if (!als_huber_rel(c, which)) return fail(CMF_EINVAL, "%s: %s has no Huber loss (cmf_set_huber_delta first)", what, which == 0 ? "X" : "Y");
    CHK(als_huber_rel_ok(c, what, which));
    const WCsrDev &M = c->wm_sp[which][t];
    if (nnz != M.nnz) return fail(CMF_EINVAL, "%s: the caller's buffers hold %lld entries, the pattern stores %lld", what, (long long)nnz, (long long)M.nnz);
    DeviceGuard dg(c->device);
    CHK(als_huber_refresh(c, which, t));
    if (M.nnz && w_eff) HIPCHK(hipMemcpyAsync(w_eff, M.hw, (size_t)M.nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (M.nnz && p_eff) HIPCHK(hipMemcpyAsync(p_eff, M.hp, (size_t)M.nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

#endif // CMF_ALS_HOST
