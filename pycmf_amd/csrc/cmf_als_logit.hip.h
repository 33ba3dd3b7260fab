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
//   als_logit_normal_kernel<KP>   als_normal_kernel's geometry, restated (that kernel and AlsPiece stay as they are: a fit without
//                          a logistic relation launches exactly what it launched before this file).  A piece carries its row index
//                          (AlsLogitPiece); the LPR lanes that hold one gathered row in rr[] hold the same columns of the current
//                          row in fr[] (CPT more f32x4 per lane, loaded once per workgroup).  When a staged tile leaves the
//                          registers, a logistic side forms the partial dot sum rr . fr per lane, reduces it over the LPR lanes in
//                          the fixed order of group_sum (every lane of the group ends with the same bits of s), and sets
//                              kappa = |s| < 1e-4 ? 0.25f : tanhf(0.5f s) / (2 s),   sq = sqrtf(w kappa),   pe = p - 0.5f w;
//                          a Frobenius side's piece of the same launch keeps sq = sqrtf(w), pe = p (the flag is uniform over the
//                          workgroup).  The reweighting sits in `stage`, not in `gather`: the loads of gather(tl + 2) stay in flight
//                          across the MFMAs of step tl, and the dot waits for them only where the registers are consumed anyway.
//                          The pieces' partial sums go to als_finish_kernel, unchanged.
//   als_logit_loss_kernel<GL>     sum_O w [max(s, 0) + log1p(exp(-|s|)) - t s]: one 256-thread workgroup per piece of at most 2048
//                          stored entries of one row (AlsBiasPiece, the lane layout of als_bias_piece_kernel), s in float32, the
//                          terms added in float64 per lane group, the groups in group order; the pieces are added in piece order
//                          behind the kernel boundary (als_logit_sum_kernel, one thread).
// No atomics anywhere, vector stores only: a repeated call from the same state is bit-identical.
#ifndef CMF_ALS_LOGIT_KERNELS
#define CMF_ALS_LOGIT_KERNELS
#include "cmf_kernels.hip.h"
#include "cmf_als_bias.hip.h"

namespace cmfk {

struct AlsLogitPiece {
    int64_t beg;            // first stored entry
    int32_t len;            // entries (1 .. piece length)
    int32_t side;           // 0 | 1: which of the two CSR images of the sweep
    int64_t row;            // of the swept factor
};
struct AlsLogitArgs {
    AlsSide s0, s1;
    const AlsLogitPiece *pieces; // one per workgroup
    float *Hp;              // as AlsArgs
    float *gp;
    const float *F;         // the swept factor, pitch KP: the current rows
    int logit0, logit1;     // the side is logistic (1) or Frobenius (0)
};

// kappa(s) = tanh(s / 2) / (2 s), 1/4 at 0 (the guard: tanh(s / 2) / (2 s) = 1/4 - s^2 / 48 + ..., below 2^-24 off 1/4 for |s| < 1e-4)
__device__ __forceinline__ float als_logit_kappa(float s) { return fabsf(s) < 1e-4f ? 0.25f : tanhf(0.5f * s) / (2.0f * s); }

template <int KP>
__global__ __launch_bounds__(512) void als_logit_normal_kernel(AlsLogitArgs g) {
    using C = AlsCfg<KP>;
    __shared__ __attribute__((aligned(16))) float sm[2 * C::TILE];
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, lh = lane >> 5;
    const int uw = __builtin_amdgcn_readfirstlane(t >> 6);
    const AlsLogitPiece pc = g.pieces[blockIdx.x];
    const bool second = pc.side != 0;
    const bool logit = (second ? g.logit1 : g.logit0) != 0;   // uniform over the workgroup
    const int32_t *idx = (second ? g.s1.idx : g.s0.idx) + pc.beg;
    const float *pv = (second ? g.s1.pv : g.s0.pv) + pc.beg;
    const float *wv = (second ? g.s1.wv : g.s0.wv) + pc.beg;
    const float *B = second ? g.s1.B : g.s0.B;
    const int ns = pc.len, nt = (ns + 31) >> 5;
    const int trow = t / C::LPR, tl16 = t % C::LPR;
    const bool loader = t < 32 * C::LPR;    // k_pad = 32: half of the threads cover the tile

    f32x4 rr[C::CPT], gacc[C::CPT], fr[C::CPT];
    float wq = 0.f, pq = 0.f;               // w and p of the gathered row, as stored
#pragma unroll
    for (int q = 0; q < C::CPT; ++q) rr[q] = gacc[q] = fr[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (logit && loader) {                  // the current row: the columns this lane holds of every gathered row
        const float *src = g.F + pc.row * KP + 4 * tl16;
#pragma unroll
        for (int c = 0; c < C::CPT; ++c) fr[c] = *reinterpret_cast<const f32x4 *>(src + 4 * c * C::LPR);
    }
    f32x16 hs[5];
#pragma unroll
    for (int n = 0; n < 5; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) hs[n][r] = 0.f;

    // this wave's fragments: block columns of the staged image (all wave-uniform)
    int wty, fcol[5] = {0, 0, 0, 0, 0};
    bool mfma_wave = true;
    if constexpr (KP == 256) {
        wty = uw < 4 ? 0 : ((uw & 1) ? 2 : 1);
        const int sbase = uw >= 6 ? 4 : 0;
        if (wty == 0) { fcol[0] = uw; fcol[1] = 4; fcol[2] = 5; fcol[3] = 6; fcol[4] = 7; }
        else if (wty == 1) { fcol[0] = sbase; fcol[1] = sbase + 1; fcol[2] = sbase + 2; fcol[3] = sbase + 3; }
        else { fcol[0] = sbase + 1; fcol[1] = sbase + 2; fcol[2] = sbase + 3; }
    } else {
        wty = 3;
        mfma_wave = uw < C::WM * C::WN;
        fcol[0] = uw / C::WN;
#pragma unroll
        for (int y = 0; y < C::TN; ++y) fcol[1 + y] = (uw % C::WN) * C::TN + y;
    }

    auto gather = [&](int tl) { // the rows of step tl into registers; beyond the end of the piece: zeros
        const int q = 32 * tl + trow;
        if (loader && q < ns) {
            const float *src = B + (int64_t)idx[q] * KP + 4 * tl16;
#pragma unroll
            for (int c = 0; c < C::CPT; ++c) rr[c] = *reinterpret_cast<const f32x4 *>(src + 4 * c * C::LPR);
            wq = wv[q];
            pq = pv[q];
        } else {
#pragma unroll
            for (int c = 0; c < C::CPT; ++c) rr[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            wq = 0.f;
            pq = 0.f;
        }
    };
    auto stage = [&](int nb) { // registers -> gradient part and the sqrt(w kappa)-scaled LDS image
        float sq, pe = pq;
        if (logit) {           // (all lanes: a row past the end of the piece is zeros with w = 0; the lanes of a row's group stay together)
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < C::CPT; ++c) d += rr[c][0] * fr[c][0] + rr[c][1] * fr[c][1] + rr[c][2] * fr[c][2] + rr[c][3] * fr[c][3];
            const float s = group_sum<C::LPR>(d);
            sq = sqrtf(wq * als_logit_kappa(s));
            pe = pq - 0.5f * wq;
        } else {
            sq = sqrtf(wq);
        }
        if (!loader) return;
        float *dst = sm + nb * C::TILE + trow * KP + 4 * tl16;
#pragma unroll
        for (int c = 0; c < C::CPT; ++c) {
            gacc[c] += pe * rr[c];
            *reinterpret_cast<f32x4 *>(dst + 4 * c * C::LPR) = sq * rr[c];
        }
    };
    auto tile = [&](auto typ, int cb) {
        constexpr int TY = decltype(typ)::value;
        constexpr int NF = als_nf<KP>(TY), NP = als_np<KP>(TY);
        const float *R = sm + cb * C::TILE + l31;
        float b[2][NF];
        auto ld_frag = [&](int sidx, float *db) {
            const int kk = 2 * sidx + lh;
#pragma unroll
            for (int f = 0; f < NF; ++f) db[f] = R[kk * KP + 32 * fcol[f]];
        };
        ld_frag(0, b[0]);
#pragma unroll
        for (int sidx = 0; sidx < 16; ++sidx) {
            if (sidx + 1 < 16) ld_frag(sidx + 1, b[(sidx + 1) & 1]);
#pragma unroll
            for (int n = 0; n < NP; ++n)
                hs[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[sidx & 1][als_ai(TY, n)], b[sidx & 1][als_bi(TY, n)], hs[n], 0, 0, 0);
        }
    };

    gather(0);
    stage(0);
    if (nt > 1) gather(1);
    __syncthreads();
    for (int tl = 0; tl < nt; ++tl) {
        // tile (tl + 1) & 1 was last read before the barrier that closed step tl - 1
        if (tl + 1 < nt) {
            stage((tl + 1) & 1);
            if (tl + 2 < nt) gather(tl + 2);
        }
        if constexpr (KP == 256) {
            if (wty == 0) tile(AlsIntC<0>(), tl & 1);
            else if (wty == 1) tile(AlsIntC<1>(), tl & 1);
            else tile(AlsIntC<2>(), tl & 1);
        } else {
            if (mfma_wave) tile(AlsIntC<3>(), tl & 1);
        }
        __syncthreads();
    }

    // register r of a lane: row (r & 3) + 8 (r >> 2) + 4 lh of the block (the A fragment's block column), column l31 (the B fragment's)
    float *Hd = g.Hp + (int64_t)blockIdx.x * KP * KP;
    auto store = [&](auto typ) {
        constexpr int TY = decltype(typ)::value;
        constexpr int NP = als_np<KP>(TY);
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            float *dst = Hd + (int64_t)(32 * fcol[als_ai(TY, n)] + 4 * lh) * KP + 32 * fcol[als_bi(TY, n)] + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[((r & 3) + 8 * (r >> 2)) * KP] = hs[n][r];
        }
    };
    if constexpr (KP == 256) {
        if (wty == 0) store(AlsIntC<0>());
        else if (wty == 1) store(AlsIntC<1>());
        else store(AlsIntC<2>());
    } else {
        if (mfma_wave) store(AlsIntC<3>());
    }
    // gradient part: the 32 tile rows' partial sums through LDS, added in row order
    if (loader) {
#pragma unroll
        for (int c = 0; c < C::CPT; ++c) *reinterpret_cast<f32x4 *>(sm + trow * KP + 4 * (c * C::LPR + tl16)) = gacc[c];
    }
    __syncthreads();
    if (t < KP) {
        float v = 0.f;
#pragma unroll
        for (int r = 0; r < 32; ++r) v += sm[r * KP + t];
        g.gp[(int64_t)blockIdx.x * KP + t] = v;
    }
}

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
#endif // CMF_ALS_LOGIT_KERNELS

// ------------------------------------------------------------------ host side (included by cmf_als.hip.h behind AlsPlan)
#if defined(CMF_ALS_LOGIT_HOST) && !defined(CMF_ALS_LOGIT_HOST_DONE)
#define CMF_ALS_LOGIT_HOST_DONE

enum { ALS_LOGIT_LOSS_PIECE = 2048 };

static bool als_logit_rel(const cmf_ctx *c, int which) { return c->rel_loss[which] == CMF_LOSS_LOGISTIC; }

// does the sweep of factor f read a logistic relation?
static bool als_logit_sweep(const cmf_ctx *c, const AlsSweep &sw) {
    for (int s = 0; s < sw.nrel; ++s)
        if (als_logit_rel(c, sw.rel[s].which)) return true;
    return false;
}

// the relations X (U, V sweeps) / Y (V, Z sweeps) a step with this mask reads
static bool als_logit_swept(const cmf_ctx *c, int mask) {
    return ((mask & (CMF_UPD_U | CMF_UPD_V)) && als_logit_rel(c, 0)) || ((mask & (CMF_UPD_Z | CMF_UPD_V)) && als_logit_rel(c, 1));
}

// What a step that sweeps a logistic relation cannot do: the relation must be observed (CSR weights), without a background weight and
// without biases.  cg: the entry point asked for the conjugate-gradient route, which has no reweighting pass.
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
        if (cg)
            return fail(CMF_EUNSUPPORTED, "%s: %s has a logistic loss; the conjugate-gradient rows have no reweighting pass: use cmf_als_step or cmf_als_nnls_step", what, nm);
    }
    return CMF_OK;
}

// the pieces of a plan with their rows (row r_begin + r owns pl.first[r] .. pl.first[r + 1])
static void als_logit_pieces(const AlsPlan &pl, int64_t r_begin, std::vector<cmfk::AlsLogitPiece> &out) {
    out.resize(pl.pieces.size());
    for (size_t r = 0; r + 1 < pl.first.size(); ++r)
        for (int64_t p = pl.first[r]; p < pl.first[r + 1]; ++p) {
            const cmfk::AlsPiece &q = pl.pieces[(size_t)p];
            out[(size_t)p] = cmfk::AlsLogitPiece{q.beg, q.len, q.side, r_begin + (int64_t)r};
        }
}

static int als_logit_launch_normal(cmf_ctx *c, const cmfk::AlsLogitArgs &a, int64_t npieces, int64_t nnz) {
    if (npieces <= 0) return CMF_OK;
    Timed tm(c, CMF_K_ROWHESS, 2.0 * (double)nnz * c->k * c->k + 2.0 * (double)nnz * c->k);
    const dim3 grid((unsigned)npieces), block(512);
    ALS_LAUNCH_KP(c, als_logit_normal_kernel, "ALS normal equations are", hipLaunchKernelGGL(kern, grid, block, 0, c->stream, a));
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
    const int64_t L = ALS_LOGIT_LOSS_PIECE;
    for (int64_t r = 0; r < M.rows; ++r)
        for (int64_t q = ip[(size_t)r]; q < ip[(size_t)r + 1]; q += L)
            pieces.push_back(cmfk::AlsBiasPiece{q, (int32_t)std::min<int64_t>(L, ip[(size_t)r + 1] - q), (int32_t)r});
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
        switch (c->kp) {
        case 32: hipLaunchKernelGGL((cmfk::als_logit_loss_kernel<8>), grid, block, 0, c->stream, a); break;
        case 64: hipLaunchKernelGGL((cmfk::als_logit_loss_kernel<16>), grid, block, 0, c->stream, a); break;
        case 128: hipLaunchKernelGGL((cmfk::als_logit_loss_kernel<32>), grid, block, 0, c->stream, a); break;
        default: hipLaunchKernelGGL((cmfk::als_logit_loss_kernel<64>), grid, block, 0, c->stream, a); break;
        }
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

#endif // CMF_ALS_LOGIT_HOST
