// cmf_als.hip.h -- ALS (alternating least squares) on the quadratic objective over an observed pattern
//   1/2 sum_{Ox} wx_ij (x_ij - u_i . v_j)^2 + 1/2 sum_{Oy} wy_jc (y_jc - v_j . z_c)^2 + l2 / 2 (|U|^2 + |V|^2 + |Z|^2),   l2 > 0.
// Every row f_i of the factor being swept has its own k x k system
//   (sum_{c in O_i} w_ic b_c b_c^T + S + l2 I) f_i = sum_{c in O_i} w_ic t_ic b_c + N_i
// where an OBSERVED relation (weights bound as CSR, cmf_set_weighted_csr) contributes the sums over its stored entries and a FULL
// relation (no weights: every cell counts with weight 1) the shared Gram S = B^T B and the row N_i of T B.  Under a background
// weight c0 (cmf_als_bg.hip.h, implicit feedback) an observed relation counts the cells outside its pattern too: the kernels read
// the excess weights w - c0 where they read w, and S = sum_sides coef Gram(B_side) (als_shared_terms).  What depended on "a full
// side exists" depends on "S is set".  The route of a sweep (als_route; sweeps / cg_steps: 0 where the entry point has no count):
//   route         taken when                                           what it does
//   shared exact  no observed relation; signed, or sweeps = 0          ONE matrix G + l2 I for all rows, inverted once in float64
//                                                                      (shared_inverse64), one product, projected if non-negative
//   shared HALS   no observed relation; non-negative, sweeps > 0       hals_sweep (cmf_hals.hip.h) `sweeps` times on the one Gram
//   rows exact    observed; non-negative with sweeps = 0, or signed    the finished systems through safe_solve_rows (cmf_newton.hip.h):
//                 with cg_steps = 0                                    Hessians declared positive semi-definite, threshold l2 / 16
//                                                                      (lambda_min(H_i) >= l2: the spectral clamp never acts), no
//                                                                      float64 refinement; projected if non-negative
//   rows NNLS     observed; non-negative, sweeps > 0                   the finished systems to als_nnls_kernel (cmf_als_nnls.hip.h):
//                                                                      cyclic coordinate descent from the current rows, in place
//   rows CG       observed; signed, cg_steps > 0                       no systems: als_cg_kernel (cmf_als_cg.hip.h) runs matrix-free
//                                                                      CG steps per row from the current rows, in place; the host
//                                                                      sorts the rows into LDS capacity classes by length; a row
//                                                                      longer than "als_cg_piece" entries is cut into pieces
//                                                                      (als_cg_piece_kernel / als_cg_combine_kernel)
//   rows NNCG     observed; non-negative, nn_cg_steps > 0 (before      no systems: als_nncg_kernel (cmf_als_nncg.hip.h) runs matrix-free
//                 `sweeps` is looked at; cmf_als_nncg_step only)       projected CG steps per row from the current rows clamped at
//                                                                      zero, in place; the classes and the pieces of rows CG
//   rows dual     a sweep on rows exact with S = N = null and no        the rows of 1 .. dual_max stored entries whose class width
//                 logistic relation, under cmf_als_dual_step's          NP(n) < k_pad: K = A A^T + l2 I_n (als_dual_gram_kernel,
//                 permission dual_max >= 1                              cmf_als_dual.hip.h), K z = y through safe_solve_rows, f = A^T z;
//                                                                      the same exact row from an n x n system; other rows: rows exact
//
// The finished systems (als_chunks).  als_normal_kernel<KP, LG>: one 512-thread workgroup per PIECE of a row (at most `als_piece` stored
// entries, a multiple of 32) of a CSR image (indptr, idx, pv = w t, wv = w).  The gathered rows b_e are staged 32 at a time through
// registers into a double-buffered LDS tile, scaled by sqrt(w_e); while they are in registers the owning lanes add p_e b_e to the
// gradient part g.  H is a rank-32 update per step on v_mfma_f32_32x32x2_f32, both operands read from the ONE staged image:
//     H = sum_e (sqrt(w_e) b_e)(sqrt(w_e) b_e)^T,     g = sum_e p_e b_e.
// The geometry is that of row_hess_kernel in its single-image symmetric form (cmf_rowhess.hip.h, SYM = 3), restated here, not
// shared: 16 lanes per gathered row, row-major 32 x KP tiles, and at k_pad = 256 only the 36 blocks (32 x 32) on or above the block
// diagonal, spread 4 + 5 + 5 over the wave types
//     waves 0-3:            (w, 4) (w, 5) (w, 6) (w, 7)                                   5 fragments per k-pair
//     waves 4, 6 (base b):  (b, b) (b, b+1) (b, b+2) (b, b+3) (b+3, b+3)                  4 fragments
//     waves 5, 7 (base b):  (b+1, b+1) (b+1, b+2) (b+1, b+3) (b+2, b+2) (b+2, b+3)        3 fragments
// Below k_pad = 256 every block is formed (wave (wm, wn) owns block row wm, TN block columns).  Unlike row_hess_kernel there is no
// targets image, and under LG = false (no relation of the sweep is logistic) no dot product with the current row: the system does
// not depend on f_i.
// LG = true: the sweep reads a logistic relation (cmf_als_logit.hip.h), whose system is the one above under w kappa in place of w and
// w (t - 1/2) in place of w t, kappa taken at the score under the CURRENT row.  The LPR lanes that hold one gathered row in rr[] hold
// the same columns of the piece's row (AlsPiece::row) of F in fr[] (CPT more f32x4 per lane, loaded once per workgroup).  When a
// staged tile leaves the registers, a logistic side forms the partial dot sum rr . fr per lane, reduces it over the LPR lanes in the
// fixed order of group_sum (every lane of the group ends with the same bits of s), and sets
//     kappa = |s| < 1e-4 ? 0.25f : tanhf(0.5f s) / (2 s),   sq = sqrtf(w kappa),   pe = p - 0.5f w;
// a Frobenius side's piece of the same launch keeps sq = sqrtf(w), pe = p (logit0 / logit1: uniform over the workgroup).  The
// reweighting sits in `stage`, not in `gather`: the loads of gather(tl + 2) stay in flight across the MFMAs of step tl, and the dot
// waits for them only where the registers are consumed anyway.  Everything else is the one body: LG = false compiles to the kernel
// without any of this, so a fit without a logistic relation pays nothing for it.  It takes sqrtf(w) in `gather`: taken in `stage`,
// as the logistic instance must, the Frobenius pass measured 0.4 % (C5, k = 256) to 1.1 % (k = 64) slower.
// A piece writes its partial H (the blocks it formed) and g to its own scratch slot; als_finish_kernel adds the pieces of a row in
// piece order, mirrors the upper triangle (so H_i is symmetric to the bit), adds S, l2 on the first k diagonal entries and 1 on the
// padding diagonal, and N_i to g.  No atomics anywhere: a repeated call from the same state is bit-identical.  Padding columns of
// the factors are zero, so the padding of H_i and g_i is exact zeros (unit diagonal apart).
#pragma once
#include "cmf_kernels.hip.h"
#include "cmf_als_nnls.hip.h"
#include "cmf_als_cg.hip.h"
#include "cmf_als_nncg.hip.h"
#include "cmf_als_bg.hip.h"

namespace cmfk {

struct AlsSide {
    const int32_t *idx;
    const float *pv, *wv;   // p = w t, w
    const float *B;         // the gathered factor, pitch KP
};
struct AlsPiece {
    int64_t beg;            // first stored entry
    int32_t len;            // entries (1 .. piece length)
    int32_t side;           // 0 | 1: which of the two CSR images of the sweep
    int64_t row;            // of the swept factor
};
struct AlsArgs {
    AlsSide s0, s1;
    const AlsPiece *pieces; // one per workgroup
    float *Hp;              // [piece][KP][KP] partial Hessians (blocks on or above the block diagonal at KP = 256, all blocks below)
    float *gp;              // [piece][KP]
    const float *F;         // LG: the swept factor, pitch KP: the current rows
    int logit0, logit1;     // LG: the side is logistic (1) or Frobenius (0)
};

template <int KP>
struct AlsCfg {
    static constexpr int LPR = KP / 4 < 16 ? KP / 4 : 16;  // lanes per gathered row
    static constexpr int CPT = (KP / 4) / LPR;             // 16-byte chunks of that row per lane (chunk q * LPR + lane)
    static constexpr int WM = KP >= 128 ? 4 : (KP == 64 ? 2 : 1);
    static constexpr int WN = KP >= 64 ? 2 : 1;
    static constexpr int TN = KP == 128 ? 2 : 1;
    static constexpr int TILE = 32 * KP;
};

// wave type 0 / 1 / 2: the symmetric map of k_pad = 256 (above); type 3: block row wm, TN block columns (k_pad < 256)
template <int KP>
__host__ __device__ constexpr int als_nf(int ty) { return ty == 0 ? 5 : (ty == 1 ? 4 : (ty == 2 ? 3 : 1 + AlsCfg<KP>::TN)); }
template <int KP>
__host__ __device__ constexpr int als_np(int ty) { return ty == 0 ? 4 : (ty == 3 ? AlsCfg<KP>::TN : 5); }
__host__ __device__ constexpr int als_ai(int ty, int n) { return ty == 1 ? (n == 4 ? 3 : 0) : (ty == 2 ? (n >= 3 ? 1 : 0) : 0); }
__host__ __device__ constexpr int als_bi(int ty, int n) { return ty == 1 ? (n == 4 ? 3 : n) : (ty == 2 ? (n < 3 ? n : n - 2) : n + 1); }
template <int V>
struct AlsIntC {
    static constexpr int value = V;
};

// kappa(s) = tanh(s / 2) / (2 s), 1/4 at 0 (the guard: tanh(s / 2) / (2 s) = 1/4 - s^2 / 48 + ..., below 2^-24 off 1/4 for |s| < 1e-4)
__device__ __forceinline__ float als_logit_kappa(float s) { return fabsf(s) < 1e-4f ? 0.25f : tanhf(0.5f * s) / (2.0f * s); }

template <int KP, bool LG>
__global__ __launch_bounds__(512) void als_normal_kernel(AlsArgs g) {
    using C = AlsCfg<KP>;
    __shared__ __attribute__((aligned(16))) float sm[2 * C::TILE];
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, lh = lane >> 5;
    const int uw = __builtin_amdgcn_readfirstlane(t >> 6);
    const AlsPiece pc = g.pieces[blockIdx.x];
    const bool second = pc.side != 0;
    const bool logit = LG && (second ? g.logit1 : g.logit0) != 0;   // uniform over the workgroup
    const int32_t *idx = (second ? g.s1.idx : g.s0.idx) + pc.beg;
    const float *pv = (second ? g.s1.pv : g.s0.pv) + pc.beg;
    const float *wv = (second ? g.s1.wv : g.s0.wv) + pc.beg;
    const float *B = second ? g.s1.B : g.s0.B;
    const int ns = pc.len, nt = (ns + 31) >> 5;
    const int trow = t / C::LPR, tl16 = t % C::LPR;
    const bool loader = t < 32 * C::LPR;    // k_pad = 32: half of the threads cover the tile

    f32x4 rr[C::CPT], gacc[C::CPT];
    [[maybe_unused]] f32x4 fr[C::CPT];      // LG: the columns this lane holds of every gathered row, of the current row
    float wq = 0.f, pq = 0.f;               // of the gathered row: p as stored, and w (LG) or its root (the root needs the row under LG)
#pragma unroll
    for (int q = 0; q < C::CPT; ++q) rr[q] = gacc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (LG) {
#pragma unroll
        for (int q = 0; q < C::CPT; ++q) fr[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (logit && loader) {
            const float *src = g.F + pc.row * KP + 4 * tl16;
#pragma unroll
            for (int c = 0; c < C::CPT; ++c) fr[c] = *reinterpret_cast<const f32x4 *>(src + 4 * c * C::LPR);
        }
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
            if constexpr (LG) wq = wv[q];
            else wq = sqrtf(wv[q]);
            pq = pv[q];
        } else {
#pragma unroll
            for (int c = 0; c < C::CPT; ++c) rr[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            wq = 0.f;
            pq = 0.f;
        }
    };
    auto stage = [&](int nb) { // registers -> gradient part and the sqrt(w)-scaled (logistic: sqrt(w kappa)-scaled) LDS image
        float sq = wq, pe = pq;   // LG = false: gather took the root
        if constexpr (LG) {
            if (!logit) {
                sq = sqrtf(wq);
            } else {       // (all lanes: a row past the end of the piece is zeros with w = 0; the lanes of a row's group stay together)
                float d = 0.f;
#pragma unroll
                for (int c = 0; c < C::CPT; ++c) d += rr[c][0] * fr[c][0] + rr[c][1] * fr[c][1] + rr[c][2] * fr[c][2] + rr[c][3] * fr[c][3];
                const float s = group_sum<C::LPR>(d);
                sq = sqrtf(wq * als_logit_kappa(s));
                pe = pq - 0.5f * wq;
            }
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

// H_i = sum of the row's pieces (in piece order) + S + l2 I_k (+ 1 on the padding diagonal), both triangles from the upper one;
// g_i = sum of the pieces + N_i.  first[row] .. first[row + 1] (minus pbase) are the row's slots.  One workgroup per row walks the
// 32 x 32 blocks on or above the block diagonal: a block is read and written along its rows, and its mirror image leaves through a
// 32 x 33 LDS tile, along rows too.
__global__ __launch_bounds__(256) void als_finish_kernel(const float *Hp, const float *gp, const int64_t *first, int64_t pbase, const float *S,
                                                         const float *N, float l2, int k, int kp, float *H, float *g) {
    __shared__ float tl[32][33];
    const int64_t row = blockIdx.x;
    const int64_t p0 = first[row] - pbase, p1 = first[row + 1] - pbase;
    const int64_t kk = (int64_t)kp * kp;
    float *Hr = H + row * kk;
    const int nb = kp >> 5, c = threadIdx.x & 31, r0 = threadIdx.x >> 5;
    for (int ba = 0; ba < nb; ++ba)
        for (int bb = ba; bb < nb; ++bb) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 8 * q, gi = 32 * ba + r, gj = 32 * bb + c;
                const int e = gi * kp + gj;
                float v = 0.f;
                for (int64_t p = p0; p < p1; ++p) v += Hp[p * kk + e];
                if (S) v += S[e];
                if (gi == gj) v += gi < k ? l2 : 1.0f;
                tl[r][c] = v;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 8 * q;
                if (ba == bb) {
                    Hr[(32 * ba + r) * kp + 32 * ba + c] = r <= c ? tl[r][c] : tl[c][r];
                } else {
                    Hr[(32 * ba + r) * kp + 32 * bb + c] = tl[r][c];
                    Hr[(32 * bb + r) * kp + 32 * ba + c] = tl[c][r];
                }
            }
            __syncthreads();
        }
    for (int cc = threadIdx.x; cc < kp; cc += 256) {
        float v = 0.f;
        for (int64_t p = p0; p < p1; ++p) v += gp[p * kp + cc];
        if (N) v += N[row * kp + cc];
        g[row * kp + cc] = v;
    }
}

// F <- the solved rows (projected onto the non-negative orthant where asked) on the valid block; the padding is not written
__global__ void als_apply_kernel(float *F, const float *sol, int64_t rows, int k, int kp, int non_negative) {
    const int64_t n = rows * kp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if ((int)(i % kp) >= k) continue;
        float v = sol[i];
        if (non_negative) v = fmaxf(v, 0.f);
        F[i] = v;
    }
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx)
#ifdef CMF_ALS_HOST

enum { ALS_PIECE_DEFAULT = 4096 };

struct AlsRel { int which; int t; int fb; bool data_trans; }; // relation X | Y, CSR image (0 pattern | 1 transpose), gathered factor, T B as data_times takes it
// the relations a sweep of factor f reads (V: the X side first, as in MU's numerator X^T U + Y Z)
static int als_rels(int f, AlsRel out[2]) {
    if (f == CMF_U) { out[0] = AlsRel{0, 0, CMF_V, false}; return 1; }
    if (f == CMF_Z) { out[0] = AlsRel{1, 1, CMF_V, true}; return 1; }
    out[0] = AlsRel{0, 1, CMF_U, true};
    out[1] = AlsRel{1, 0, CMF_Z, false};
    return 2;
}

// The sweep of factor f as every route reads it: its relations, which of them are observed (CSR weights bound), and the observed
// ones in order with their CSR image and gathered factor.  Built on the host: no launch, no device access.
struct AlsSweep {
    int f, nrel, nobs = 0;
    AlsRel rel[2];
    bool observed[2];                                       // of rel[s]
    struct { const WCsrDev *M; const float *B; } obs[2];   // [nobs]
};
static AlsSweep als_sweep(const cmf_ctx *c, int f) {
    AlsSweep sw;
    sw.f = f;
    sw.nrel = als_rels(f, sw.rel);
    for (int s = 0; s < sw.nrel; ++s) {
        const AlsRel &r = sw.rel[s];
        sw.observed[s] = c->wm_kind[r.which] == WM_CSR;
        if (sw.observed[s]) sw.obs[sw.nobs++] = {&c->wm_sp[r.which][r.t], c->F[r.fb]};
    }
    return sw;
}
static bool als_observed(const AlsSweep &sw) { return sw.nobs > 0; }

#define CMF_ALS_BG_HOST
#include "cmf_als_bg.hip.h"   // background weights: als_shared_terms, als_side_weights and the entry points of its own
static int64_t als_piece_len(const cmf_ctx *c) { return c->opt_als_piece > 0 ? rup(c->opt_als_piece, 32) : (int64_t)ALS_PIECE_DEFAULT; }

enum AlsRoute { ALS_SHARED_EXACT, ALS_SHARED_HALS, ALS_ROWS_EXACT, ALS_ROWS_NNLS, ALS_ROWS_CG };
// the route of one sweep (file header); nn: the factor is non-negative, sweeps / cg_steps: 0 where the entry point has no such count
static AlsRoute als_route(bool observed, bool nn, int sweeps, int cg_steps) {
    if (nn && sweeps) return observed ? ALS_ROWS_NNLS : ALS_SHARED_HALS;
    if (!observed) return ALS_SHARED_EXACT;
    return !nn && cg_steps ? ALS_ROWS_CG : ALS_ROWS_EXACT;
}

// The launch ladder of the row kernels, templates on k_pad: LAUNCH is a statement that names the instance of cmfk::KERNEL as `kern`;
// what follows LAUNCH are the kernel's template arguments behind k_pad.
#define ALS_LAUNCH_KP(c, KERNEL, WHAT, LAUNCH, ...)                                                                      \
    switch ((c)->kp) {                                                                                                   \
    case 32: { auto kern = cmfk::KERNEL<32, ##__VA_ARGS__>; LAUNCH; break; }                                             \
    case 64: { auto kern = cmfk::KERNEL<64, ##__VA_ARGS__>; LAUNCH; break; }                                             \
    case 128: { auto kern = cmfk::KERNEL<128, ##__VA_ARGS__>; LAUNCH; break; }                                           \
    case 256: { auto kern = cmfk::KERNEL<256, ##__VA_ARGS__>; LAUNCH; break; }                                           \
    default: return fail(CMF_EUNSUPPORTED, WHAT " built for n_components <= 256 (k_pad = %d)", (c)->kp);                 \
    }                                                                                                                    \
    HIPCHK(hipGetLastError())

// The ladder of the lane-group kernels, templates on GL = k_pad / 4 lanes per factor row (k_pad <= 256: the entry points' check);
// what follows KERNEL are hipLaunchKernelGGL's arguments behind the kernel.
#define ALS_LAUNCH_GL(c, KERNEL, ...)                                                                                    \
    switch ((c)->kp) {                                                                                                   \
    case 32: hipLaunchKernelGGL((cmfk::KERNEL<8>), __VA_ARGS__); break;                                                  \
    case 64: hipLaunchKernelGGL((cmfk::KERNEL<16>), __VA_ARGS__); break;                                                 \
    case 128: hipLaunchKernelGGL((cmfk::KERNEL<32>), __VA_ARGS__); break;                                                \
    default: hipLaunchKernelGGL((cmfk::KERNEL<64>), __VA_ARGS__); break;                                                 \
    }

// Rows 0 .. nrows of `nip` CSR images (ip[s]: the rows' indptr) cut into pieces of at most L stored entries: row by row, within a row
// image by image, piece(r, s, beg, len) per piece in that order.  Returns first[r], the pieces before row r ([nrows + 1]).
template <class Piece>
static std::vector<int64_t> als_cut_rows(const std::vector<int64_t> *ip, int nip, int64_t nrows, int64_t L, Piece piece) {
    std::vector<int64_t> first((size_t)nrows + 1, 0);
    int64_t n = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        first[(size_t)r] = n;
        for (int s = 0; s < nip; ++s) {
            const int64_t e = ip[s][(size_t)r + 1];
            for (int64_t q = ip[s][(size_t)r]; q < e; q += L, ++n) piece(r, s, q, (int32_t)std::min(L, e - q));
        }
    }
    first[(size_t)nrows] = n;
    return first;
}

static int als_relation_ok(cmf_ctx *c, const char *what, int which) {
    if (c->wm_kind[which] == WM_DENSE)
        return fail(CMF_EUNSUPPORTED, "%s: %s has DENSE weights bound; ALS takes weights as the CSR pattern of the observed entries (cmf_set_weighted_csr)",
                    what, which == 0 ? "X" : "Y");
    if (c->wm_kind[which] != WM_CSR && !have_data(c, which))
        return fail(CMF_EINVAL, "%s: %s has neither data nor CSR weights", what, which == 0 ? "X" : "Y");
    return CMF_OK;
}

// indptr[r0 .. r1] of every observed side back to the host (the pattern lives on the device only): the row lengths behind the
// piece plan and behind the capacity classes of the CG rows
static int als_fetch_indptr(cmf_ctx *c, const AlsSweep &sw, int64_t r0, int64_t r1, std::vector<int64_t> ip[2]) {
    for (int s = 0; s < sw.nobs; ++s) {
        ip[s].assign((size_t)(r1 - r0 + 1), 0);
        HIPCHK(hipMemcpyAsync(ip[s].data(), sw.obs[s].M->indptr + r0, ip[s].size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return CMF_OK;
}

struct AlsPlan { // the pieces of rows [r0, r1) of one sweep, host side
    std::vector<cmfk::AlsPiece> pieces;
    std::vector<int64_t> first;   // [r1 - r0 + 1]
};
static int als_plan(cmf_ctx *c, const AlsSweep &sw, int64_t r0, int64_t r1, AlsPlan &pl) {
    const int64_t L = als_piece_len(c);
    std::vector<int64_t> ip[2];
    CHK(als_fetch_indptr(c, sw, r0, r1, ip));
    pl.pieces.clear();
    pl.first = als_cut_rows(ip, sw.nobs, r1 - r0, L, [&](int64_t r, int s, int64_t beg, int32_t len) {
        pl.pieces.push_back(cmfk::AlsPiece{beg, len, s, r0 + r});
    });
    return CMF_OK;
}

#include "cmf_als_logit.hip.h"   // relation losses: als_logit_rel, als_logit_sweep, als_logit_check, the loss kernel and the entry points of its own

// lg: the sweep reads a logistic relation (a.F, a.logit0 / logit1 are set): the instance with the reweighting, and its dot products
static int als_launch_normal(cmf_ctx *c, const cmfk::AlsArgs &a, int64_t npieces, int64_t nnz, bool lg) {
    if (npieces <= 0) return CMF_OK;
    Timed tm(c, CMF_K_ROWHESS, 2.0 * (double)nnz * c->k * c->k + (lg ? 2.0 * (double)nnz * c->k : 0.0));
    const dim3 grid((unsigned)npieces), block(512);
    if (lg) {
        ALS_LAUNCH_KP(c, als_normal_kernel, "ALS normal equations are", hipLaunchKernelGGL(kern, grid, block, 0, c->stream, a), true);
    } else {
        ALS_LAUNCH_KP(c, als_normal_kernel, "ALS normal equations are", hipLaunchKernelGGL(kern, grid, block, 0, c->stream, a), false);
    }
    return CMF_OK;
}

static int als_nnls_launch(cmf_ctx *c, const float *H, const float *g, float *F, const int64_t *first, int64_t nrows, int sweeps) {
    if (nrows <= 0) return CMF_OK;
    cmfk::NnlsArgs a;
    a.H = H; a.g = g; a.F = F; a.first = first; a.nrows = nrows; a.k = c->k; a.sweeps = sweeps;
    Timed tm(c, CMF_K_HALS, 2.0 * (double)nrows * c->k * c->k * sweeps);
    const dim3 grid((unsigned)((nrows + cmfk::NNLS_WAVES - 1) / cmfk::NNLS_WAVES)), block(64 * cmfk::NNLS_WAVES);
    ALS_LAUNCH_KP(c, als_nnls_kernel, "the non-negative row solve is", hipLaunchKernelGGL(kern, grid, block, 0, c->stream, a));
    return CMF_OK;
}

// The finished systems of rows [row0, row0 + nr) as als_chunks hands them on: H [nr][k_pad][k_pad] (c->als_h), g [nr][k_pad] (those
// rows of c->als_g), and the piece index of those rows (no pieces: a row without information), null where S gives every row a system.
struct AlsChunk { int64_t row0, nr; float *H; const float *g; const int64_t *no_info; };

// Rows [r_begin, r_end) of the sweep in per-row form, chunk by chunk: als_normal_kernel over the chunk's pieces, als_finish_kernel,
// then use(chunk).  A chunk holds at most `cap` rows and (but for a single row) as many pieces.
template <class Use>
static int als_chunks(cmf_ctx *c, const AlsSweep &sw, double l2, int64_t r_begin, int64_t r_end, int64_t cap, Use use) {
    using namespace cmfk;
    const int kp = c->kp;
    const int64_t kk = (int64_t)kp * kp, rows_pad = c->frows_pad[sw.f];
    // the full relation: its Gram into every row's matrix, its product into the right-hand sides; a background: c0 times the Gram
    const float *S = nullptr, *N = nullptr;
    CHK(als_shared_terms(c, sw, &S, &N));
    AlsPlan pl;
    CHK(als_plan(c, sw, r_begin, r_end, pl));
    const bool lg = als_logit_sweep(c, sw);   // a sweep that reads a logistic relation: the LG = true instance of als_normal_kernel
    const int64_t nrows = r_end - r_begin;
    int64_t max_rows = 0, max_pieces = 0;
    std::vector<int64_t> cuts{0};
    for (int64_t r = 0; r < nrows;) {
        int64_t e = r;
        while (e < nrows && e - r < cap && (e == r || pl.first[(size_t)e + 1] - pl.first[(size_t)r] <= cap)) ++e;
        max_rows = std::max(max_rows, e - r);
        max_pieces = std::max(max_pieces, pl.first[(size_t)e] - pl.first[(size_t)r]);
        cuts.push_back(e);
        r = e;
    }
    CHK(ensure_scratch(c, c->als_h, (size_t)std::max<int64_t>(1, max_rows) * kk * sizeof(float)));
    CHK(ensure_scratch(c, c->als_part, (size_t)std::max<int64_t>(1, max_pieces) * (kk + kp) * sizeof(float)));
    CHK(ensure_scratch(c, c->als_g, (size_t)rows_pad * kp * sizeof(float)));
    const size_t pbytes = std::max<size_t>(16, pl.pieces.size() * sizeof(AlsPiece)), fbytes = pl.first.size() * sizeof(int64_t);
    CHK(ensure_scratch(c, c->als_desc, pbytes + fbytes));
    AlsPiece *dpieces = (AlsPiece *)c->als_desc.p;
    int64_t *dfirst = (int64_t *)((char *)c->als_desc.p + pbytes);
    if (!pl.pieces.empty()) HIPCHK(hipMemcpyAsync(dpieces, pl.pieces.data(), pl.pieces.size() * sizeof(AlsPiece), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dfirst, pl.first.data(), fbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vectors may go

    AlsArgs a;
    memset(&a, 0, sizeof a);
    for (int s = 0; s < sw.nobs; ++s) {
        const WCsrDev &M = *sw.obs[s].M;
        (s == 0 ? a.s0 : a.s1) = AlsSide{M.idx, als_side_targets(M), als_side_weights(M), sw.obs[s].B};
    }
    float *Hc = (float *)c->als_h.p, *Hp = (float *)c->als_part.p, *grad = (float *)c->als_g.p;
    a.Hp = Hp;
    a.gp = Hp + std::max<int64_t>(1, max_pieces) * kk;
    if (lg) {
        a.F = c->F[sw.f];
        for (int s = 0, o = 0; s < sw.nrel; ++s)
            if (sw.observed[s]) (o++ == 0 ? a.logit0 : a.logit1) = als_logit_rel(c, sw.rel[s].which) ? 1 : 0;
    }
    for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
        const int64_t c0 = cuts[ci], c1 = cuts[ci + 1], nr = c1 - c0, row0 = r_begin + c0;
        const int64_t pbase = pl.first[(size_t)c0], np = pl.first[(size_t)c1] - pbase;
        a.pieces = dpieces + pbase;
        int64_t nnz = 0;
        for (int64_t p = pbase; p < pbase + np; ++p) nnz += pl.pieces[(size_t)p].len;
        CHK(als_launch_normal(c, a, np, nnz, lg));
        {
            Timed tm(c, CMF_K_ELEMWISE);
            hipLaunchKernelGGL(als_finish_kernel, dim3((unsigned)nr), dim3(256), 0, c->stream, (const float *)Hp, (const float *)a.gp, (const int64_t *)(dfirst + c0),
                               pbase, S, N ? N + row0 * kp : nullptr, (float)l2, c->k, kp, Hc, grad + row0 * kp);
            HIPCHK(hipGetLastError());
        }
        CHK(use(AlsChunk{row0, nr, Hc, grad + row0 * kp, S ? nullptr : dfirst + c0}));
    }
    return CMF_OK;
}

// What safe_solve_rows (cmf_newton.hip.h) reads and writes of the Newton step's state: put back when the scope ends.
struct AlsNewtonStateGuard {
    cmf_ctx *const c;
    const bool psd;
    const int64_t rank1, eig;
    std::vector<int> bad;
    explicit AlsNewtonStateGuard(cmf_ctx *ctx) : c(ctx), psd(ctx->hess_psd), rank1(ctx->rank1_rows), eig(ctx->eig_clamp_rows) { bad.swap(c->bad_host); }
    ~AlsNewtonStateGuard() { c->hess_psd = psd; c->rank1_rows = rank1; c->eig_clamp_rows = eig; c->bad_host.swap(bad); }
};

// rows exact: the Cholesky solves of every chunk into c->als_sol -- the plain route of the per-row Newton sweeps
static int als_rows_solve(cmf_ctx *c, const AlsSweep &sw, double l2) {
    CHK(ensure_scratch(c, c->als_sol, (size_t)c->frows_pad[sw.f] * c->kp * sizeof(float)));
    // the threshold of that route, well below l2 <= lambda_min(H_i): its test (a Cholesky of H_i - pert I whose pivots must exceed
    // 4e-6 max H_jj) passes unless cond(H_i) is above ~2e5, where a float32 factorisation has nothing left to give
    const double pert = l2 / 16.0;
    return als_chunks(c, sw, l2, 0, c->frows[sw.f], hessian_chunk_rows(c, c->frows_pad[sw.f]), [&](const AlsChunk &ch) -> int {
        AlsNewtonStateGuard keep(c);
        c->hess_psd = true;
        return safe_solve_rows(c, ch.H, ch.g, (float *)c->als_sol.p + ch.row0 * c->kp, ch.nr, c->k, c->kp, pert);
    });
}

// rows NNLS: `sweeps` coordinate-descent sweeps of every chunk's rows of F, in place (the gathered factors are the other ones: the
// chunks to come do not read the rows written here)
static int als_rows_nnls(cmf_ctx *c, const AlsSweep &sw, double l2, int sweeps) {
    return als_chunks(c, sw, l2, 0, c->frows[sw.f], hessian_chunk_rows(c, c->frows_pad[sw.f]), [&](const AlsChunk &ch) -> int {
        return als_nnls_launch(c, ch.H, ch.g, c->F[sw.f] + ch.row0 * c->kp, ch.no_info, ch.nr, sweeps);
    });
}

// cmf_als_normal: the finished systems of rows [r_begin, r_end), one chunk, back to the host
static int als_rows_to_host(cmf_ctx *c, const AlsSweep &sw, double l2, int64_t r_begin, int64_t r_end, float *host_H, float *host_g) {
    return als_chunks(c, sw, l2, r_begin, r_end, INT64_MAX, [&](const AlsChunk &ch) -> int {
        if (host_H) HIPCHK(hipMemcpyAsync(host_H, ch.H, (size_t)ch.nr * c->kp * c->kp * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (host_g) HIPCHK(hipMemcpyAsync(host_g, ch.g, (size_t)ch.nr * c->kp * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return CMF_OK;
    });
}

static int als_apply(cmf_ctx *c, int f, const float *sol, bool nn) {
    return launch_ew(c, cmfk::als_apply_kernel, c->frows[f] * c->kp, c->F[f], sol, c->frows[f], c->k, c->kp, nn ? 1 : 0);
}

// shared exact: F <- clamp(N (G + l2 I)^-1), the inverse formed once in float64
static int als_sweep_shared(cmf_ctx *c, const AlsSweep &sw, double l2, bool nn) {
    CHK(ensure_shared64(c));
    for (int s = 0; s < sw.nrel; ++s) {
        const AlsRel &r = sw.rel[s];
        CHK(gram64(c, c->F[r.fb], c->frows_pad[r.fb], (double *)(s == 0 ? c->g64a.p : c->g64b.p), nullptr));
        CHK(data_times(c, r.which, r.data_trans, c->F[r.fb], c->num, s > 0));
    }
    CHK(launch_hess64(c, (const double *)c->g64a.p, 1.0, sw.nrel > 1 ? (const double *)c->g64b.p : nullptr, 1.0, l2));
    const int rc = shared_inverse64(c, (const double *)c->h64.p, c->k, 0.5 * l2, true);
    if (rc == CMF_EUNSUPPORTED) return fail(CMF_EHIP, "cmf_als_step: the float64 inverse of G + l2 I failed (non-finite factors?)");
    CHK(rc);
    CHK(gemm(c, MODE_NN, c->num, c->kp, c->Hinv, c->kp, c->den, c->frows_pad[sw.f], c->kp, c->kp));
    return als_apply(c, sw.f, c->den, nn);
}

static int als_check(cmf_ctx *c, const char *what, double l2, int mask) {
    if (!(l2 > 0.0) || !std::isfinite(l2)) return fail(CMF_EINVAL, "%s: l2 must be positive (a row with fewer than k observations is singular otherwise), got %g", what, l2);
    if (mask <= 0 || mask > 7) return fail(CMF_EINVAL, "%s: update_mask must name at least one of U, V, Z (got %d)", what, mask);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: n_components <= 256 only (k_pad = %d)", what, c->kp);
    CHK(als_logit_check(c, what, mask));
    if (mask & (CMF_UPD_U | CMF_UPD_V)) CHK(als_relation_ok(c, what, 0));
    if (mask & (CMF_UPD_Z | CMF_UPD_V)) CHK(als_relation_ok(c, what, 1));
    return CMF_OK;
}

// shared HALS: N and G as cmf_hals_step forms them, `sweeps` passes of hals_sweep
static int als_nnls_sweep_shared(cmf_ctx *c, int f, double l2, int sweeps) {
    const float *N = c->num, *G = c->G2;
    if (f == CMF_V) {
        CHK(cmf_mu_v_partials(c, c->vbuf));
        N = c->vbuf;
        G = c->vbuf + c->dp * c->kp;
    } else {
        CHK(gram32(c, c->F[CMF_V], c->dp, c->G2));
        CHK(data_times(c, f == CMF_U ? 0 : 1, f == CMF_Z, c->F[CMF_V], c->num));
    }
    for (int s = 0; s < sweeps; ++s) CHK(hals_sweep(c, f, N, G, 0.0, l2));
    return CMF_OK;
}

enum { ALS_CG_LDS_TOTAL = 156 * 1024, ALS_CG_CLASSES = 4 };   // (156 KB: the largest dynamic LDS any kernel here asks for)
// bytes of dynamic LDS the gathered rows of one row may take ("als_cg_lds": 0 every row streams; at most what is left of 156 KB).
// The default leaves room for four workgroups per CU: measured on C5's pattern at k_pad = 256, rows of 100 entries resident at one
// workgroup per CU take twice the time of the same rows gathered again in every pass at eight.
static int64_t als_cg_lds_bytes(const cmf_ctx *c) {
    const int64_t fixed = 4 * (int64_t)cmfk::als_cg_fixed_floats(c->kp);
    return c->opt_als_cg_lds < 0 ? ALS_CG_LDS_TOTAL / 4 - fixed : std::min<int64_t>(c->opt_als_cg_lds, ALS_CG_LDS_TOTAL - fixed);
}

static int als_cg_launch(cmf_ctx *c, const cmfk::AlsCgArgs &a, int64_t nrows) {
    if (nrows <= 0) return CMF_OK;
    const size_t lds = 4 * (size_t)cmfk::als_cg_fixed_floats(c->kp) + (size_t)a.cap * cmfk::als_cg_entry_bytes(c->kp);
    const dim3 grid((unsigned)nrows), block(256);
    ALS_LAUNCH_KP(c, als_cg_kernel, "the conjugate-gradient row solve is",
                  CHK(allow_big_lds(c, (const void *)kern, ALS_CG_LDS_TOTAL)); hipLaunchKernelGGL(kern, grid, block, lds, c->stream, a));
    return CMF_OK;
}

enum { ALS_CG_PIECE_DEFAULT = 2048 };   // the fastest of 2048, 4096, 16384 and 65536 on the V sweep of C5 Zipf at k = 256
// entries per piece of a long row of the CG route ("als_cg_piece": > 0 rounded up to 16; 0 the default; < 0 no row is ever cut)
static int64_t als_cg_piece_len(const cmf_ctx *c) {
    if (c->opt_als_cg_piece < 0) return INT64_MAX;
    return c->opt_als_cg_piece > 0 ? rup(c->opt_als_cg_piece, 16) : (int64_t)ALS_CG_PIECE_DEFAULT;
}

// the long rows of a sweep: 2 (steps + 1) launches, pieces then combine, once for r = g - H f and once per step
static int als_cg_long_rows(cmf_ctx *c, cmfk::AlsCgPieceArgs &a, int64_t nlong, int64_t npieces, int steps) {
    if (nlong <= 0) return CMF_OK;
    const dim3 pgrid((unsigned)npieces), cgrid((unsigned)nlong), block(256);
    for (int s = 0; s <= steps; ++s) {
        a.phase = s == 0 ? 0 : (s == steps ? 2 : 1);
        ALS_LAUNCH_KP(c, als_cg_piece_kernel, "the conjugate-gradient row solve is", hipLaunchKernelGGL(kern, pgrid, block, 0, c->stream, a));
        ALS_LAUNCH_KP(c, als_cg_combine_kernel, "the conjugate-gradient row solve is", hipLaunchKernelGGL(kern, cgrid, block, 0, c->stream, a));
    }
    return CMF_OK;
}

// The launches of the non-negative rows (cmf_als_nncg.hip.h) behind the plan of als_cg_rows: one launch per capacity class, then the
// long rows -- 2 launches for r = g - H f and 4 per step (piece, combine A, piece, combine B).  The passes every row ran stay on the
// device; they come back (4 bytes a row) only for cmf_als_nncg_passes, or with kernel timing on, behind the timed stretch, to charge
// 4 len k flops per pass (+ 2 k^2 with a full side): a sweep without either waits for nothing.
static int als_nncg_count(cmf_ctx *c) {
    if (c->als_nncg_counted) return CMF_OK;
    const size_t n = c->als_nncg_lens.size();
    std::vector<int32_t> passes(n, 0);
    if (n) {
        HIPCHK(hipMemcpyAsync(passes.data(), c->als_nncg_passes.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    int64_t total = 0, entry_passes = 0;
    for (size_t r = 0; r < n; ++r) {
        total += passes[r];
        entry_passes += (int64_t)c->als_nncg_lens[r] * passes[r];
    }
    c->als_nncg_last[2] = total;
    c->als_nncg_last[3] = entry_passes;
    c->als_nncg_counted = true;
    return CMF_OK;
}

static int als_nncg_launches(cmf_ctx *c, const cmfk::AlsCgArgs &a, const std::vector<int64_t> *ip, int nobs, const std::vector<int64_t> *list,
                             const int64_t *caps, const int64_t *drows, const cmfk::AlsCgLongRow *dlongs, const cmfk::AlsCgPiece *dpieces,
                             const std::vector<cmfk::AlsCgLongRow> &longs, int64_t npieces, int64_t nrows) {
    using namespace cmfk;
    const int kp = c->kp, steps = a.steps;
    const size_t nl = longs.size();
    CHK(ensure_scratch(c, c->als_nncg_passes, (size_t)nrows * sizeof(int32_t)));
    HIPCHK(hipMemsetAsync(c->als_nncg_passes.p, 0, (size_t)nrows * sizeof(int32_t), c->stream));
    AlsNncgArgs na;
    na.a = a;
    na.passes = (int32_t *)c->als_nncg_passes.p;
    AlsNncgLongArgs pa;
    memset(&pa, 0, sizeof pa);
    if (nl) {   // scratch of the long rows: state [5][k_pad] per row | partials [k_pad] per piece | a record per row
        const size_t sfloats = (5 * nl + (size_t)npieces) * (size_t)kp;
        CHK(ensure_scratch(c, c->als_cg_long, sfloats * sizeof(float) + nl * sizeof(AlsNncgRow)));
        pa.s0 = a.s0; pa.s1 = a.s1;
        pa.pieces = dpieces; pa.rows = dlongs;
        pa.S = a.S; pa.N = a.N; pa.Fin = a.Fin; pa.Fout = a.Fout; pa.out_row0 = a.out_row0;
        pa.state = (float *)c->als_cg_long.p;
        pa.partial = pa.state + 5 * nl * (size_t)kp;
        pa.info = (AlsNncgRow *)(pa.state + sfloats);
        pa.passes = na.passes;
        pa.l2 = a.l2; pa.k = a.k;
    }
    c->als_nncg_lens.assign((size_t)nrows, 0);
    for (int64_t r = 0; r < nrows; ++r)
        for (int s = 0; s < nobs; ++s) c->als_nncg_lens[(size_t)r] += (int32_t)(ip[s][(size_t)r + 1] - ip[s][(size_t)r]);
    c->als_nncg_counted = false;
    bool timed = false;
    {
        Timed tm(c, CMF_K_ROWHESS, 0.0);
        timed = tm.on;
        int64_t done = 0;
        for (int q = 0; q <= ALS_CG_CLASSES; ++q) {
            const int64_t n = (int64_t)list[q].size();
            na.a.rows = drows + done;
            na.a.cap = (int)caps[q];
            done += n;
            if (n <= 0) continue;
            const size_t lds = 4 * (size_t)als_cg_fixed_floats(kp) + (size_t)na.a.cap * als_cg_entry_bytes(kp);
            const dim3 grid((unsigned)n), block(256);
            ALS_LAUNCH_KP(c, als_nncg_kernel, "the non-negative conjugate-gradient row solve is",
                          CHK(allow_big_lds(c, (const void *)kern, ALS_CG_LDS_TOTAL)); hipLaunchKernelGGL(kern, grid, block, lds, c->stream, na));
        }
        if (nl) {
            const dim3 pgrid((unsigned)npieces), cgrid((unsigned)nl), block(256);
            for (int s = 0; s <= 2 * steps; ++s) {
                pa.stage = s == 0 ? 0 : 2 - (s & 1);
                pa.last = s == 2 * steps ? 1 : 0;
                ALS_LAUNCH_KP(c, als_nncg_piece_kernel, "the non-negative conjugate-gradient row solve is", hipLaunchKernelGGL(kern, pgrid, block, 0, c->stream, pa));
                ALS_LAUNCH_KP(c, als_nncg_combine_kernel, "the non-negative conjugate-gradient row solve is", hipLaunchKernelGGL(kern, cgrid, block, 0, c->stream, pa));
            }
        }
    }
    if (timed) {   // (the scope has recorded its events: the read-back is not in the timed stretch)
        CHK(als_nncg_count(c));
        c->pending.back().flops = 4.0 * (double)c->als_nncg_last[3] * c->k + (a.S ? 2.0 * (double)c->als_nncg_last[2] * c->k * c->k : 0.0);
    }
    return CMF_OK;
}

// rows CG: rows [r_begin, r_end) of the sweep (which has an observed relation) by `steps` CG steps from the rows of c->F[f];
// row r goes to Fout + (r - out_row0) * k_pad (in place: Fout = c->F[f], out_row0 = 0 -- the gathered factors are the other ones).
// The rows are sorted into capacity classes by their stored entries: capacity / 8, / 4, / 2 and the whole capacity keep the
// gathered rows in LDS (shorter rows: more workgroups per CU), longer rows stream; one launch per class.  A row with more than
// als_cg_piece_len entries goes to none of them: it is cut into pieces (cmf_als_cg.hip.h), all such rows of the sweep together.
// nn: the non-negative rows of cmf_als_nncg.hip.h instead (the same classes, the same pieces; the passes every row ran come back to
// the host, which charges the passes actually run).
static int als_cg_rows(cmf_ctx *c, const AlsSweep &sw, double l2, int64_t r_begin, int64_t r_end, int steps, float *Fout, int64_t out_row0, bool nn = false) {
    using namespace cmfk;
    const char *what = nn ? "cmf_als_nncg_step" : "cmf_als_cg_step";
    const int kp = c->kp;
    const int64_t nrows = r_end - r_begin;
    AlsCgArgs a;
    memset(&a, 0, sizeof a);
    CHK(als_shared_terms(c, sw, &a.S, &a.N)); // as als_chunks
    std::vector<int64_t> ip[2];
    CHK(als_fetch_indptr(c, sw, r_begin, r_end, ip));
    for (int s = 0; s < sw.nobs; ++s) {
        const WCsrDev &M = *sw.obs[s].M;
        (s == 0 ? a.s0 : a.s1) = AlsCgSide{M.indptr, M.idx, als_side_targets(M), als_side_weights(M), sw.obs[s].B};
    }
    const int64_t cap_max = als_cg_lds_bytes(c) / als_cg_entry_bytes(kp);
    int64_t caps[ALS_CG_CLASSES + 1];
    for (int q = 0; q < ALS_CG_CLASSES; ++q) caps[q] = cap_max >> (ALS_CG_CLASSES - 1 - q);
    caps[ALS_CG_CLASSES] = 0;                                   // the streamed class
    const int64_t L = als_cg_piece_len(c);
    std::vector<int64_t> list[ALS_CG_CLASSES + 1];
    std::vector<AlsCgLongRow> longs;
    std::vector<AlsCgPiece> pieces;
    int64_t nnz = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        int64_t len = 0;
        for (int s = 0; s < sw.nobs; ++s) len += ip[s][(size_t)r + 1] - ip[s][(size_t)r];
        if (len > INT32_MAX) return fail(CMF_EUNSUPPORTED, "%s: a row with more than 2^31 - 1 stored entries", what);
        nnz += len;
        if (len > L) {
            const int64_t np = (len + L - 1) / L;
            if ((int64_t)pieces.size() + np > INT32_MAX) return fail(CMF_EUNSUPPORTED, "%s: more than 2^31 - 1 pieces of long rows (als_cg_piece too small)", what);
            const int32_t slot = (int32_t)longs.size();
            longs.push_back(AlsCgLongRow{r_begin + r, (int32_t)pieces.size(), (int32_t)np});
            for (int64_t q = 0; q < len; q += L) pieces.push_back(AlsCgPiece{slot, (int32_t)q, (int32_t)std::min(L, len - q), 0});
            continue;
        }
        int q = 0;
        while (q < ALS_CG_CLASSES && len > caps[q]) ++q;
        list[q].push_back(r_begin + r);
    }
    int64_t *last = nn ? c->als_nncg_last : c->als_cg_last;
    last[0] = (int64_t)longs.size();
    last[1] = (int64_t)pieces.size();
    std::vector<int64_t> all;
    all.reserve((size_t)nrows);
    for (int q = 0; q <= ALS_CG_CLASSES; ++q) all.insert(all.end(), list[q].begin(), list[q].end());
    // descriptors, once per sweep: the rows of the class launches | the long rows | their pieces
    const size_t rbytes = std::max<size_t>(16, all.size() * sizeof(int64_t)), lbytes = longs.size() * sizeof(AlsCgLongRow);
    CHK(ensure_scratch(c, c->als_desc, rbytes + lbytes + pieces.size() * sizeof(AlsCgPiece)));
    int64_t *drows = (int64_t *)c->als_desc.p;
    AlsCgLongRow *dlongs = (AlsCgLongRow *)((char *)c->als_desc.p + rbytes);
    AlsCgPiece *dpieces = (AlsCgPiece *)((char *)dlongs + lbytes);
    if (!all.empty()) HIPCHK(hipMemcpyAsync(drows, all.data(), all.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (!longs.empty()) {
        HIPCHK(hipMemcpyAsync(dlongs, longs.data(), lbytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dpieces, pieces.data(), pieces.size() * sizeof(AlsCgPiece), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vectors may go
    a.Fin = c->F[sw.f];
    a.Fout = Fout;
    a.out_row0 = out_row0;
    a.l2 = (float)l2;
    a.k = c->k;
    a.steps = steps;
    if (nn) return als_nncg_launches(c, a, ip, sw.nobs, list, caps, drows, dlongs, dpieces, longs, (int64_t)pieces.size(), nrows);
    AlsCgPieceArgs pa;
    memset(&pa, 0, sizeof pa);
    if (!longs.empty()) {   // scratch of the long rows: state [3][k_pad] per row | partials [k_pad] per piece | r.r | alive flags
        const size_t nl = longs.size(), sfloats = (3 * nl + pieces.size()) * (size_t)kp;
        CHK(ensure_scratch(c, c->als_cg_long, (sfloats + 2 * nl) * sizeof(float)));
        pa.s0 = a.s0; pa.s1 = a.s1;
        pa.pieces = dpieces; pa.rows = dlongs;
        pa.S = a.S; pa.N = a.N; pa.Fin = a.Fin; pa.Fout = Fout; pa.out_row0 = out_row0;
        pa.state = (float *)c->als_cg_long.p;
        pa.partial = pa.state + 3 * nl * (size_t)kp;
        pa.rr = pa.state + sfloats;
        pa.alive = (int32_t *)(pa.rr + nl);
        pa.l2 = a.l2; pa.k = a.k;
    }
    Timed tm(c, CMF_K_ROWHESS, (4.0 * (double)nnz * c->k + (a.S ? 2.0 * (double)nrows * c->k * c->k : 0.0)) * (steps + 1));
    int64_t done = 0;
    for (int q = 0; q <= ALS_CG_CLASSES; ++q) {
        a.rows = drows + done;
        a.cap = (int)caps[q];
        CHK(als_cg_launch(c, a, (int64_t)list[q].size()));
        done += (int64_t)list[q].size();
    }
    return als_cg_long_rows(c, pa, (int64_t)longs.size(), (int64_t)pieces.size(), steps);
}

// cmf_als_dual.hip.h: under the permission of cmf_als_dual_step an ELIGIBLE sweep on the exact row route (no shared term, no logistic
// relation) solves its rows of few stored entries in dual form and sets *taken; otherwise nothing is launched and *taken is false
static int als_dual_sweep(cmf_ctx *c, const AlsSweep &sw, double l2, bool nn, bool *taken);

// sweeps == 0: the solved rows of the factors in nn_mask are projected; sweeps > 0: those factors are swept by coordinate descent;
// cg_steps > 0: a signed factor with an observed relation runs that many CG steps per row instead of the exact solves;
// nn_cg_steps > 0: a non-negative factor with an observed relation runs that many projected CG steps per row (cmf_als_nncg.hip.h)
static int als_step(cmf_ctx *c, double l2, int nn_mask, int mask, int sweeps, int cg_steps = 0, int nn_cg_steps = 0) {
    DeviceGuard dg(c->device);
    const int bits[3] = {CMF_UPD_V, CMF_UPD_U, CMF_UPD_Z}, fs[3] = {CMF_V, CMF_U, CMF_Z}; // sweep order V, U, Z (cmf_solvers.py:248-263)
    const int nnb[3] = {CMF_NN_V, CMF_NN_U, CMF_NN_Z};
    for (int s = 0; s < 3; ++s) {
        const int f = fs[s];
        if (!(mask & bits[s]) || c->frows[f] <= 0) continue;
        const bool nn = (nn_mask & nnb[s]) != 0;
        const AlsSweep sw = als_sweep(c, f);
        if (nn && nn_cg_steps && als_observed(sw)) {
            CHK(als_cg_rows(c, sw, l2, 0, c->frows[f], nn_cg_steps, c->F[f], 0, true));
            continue;
        }
        switch (als_route(als_observed(sw), nn, sweeps, cg_steps)) {
        case ALS_SHARED_EXACT: CHK(als_sweep_shared(c, sw, l2, nn)); break;
        case ALS_SHARED_HALS: CHK(als_nnls_sweep_shared(c, f, l2, sweeps)); break;
        case ALS_ROWS_NNLS: CHK(als_rows_nnls(c, sw, l2, sweeps)); break;
        case ALS_ROWS_CG: CHK(als_cg_rows(c, sw, l2, 0, c->frows[f], cg_steps, c->F[f], 0)); break;
        case ALS_ROWS_EXACT: {
            bool dual = false;   // under cmf_als_dual_step's permission an eligible sweep solves its short rows in dual form
            CHK(als_dual_sweep(c, sw, l2, nn, &dual));
            if (dual) break;
            CHK(als_rows_solve(c, sw, l2));
            CHK(als_apply(c, f, (const float *)c->als_sol.p, nn));
            break;
        }
        }
    }
    return CMF_OK;
}

extern "C" int cmf_als_step(cmf_ctx *c, double l2, int nn_mask, int mask) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_step", l2, mask));
    return als_step(c, l2, nn_mask, mask, 0);
}

// the range of a sweep or step count: lo .. 1024
static int als_count_ok(const char *what, const char *name, int n, int lo = 1) {
    if (n < lo || n > 1024) return fail(CMF_EINVAL, "%s: %s must be %d .. 1024, got %d", what, name, lo, n);
    return CMF_OK;
}

extern "C" int cmf_als_nnls_step(cmf_ctx *c, double l2, int nn_mask, int mask, int sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_nnls_step", l2, mask));
    CHK(als_count_ok("cmf_als_nnls_step", "sweeps", sweeps));
    return als_step(c, l2, nn_mask, mask, sweeps);
}

extern "C" int cmf_als_cg_step(cmf_ctx *c, double l2, int nn_mask, int mask, int cg_steps, int nn_sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_cg_step", l2, mask));
    CHK(als_count_ok("cmf_als_cg_step", "cg_steps", cg_steps));
    CHK(als_count_ok("cmf_als_cg_step", "nn_sweeps", nn_sweeps, 0));
    CHK(als_logit_check(c, "cmf_als_cg_step", mask, true));
    return als_step(c, l2, nn_mask, mask, nn_sweeps, cg_steps);
}

// test entry: the rows the CG route would write for rows [row0, row0 + nrows) of sweep `which`; the factors are left alone
extern "C" int cmf_als_cg_rows(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, int cg_steps, float *host_f) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "cmf_als_cg_rows: bad factor selector");
    CHK(als_check(c, "cmf_als_cg_rows", l2, 1 << which));
    CHK(als_count_ok("cmf_als_cg_rows", "cg_steps", cg_steps));
    CHK(als_logit_check(c, "cmf_als_cg_rows", 1 << which, true));
    if (row0 < 0 || nrows < 0 || row0 + nrows > c->frows[which]) return fail(CMF_EINVAL, "cmf_als_cg_rows: rows out of range");
    const AlsSweep sw = als_sweep(c, which);
    if (!als_observed(sw)) return fail(CMF_EINVAL, "cmf_als_cg_rows: this sweep has no observed relation: one shared matrix, no per-row systems");
    if (nrows == 0) return CMF_OK;
    if (!host_f) return fail(CMF_EINVAL, "cmf_als_cg_rows: null output");
    DeviceGuard dg(c->device);
    const size_t bytes = (size_t)nrows * c->kp * sizeof(float);
    CHK(ensure_scratch(c, c->als_cg_ws, bytes));
    HIPCHK(hipMemsetAsync(c->als_cg_ws.p, 0, bytes, c->stream));
    CHK(als_cg_rows(c, sw, l2, row0, row0 + nrows, cg_steps, (float *)c->als_cg_ws.p, row0));
    HIPCHK(hipMemcpyAsync(host_f, c->als_cg_ws.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

// test entry: the long rows and the pieces of the last CG sweep (or cmf_als_cg_rows call)
extern "C" int cmf_als_cg_last(cmf_ctx *c, int64_t *out2) {
    if (!c || !out2) return fail(CMF_EINVAL, "cmf_als_cg_last: null context or output");
    out2[0] = c->als_cg_last[0];
    out2[1] = c->als_cg_last[1];
    return CMF_OK;
}

// What the non-negative CG rows cannot sweep: a logistic relation (no reweighting pass) and a relation with biases bound
static int als_nncg_sweep_ok(cmf_ctx *c, const char *what, const AlsSweep &sw) {
    for (int s = 0; s < sw.nrel; ++s) {
        const int w = sw.rel[s].which;
        const char *nm = w == 0 ? "X" : "Y";
        if (als_logit_rel(c, w))
            return fail(CMF_EUNSUPPORTED, "%s: %s has a logistic loss; the non-negative conjugate-gradient rows have no reweighting pass: use cmf_als_nnls_step", what, nm);
        if (c->als_bias[w].on)
            return fail(CMF_EUNSUPPORTED, "%s: %s has biases bound; the non-negative conjugate-gradient rows under biases are not built: use cmf_als_bias_step", what, nm);
    }
    return CMF_OK;
}

extern "C" int cmf_als_nncg_step(cmf_ctx *c, double l2, int nn_mask, int mask, int cg_steps, int nn_cg_steps, int nn_sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_nncg_step", l2, mask));
    CHK(als_count_ok("cmf_als_nncg_step", "cg_steps", cg_steps, 0));
    CHK(als_count_ok("cmf_als_nncg_step", "nn_cg_steps", nn_cg_steps));
    CHK(als_count_ok("cmf_als_nncg_step", "nn_sweeps", nn_sweeps, 0));
    const int bits[3] = {CMF_UPD_U, CMF_UPD_V, CMF_UPD_Z}, nnb[3] = {CMF_NN_U, CMF_NN_V, CMF_NN_Z}, fs[3] = {CMF_U, CMF_V, CMF_Z};
    bool any = false;
    for (int s = 0; s < 3; ++s) {
        if (!(mask & bits[s]) || !(nn_mask & nnb[s]) || c->frows[fs[s]] <= 0) continue;
        const AlsSweep sw = als_sweep(c, fs[s]);
        if (!als_observed(sw)) continue;
        CHK(als_nncg_sweep_ok(c, "cmf_als_nncg_step", sw));
        any = true;
    }
    if (!any) {   // no factor on the new route: the entry point that names the routes left
        if (cg_steps) return cmf_als_cg_step(c, l2, nn_mask, mask, cg_steps, nn_sweeps);
        return nn_sweeps ? cmf_als_nnls_step(c, l2, nn_mask, mask, nn_sweeps) : cmf_als_step(c, l2, nn_mask, mask);
    }
    if (cg_steps) CHK(als_logit_check(c, "cmf_als_nncg_step", mask, true));
    return als_step(c, l2, nn_mask, mask, nn_sweeps, cg_steps, nn_cg_steps);
}

// test entry: the rows the non-negative CG route would write for rows [row0, row0 + nrows) of sweep `which`; the factors are left alone
extern "C" int cmf_als_nncg_rows(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, int nn_cg_steps, float *host_f) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "cmf_als_nncg_rows: bad factor selector");
    CHK(als_check(c, "cmf_als_nncg_rows", l2, 1 << which));
    CHK(als_count_ok("cmf_als_nncg_rows", "nn_cg_steps", nn_cg_steps));
    if (row0 < 0 || nrows < 0 || row0 + nrows > c->frows[which]) return fail(CMF_EINVAL, "cmf_als_nncg_rows: rows out of range");
    const AlsSweep sw = als_sweep(c, which);
    if (!als_observed(sw)) return fail(CMF_EINVAL, "cmf_als_nncg_rows: this sweep has no observed relation: one shared matrix, no per-row systems");
    CHK(als_nncg_sweep_ok(c, "cmf_als_nncg_rows", sw));
    if (nrows == 0) return CMF_OK;
    if (!host_f) return fail(CMF_EINVAL, "cmf_als_nncg_rows: null output");
    DeviceGuard dg(c->device);
    const size_t bytes = (size_t)nrows * c->kp * sizeof(float);
    CHK(ensure_scratch(c, c->als_cg_ws, bytes));
    HIPCHK(hipMemsetAsync(c->als_cg_ws.p, 0, bytes, c->stream));
    CHK(als_cg_rows(c, sw, l2, row0, row0 + nrows, nn_cg_steps, (float *)c->als_cg_ws.p, row0, true));
    HIPCHK(hipMemcpyAsync(host_f, c->als_cg_ws.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

// test entries: the long rows and the pieces of the last non-negative CG sweep (or cmf_als_nncg_rows call); the passes its rows ran
// and the stored entries those passes read
extern "C" int cmf_als_nncg_last(cmf_ctx *c, int64_t *out2) {
    if (!c || !out2) return fail(CMF_EINVAL, "cmf_als_nncg_last: null context or output");
    out2[0] = c->als_nncg_last[0];
    out2[1] = c->als_nncg_last[1];
    return CMF_OK;
}
extern "C" int cmf_als_nncg_passes(cmf_ctx *c, int64_t *out2) {
    if (!c || !out2) return fail(CMF_EINVAL, "cmf_als_nncg_passes: null context or output");
    DeviceGuard dg(c->device);
    CHK(als_nncg_count(c));
    out2[0] = c->als_nncg_last[2];
    out2[1] = c->als_nncg_last[3];
    return CMF_OK;
}

// test entry: the kernel on the caller's systems (cmf_als_normal's layout), f in / out
extern "C" int cmf_als_nnls_rows(cmf_ctx *c, int64_t nrows, const float *host_H, const float *host_g, float *host_f, int sweeps) {
    NEED_PROBLEM(c);
    if (!host_H || !host_g || !host_f || nrows < 0) return fail(CMF_EINVAL, "cmf_als_nnls_rows: null pointer or negative row count");
    CHK(als_count_ok("cmf_als_nnls_rows", "sweeps", sweeps));
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_als_nnls_rows: n_components <= 256 only (k_pad = %d)", c->kp);
    if (nrows == 0) return CMF_OK;
    DeviceGuard dg(c->device);
    const int64_t kp = c->kp, nh = nrows * kp * kp, nv = nrows * kp;
    CHK(ensure_scratch(c, c->als_nnls_ws, (size_t)(nh + 2 * nv) * sizeof(float)));
    float *H = (float *)c->als_nnls_ws.p, *g = H + nh, *f = g + nv;
    HIPCHK(hipMemcpyAsync(H, host_H, (size_t)nh * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g, host_g, (size_t)nv * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(f, host_f, (size_t)nv * sizeof(float), hipMemcpyHostToDevice, c->stream));
    CHK(als_nnls_launch(c, H, g, f, nullptr, nrows, sweeps));
    HIPCHK(hipMemcpyAsync(host_f, f, (size_t)nv * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_als_normal(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, float *host_H, float *host_g) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "cmf_als_normal: bad factor selector");
    CHK(als_check(c, "cmf_als_normal", l2, 1 << which));
    if (row0 < 0 || nrows < 0 || row0 + nrows > c->frows[which]) return fail(CMF_EINVAL, "cmf_als_normal: rows out of range");
    const AlsSweep sw = als_sweep(c, which);
    if (!als_observed(sw)) return fail(CMF_EINVAL, "cmf_als_normal: this sweep has no observed relation: one shared matrix, no per-row systems");
    if (nrows == 0) return CMF_OK;
    DeviceGuard dg(c->device);
    return als_rows_to_host(c, sw, l2, row0, row0 + nrows, host_H, host_g);
}

extern "C" int cmf_als_layout(cmf_ctx *c, int64_t *out4) {
    NEED_PROBLEM(c);
    if (!out4) return fail(CMF_EINVAL, "cmf_als_layout: null output");
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_als_layout: n_components <= 256 only (k_pad = %d)", c->kp);
    DeviceGuard dg(c->device);
    out4[0] = als_piece_len(c);
    const int fs[3] = {CMF_U, CMF_V, CMF_Z};
    for (int s = 0; s < 3; ++s) {
        const AlsSweep sw = als_sweep(c, fs[s]);
        AlsPlan pl;
        if (als_observed(sw)) CHK(als_plan(c, sw, 0, c->frows[fs[s]], pl));
        out4[1 + s] = (int64_t)pl.pieces.size();
    }
    return CMF_OK;
}

#endif // CMF_ALS_HOST
