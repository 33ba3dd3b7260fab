// cmf_als.hip.h -- ALS (alternating least squares) on the quadratic objective over an observed pattern
//   1/2 sum_{Ox} wx_ij (x_ij - u_i . v_j)^2 + 1/2 sum_{Oy} wy_jc (y_jc - v_j . z_c)^2 + l2 / 2 (|U|^2 + |V|^2 + |Z|^2),   l2 > 0.
// Every row f_i of the factor being swept has its own k x k system
//   (sum_{c in O_i} w_ic b_c b_c^T + S + l2 I) f_i = sum_{c in O_i} w_ic t_ic b_c + N_i
// where an OBSERVED relation (weights bound as CSR, cmf_set_weighted_csr) contributes the sums over its stored entries and a FULL
// relation (no weights: every cell counts with weight 1) the shared Gram S = B^T B and the row N_i of T B.  Under a background
// weight c0 (cmf_als_bg.hip.h, implicit feedback) an observed relation counts the cells outside its pattern too: the kernels read
// the excess weights w - c0 where they read w, and S = sum_sides coef Gram(B_side) (als_shared_terms).  What depended on "a full
// side exists" depends on "S is set".
//
// The host side (cmf_als_steps.hip.h).  Every step entry point checks its own arguments under its own name, fills an AlsStepOpts
// { nn_sweeps, cg_steps, nn_cg_steps, dual_max, biases } (0 / false where it has no such argument) and calls als_step, the one
// place that sweeps: V, U, Z, each by the route als_route gives it from the facts of the sweep (observed; S is set; a logistic
// relation; k_pad; the factor is non-negative) and those options -- the first row of this table that applies:
//   route         taken when                                           what it does
//   rows NNCG     observed; non-negative, nn_cg_steps > 0              no systems: als_nncg_kernel (cmf_als_nncg.hip.h) runs matrix-free
//                                                                      projected CG steps per row from the current rows clamped at
//                                                                      zero, in place; the classes and the pieces of rows CG
//   rows NNLS     observed; non-negative, nn_sweeps > 0                the finished systems to als_nnls_kernel (cmf_als_nnls.hip.h):
//                                                                      cyclic coordinate descent from the current rows, in place
//   shared HALS   no observed relation; non-negative, nn_sweeps > 0    hals_sweep (cmf_hals.hip.h) nn_sweeps times on the one Gram
//   shared exact  no observed relation (otherwise)                     ONE matrix G + l2 I for all rows, inverted once in float64
//                                                                      (shared_inverse64), one product, projected if non-negative
//   rows CG       observed; signed, cg_steps > 0                       no systems: als_cg_kernel (cmf_als_cg.hip.h) runs matrix-free
//                                                                      CG steps per row from the current rows, in place; the host
//                                                                      sorts the rows into LDS capacity classes by length; a row
//                                                                      longer than "als_cg_piece" entries is cut into pieces
//                                                                      (als_cg_piece_kernel / als_cg_combine_kernel)
//   rows dual     observed (otherwise); dual_max > 0, S not set, no    the rows of 1 .. dual_max stored entries whose class width
//                 logistic relation, k_pad > 32                        NP(n) < k_pad: K = A A^T + l2 I_n (als_dual_gram_kernel,
//                                                                      cmf_als_dual.hip.h), K z = y through the exact solve, f = A^T z:
//                                                                      the same exact row from an n x n system; rows without an entry:
//                                                                      zeros; other rows: rows exact, as a plan of listed rows.  No
//                                                                      row of the plan dual: nothing is launched, rows exact runs
//   rows exact    observed (otherwise)                                 the finished systems through the exact solve (als_solve_rows:
//                                                                      safe_solve_rows, cmf_newton.hip.h, Hessians declared positive
//                                                                      semi-definite, threshold l2 / 16; lambda_min(H_i) >= l2: the
//                                                                      spectral clamp never acts), no float64 refinement; projected
//                                                                      if non-negative
// Under `biases` als_step refreshes the adjusted targets before the sweeps and sweeps the bias blocks after them (cmf_als_bias.hip.h).
// A PER-ROW l2 (cmf_set_l2_rows; cmf_als_steps.hip.h): with multipliers m_F bound for the swept factor, row i of every row route reads
// lambda_i = l2 * m_F[i] where it reads l2 below -- one float32 product (als_row_l2, cmf_als_cg.hip.h) in the LR = true instance of
// als_finish_kernel, als_cg_kernel / als_cg_combine_kernel, als_nncg_kernel / als_nncg_combine_kernel and als_dual_gram_kernel; the
// exact solve takes its threshold from l2 min(m_F); the shared routes take equal multipliers only.  Nothing bound: the LR = false
// instances, which are the kernels without any of this.
//
// The finished systems.  ONE chunk loop (als_chunks) is the only caller of als_normal_kernel / als_finish_kernel.  It takes a plan
// (AlsPlan: the pieces, first[], where the finished g of a slot goes, the shared terms or null) -- of a range of rows for rows
// exact, rows NNLS and cmf_als_normal, of the listed formed rows for rows dual -- cuts it into chunks of at most `cap` slots and
// pieces, and hands every finished chunk to its caller's `use`.
// als_normal_kernel<KP, LG>: one 512-thread workgroup per PIECE of a row (at most `als_piece` stored
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
#include "cmf_als_dual.hip.h"

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
// LR: l2m are the multipliers of cmf_set_l2_rows; slot `row` is row lrows[row] of them (a plan of listed rows) or, lrows null, row
// `row` (a plan of a range: the host passes the pointer at its first row).  LR = false: neither is read.
template <bool LR>
__global__ __launch_bounds__(256) void als_finish_kernel(const float *Hp, const float *gp, const int64_t *first, int64_t pbase, const float *S,
                                                         const float *N, float l2, int k, int kp, float *H, float *g, const float *l2m, const int64_t *lrows) {
    __shared__ float tl[32][33];
    const int64_t row = blockIdx.x;
    if constexpr (LR) l2 = als_row_l2<true>(l2, l2m, lrows ? lrows[row] : row);   // uniform over the workgroup
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

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx): what the
// bias, background and loss headers need too -- the sweep descriptor, the launch ladders, the piece plan.  The sweeps themselves:
// cmf_als_steps.hip.h, behind those headers.
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

static int64_t als_piece_len(const cmf_ctx *c) { return c->opt_als_piece > 0 ? rup(c->opt_als_piece, 32) : (int64_t)ALS_PIECE_DEFAULT; }

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

// ... for a kernel with one more template argument behind GL (TARG)
#define ALS_LAUNCH_GL_T(c, KERNEL, TARG, ...)                                                                            \
    switch ((c)->kp) {                                                                                                   \
    case 32: hipLaunchKernelGGL((cmfk::KERNEL<8, TARG>), __VA_ARGS__); break;                                            \
    case 64: hipLaunchKernelGGL((cmfk::KERNEL<16, TARG>), __VA_ARGS__); break;                                           \
    case 128: hipLaunchKernelGGL((cmfk::KERNEL<32, TARG>), __VA_ARGS__); break;                                          \
    default: hipLaunchKernelGGL((cmfk::KERNEL<64, TARG>), __VA_ARGS__); break;                                           \
    }

// Rows of `nip` CSR images (ip[s]: the rows' indptr) cut into pieces of at most L stored entries: row by row, within a row image by
// image, piece(r, s, beg, len) per piece in that order.  The rows are 0 .. nrows, or the listed ones (`rows`, ascending or not).
// Returns first[i], the pieces before the i-th of those rows ([rows + 1]).
template <class Piece>
static std::vector<int64_t> als_cut_rows(const std::vector<int64_t> *ip, int nip, int64_t nrows, int64_t L, Piece piece, const std::vector<int64_t> *rows = nullptr) {
    const int64_t cnt = rows ? (int64_t)rows->size() : nrows;
    std::vector<int64_t> first((size_t)cnt + 1, 0);
    int64_t n = 0;
    for (int64_t i = 0; i < cnt; ++i) {
        const int64_t r = rows ? (*rows)[(size_t)i] : i;
        first[(size_t)i] = n;
        for (int s = 0; s < nip; ++s) {
            const int64_t e = ip[s][(size_t)r + 1];
            for (int64_t q = ip[s][(size_t)r]; q < e; q += L, ++n) piece(r, s, q, (int32_t)std::min(L, e - q));
        }
    }
    first[(size_t)cnt] = n;
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

// the stored entries of rows 0 .. nrows over the observed sides (ip: als_fetch_indptr)
static std::vector<int64_t> als_row_lens(const std::vector<int64_t> *ip, int nobs, int64_t nrows) {
    std::vector<int64_t> len((size_t)nrows, 0);
    for (int s = 0; s < nobs; ++s)
        for (int64_t r = 0; r < nrows; ++r) len[(size_t)r] += ip[s][(size_t)r + 1] - ip[s][(size_t)r];
    return len;
}

// The rows whose systems the chunk loop (als_chunks, cmf_als_steps.hip.h) forms.  Slot i is one row of the swept factor; its pieces
// are pieces[first[i] .. first[i + 1]), in the order of als_cut_rows.
struct AlsPlan {
    std::vector<cmfk::AlsPiece> pieces;       // AlsPiece::row: the row of the swept factor
    std::vector<int64_t> first;               // [slots + 1]
    int64_t row0 = 0;                         // a range: slot i is row row0 + i, and its finished g is that row of c->als_g
    std::vector<int64_t> rows;                // a list (the dual route's): row lists that go to the device with the plan; the slots are
    bool listed = false;                      // ... listed rows, and the finished g of a chunk's slots starts at row 0 of c->als_g
    const float *S = nullptr, *N = nullptr;   // the shared terms of the sweep (als_shared_terms), or null
    const cmfk::AlsPiece *dpieces = nullptr;  // als_plan_upload: pieces, first and rows on the device (c->als_desc)
    const int64_t *dfirst = nullptr, *drows = nullptr;
};
// the plan of rows [r0, r1)
static int als_plan(cmf_ctx *c, const AlsSweep &sw, int64_t r0, int64_t r1, AlsPlan &pl) {
    std::vector<int64_t> ip[2];
    CHK(als_fetch_indptr(c, sw, r0, r1, ip));
    pl.row0 = r0;
    pl.pieces.clear();
    pl.first = als_cut_rows(ip, sw.nobs, r1 - r0, als_piece_len(c), [&](int64_t r, int s, int64_t beg, int32_t len) {
        pl.pieces.push_back(cmfk::AlsPiece{beg, len, s, r0 + r});
    });
    return CMF_OK;
}
static int als_plan_upload(cmf_ctx *c, AlsPlan &pl) {
    const size_t pbytes = std::max<size_t>(16, pl.pieces.size() * sizeof(cmfk::AlsPiece)), fbytes = pl.first.size() * sizeof(int64_t);
    const size_t rbytes = pl.rows.size() * sizeof(int64_t);
    CHK(ensure_scratch(c, c->als_desc, pbytes + fbytes + rbytes));
    char *d = (char *)c->als_desc.p;
    if (!pl.pieces.empty()) HIPCHK(hipMemcpyAsync(d, pl.pieces.data(), pl.pieces.size() * sizeof(cmfk::AlsPiece), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d + pbytes, pl.first.data(), fbytes, hipMemcpyHostToDevice, c->stream));
    if (rbytes) HIPCHK(hipMemcpyAsync(d + pbytes + fbytes, pl.rows.data(), rbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vectors may go
    pl.dpieces = (const cmfk::AlsPiece *)d;
    pl.dfirst = (const int64_t *)(d + pbytes);
    pl.drows = (const int64_t *)(d + pbytes + fbytes);
    return CMF_OK;
}

#endif // CMF_ALS_HOST
