// cmf_als.hip.h -- ALS (alternating least squares) on the quadratic objective over an observed pattern
//   1/2 sum_{Ox} wx_ij (x_ij - u_i . v_j)^2 + 1/2 sum_{Oy} wy_jc (y_jc - v_j . z_c)^2 + l2 / 2 (|U|^2 + |V|^2 + |Z|^2),   l2 > 0.
// Every row f_i of the factor being swept is the exact minimiser of its own k x k system
//   (sum_{c in O_i} w_ic b_c b_c^T + S + l2 I) f_i = sum_{c in O_i} w_ic t_ic b_c + N_i
// where an OBSERVED relation (weights bound as CSR, cmf_set_weighted_csr) contributes the sums over its stored entries and a FULL
// relation (no weights: every cell counts with weight 1) the shared Gram S = B^T B and the row N_i of T B.
//
// als_normal_kernel<KP>: one 512-thread workgroup per PIECE of a row (at most `als_piece` stored entries, a multiple of 32) of a CSR
// image (indptr, idx, pv = w t, wv = w).  The gathered rows b_e are staged 32 at a time through registers into a double-buffered
// LDS tile, scaled by sqrt(w_e); while they are in registers the owning lanes add p_e b_e to the gradient part g.  H is a rank-32
// update per step on v_mfma_f32_32x32x2_f32, both operands read from the ONE staged image:
//     H = sum_e (sqrt(w_e) b_e)(sqrt(w_e) b_e)^T,     g = sum_e p_e b_e.
// The geometry is that of row_hess_kernel in its single-image symmetric form (cmf_rowhess.hip.h, SYM = 3), restated here, not
// shared: 16 lanes per gathered row, row-major 32 x KP tiles, and at k_pad = 256 only the 36 blocks (32 x 32) on or above the block
// diagonal, spread 4 + 5 + 5 over the wave types
//     waves 0-3:            (w, 4) (w, 5) (w, 6) (w, 7)                                   5 fragments per k-pair
//     waves 4, 6 (base b):  (b, b) (b, b+1) (b, b+2) (b, b+3) (b+3, b+3)                  4 fragments
//     waves 5, 7 (base b):  (b+1, b+1) (b+1, b+2) (b+1, b+3) (b+2, b+2) (b+2, b+3)        3 fragments
// Below k_pad = 256 every block is formed (wave (wm, wn) owns block row wm, TN block columns).  Unlike row_hess_kernel there is no
// dot product with the current row and no targets image: the system does not depend on f_i.
// A piece writes its partial H (the blocks it formed) and g to its own scratch slot; als_finish_kernel adds the pieces of a row in
// piece order, mirrors the upper triangle (so H_i is symmetric to the bit), adds S, l2 on the first k diagonal entries and 1 on the
// padding diagonal, and N_i to g.  No atomics anywhere: a repeated call from the same state is bit-identical.  Padding columns of
// the factors are zero, so the padding of H_i and g_i is exact zeros (unit diagonal apart).
// The solves go through safe_solve_rows (cmf_newton.hip.h) with the Hessians declared positive semi-definite, the threshold l2 / 16
// (lambda_min(H_i) >= l2: the spectral clamp never acts) and the float64 refinement off.
// A sweep without an observed side has ONE matrix G + l2 I for all rows: inverted once in float64 (shared_inverse64) and applied
// with one product.
// Non-negative rows (cmf_als_nnls_step): the finished systems of a chunk go to als_nnls_kernel (cmf_als_nnls.hip.h) instead of the
// Cholesky solves -- cyclic coordinate descent from the current rows, `sweeps` passes; a sweep whose relations are all full runs
// hals_sweep (cmf_hals.hip.h) that many times on the one Gram.
// Signed rows by conjugate gradients (cmf_als_cg_step): a signed swept factor with an observed relation skips the normal equations
// and the Cholesky solves altogether -- als_cg_kernel (cmf_als_cg.hip.h) runs `cg_steps` matrix-free CG steps per row from the
// current rows, in place.  The host sorts the rows into a few LDS capacity classes by their length (als_cg_rows).
// Background weights (cmf_als_bg.hip.h, implicit feedback): an observed relation may count the cells outside its pattern with a
// weight c0 -- the kernels above then read the excess weights w - c0 where they read w, and S becomes sum_sides coef Gram(B_side)
// (als_shared_terms); everything that depended on "a full side exists" depends on "S is set".
#pragma once
#include "cmf_kernels.hip.h"
#include "cmf_als_nnls.hip.h"
#include "cmf_als_cg.hip.h"
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
};
struct AlsArgs {
    AlsSide s0, s1;
    const AlsPiece *pieces; // one per workgroup
    float *Hp;              // [piece][KP][KP] partial Hessians (blocks on or above the block diagonal at KP = 256, all blocks below)
    float *gp;              // [piece][KP]
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

template <int KP>
__global__ __launch_bounds__(512) void als_normal_kernel(AlsArgs g) {
    using C = AlsCfg<KP>;
    __shared__ __attribute__((aligned(16))) float sm[2 * C::TILE];
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, lh = lane >> 5;
    const int uw = __builtin_amdgcn_readfirstlane(t >> 6);
    const AlsPiece pc = g.pieces[blockIdx.x];
    const bool second = pc.side != 0;
    const int32_t *idx = (second ? g.s1.idx : g.s0.idx) + pc.beg;
    const float *pv = (second ? g.s1.pv : g.s0.pv) + pc.beg;
    const float *wv = (second ? g.s1.wv : g.s0.wv) + pc.beg;
    const float *B = second ? g.s1.B : g.s0.B;
    const int ns = pc.len, nt = (ns + 31) >> 5;
    const int trow = t / C::LPR, tl16 = t % C::LPR;
    const bool loader = t < 32 * C::LPR;    // k_pad = 32: half of the threads cover the tile

    f32x4 rr[C::CPT], gacc[C::CPT];
    float sq = 0.f, pe = 0.f;
#pragma unroll
    for (int q = 0; q < C::CPT; ++q) rr[q] = gacc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
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
            sq = sqrtf(wv[q]);
            pe = pv[q];
        } else {
#pragma unroll
            for (int c = 0; c < C::CPT; ++c) rr[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            sq = 0.f;
            pe = 0.f;
        }
    };
    auto stage = [&](int nb) { // registers -> gradient part and the sqrt(w)-scaled LDS image
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
#define CMF_ALS_BG_HOST
#include "cmf_als_bg.hip.h"   // background weights: als_shared_terms, als_side_weights and the entry points of its own
static int64_t als_piece_len(const cmf_ctx *c) { return c->opt_als_piece > 0 ? rup(c->opt_als_piece, 32) : (int64_t)ALS_PIECE_DEFAULT; }

static int als_relation_ok(cmf_ctx *c, const char *what, int which) {
    if (c->wm_kind[which] == WM_DENSE)
        return fail(CMF_EUNSUPPORTED, "%s: %s has DENSE weights bound; ALS takes weights as the CSR pattern of the observed entries (cmf_set_weighted_csr)",
                    what, which == 0 ? "X" : "Y");
    if (c->wm_kind[which] != WM_CSR && !have_data(c, which))
        return fail(CMF_EINVAL, "%s: %s has neither data nor CSR weights", what, which == 0 ? "X" : "Y");
    return CMF_OK;
}

struct AlsPlan { // the pieces of rows [r0, r1) of one sweep, host side
    std::vector<cmfk::AlsPiece> pieces;
    std::vector<int64_t> first;   // [r1 - r0 + 1]
    int64_t nnz = 0;
};
// indptr of an observed side back to the host (the pattern lives on the device only)
static int als_fetch_indptr(cmf_ctx *c, const WCsrDev &M, int64_t r0, int64_t r1, std::vector<int64_t> &ip) {
    ip.assign((size_t)(r1 - r0 + 1), 0);
    HIPCHK(hipMemcpyAsync(ip.data(), M.indptr + r0, ip.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}
static int als_plan(cmf_ctx *c, const AlsRel *obs, int nobs, int64_t r0, int64_t r1, AlsPlan &pl) {
    const int64_t L = als_piece_len(c);
    std::vector<int64_t> ip[2];
    for (int s = 0; s < nobs; ++s) CHK(als_fetch_indptr(c, c->wm_sp[obs[s].which][obs[s].t], r0, r1, ip[s]));
    pl.pieces.clear();
    pl.first.assign((size_t)(r1 - r0 + 1), 0);
    pl.nnz = 0;
    for (int64_t r = 0; r < r1 - r0; ++r) {
        pl.first[(size_t)r] = (int64_t)pl.pieces.size();
        for (int s = 0; s < nobs; ++s) {
            const int64_t b = ip[s][(size_t)r], e = ip[s][(size_t)r + 1];
            pl.nnz += e - b;
            for (int64_t q = b; q < e; q += L) pl.pieces.push_back(cmfk::AlsPiece{q, (int32_t)std::min(L, e - q), s});
        }
    }
    pl.first[(size_t)(r1 - r0)] = (int64_t)pl.pieces.size();
    return CMF_OK;
}

static int als_launch_normal(cmf_ctx *c, const cmfk::AlsArgs &a, int64_t npieces, int64_t nnz) {
    if (npieces <= 0) return CMF_OK;
    Timed tm(c, CMF_K_ROWHESS, 2.0 * (double)nnz * c->k * c->k);
    const dim3 grid((unsigned)npieces), block(512);
    switch (c->kp) {
    case 32: hipLaunchKernelGGL((cmfk::als_normal_kernel<32>), grid, block, 0, c->stream, a); break;
    case 64: hipLaunchKernelGGL((cmfk::als_normal_kernel<64>), grid, block, 0, c->stream, a); break;
    case 128: hipLaunchKernelGGL((cmfk::als_normal_kernel<128>), grid, block, 0, c->stream, a); break;
    case 256: hipLaunchKernelGGL((cmfk::als_normal_kernel<256>), grid, block, 0, c->stream, a); break;
    default: return fail(CMF_EUNSUPPORTED, "ALS normal equations are built for n_components <= 256 (k_pad = %d)", c->kp);
    }
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

static int als_nnls_launch(cmf_ctx *c, const float *H, const float *g, float *F, const int64_t *first, int64_t nrows, int sweeps) {
    if (nrows <= 0) return CMF_OK;
    cmfk::NnlsArgs a;
    a.H = H; a.g = g; a.F = F; a.first = first; a.nrows = nrows; a.k = c->k; a.sweeps = sweeps;
    Timed tm(c, CMF_K_HALS, 2.0 * (double)nrows * c->k * c->k * sweeps);
    const dim3 grid((unsigned)((nrows + cmfk::NNLS_WAVES - 1) / cmfk::NNLS_WAVES)), block(64 * cmfk::NNLS_WAVES);
    switch (c->kp) {
    case 32: hipLaunchKernelGGL((cmfk::als_nnls_kernel<32>), grid, block, 0, c->stream, a); break;
    case 64: hipLaunchKernelGGL((cmfk::als_nnls_kernel<64>), grid, block, 0, c->stream, a); break;
    case 128: hipLaunchKernelGGL((cmfk::als_nnls_kernel<128>), grid, block, 0, c->stream, a); break;
    case 256: hipLaunchKernelGGL((cmfk::als_nnls_kernel<256>), grid, block, 0, c->stream, a); break;
    default: return fail(CMF_EUNSUPPORTED, "the non-negative row solve is built for n_components <= 256 (k_pad = %d)", c->kp);
    }
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// Rows [r_begin, r_end) of the sweep of factor f in per-row form: normal equations chunk by chunk, then (solve) the Cholesky
// solves into c->als_sol -- or, nnls_sweeps > 0, that many coordinate-descent sweeps of the chunk's rows of F, in place -- or
// (host_H / host_g, one chunk) the finished systems back to the host.
static int als_rows(cmf_ctx *c, int f, double l2, int64_t r_begin, int64_t r_end, bool solve, float *host_H, float *host_g, int nnls_sweeps = 0) {
    using namespace cmfk;
    AlsRel rel[2], obs[2];
    const int nrel = als_rels(f, rel);
    int nobs = 0;
    for (int s = 0; s < nrel; ++s)
        if (c->wm_kind[rel[s].which] == WM_CSR) obs[nobs++] = rel[s];
    const int kp = c->kp;
    const int64_t kk = (int64_t)kp * kp, rows_pad = c->frows_pad[f];
    // the full relation: its Gram into every row's matrix, its product into the right-hand sides; a background: c0 times the Gram
    const float *S = nullptr, *N = nullptr;
    CHK(als_shared_terms(c, rel, nrel, &S, &N));
    AlsPlan pl;
    CHK(als_plan(c, obs, nobs, r_begin, r_end, pl));
    const int64_t nrows = r_end - r_begin;
    // chunks: at most hessian_chunk_rows rows and (but for a single row) as many pieces
    const int64_t cap = solve ? hessian_chunk_rows(c, rows_pad) : std::max<int64_t>(1, nrows);
    int64_t max_rows = 0, max_pieces = 0;
    std::vector<int64_t> cuts{0};
    for (int64_t r = 0; r < nrows;) {
        int64_t e = r;
        while (e < nrows && e - r < cap && (e == r || !solve || pl.first[(size_t)e + 1] - pl.first[(size_t)r] <= cap)) ++e;
        max_rows = std::max(max_rows, e - r);
        max_pieces = std::max(max_pieces, pl.first[(size_t)e] - pl.first[(size_t)r]);
        cuts.push_back(e);
        r = e;
    }
    CHK(kl_ensure(c, c->als_h, (size_t)std::max<int64_t>(1, max_rows) * kk * sizeof(float)));
    CHK(kl_ensure(c, c->als_part, (size_t)std::max<int64_t>(1, max_pieces) * (kk + kp) * sizeof(float)));
    CHK(kl_ensure(c, c->als_g, (size_t)rows_pad * kp * sizeof(float)));
    if (!nnls_sweeps) CHK(kl_ensure(c, c->als_sol, (size_t)rows_pad * kp * sizeof(float)));
    const size_t pbytes = std::max<size_t>(16, pl.pieces.size() * sizeof(AlsPiece)), fbytes = pl.first.size() * sizeof(int64_t);
    CHK(kl_ensure(c, c->als_desc, pbytes + fbytes));
    AlsPiece *dpieces = (AlsPiece *)c->als_desc.p;
    int64_t *dfirst = (int64_t *)((char *)c->als_desc.p + pbytes);
    if (!pl.pieces.empty()) HIPCHK(hipMemcpyAsync(dpieces, pl.pieces.data(), pl.pieces.size() * sizeof(AlsPiece), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dfirst, pl.first.data(), fbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vectors may go

    AlsArgs a;
    memset(&a, 0, sizeof a);
    for (int s = 0; s < nobs; ++s) {
        const WCsrDev &M = c->wm_sp[obs[s].which][obs[s].t];
        AlsSide sd{M.idx, M.pv, als_side_weights(M), c->F[obs[s].fb]};
        if (s == 0) a.s0 = sd; else a.s1 = sd;
    }
    float *Hc = (float *)c->als_h.p, *Hp = (float *)c->als_part.p;
    float *grad = (float *)c->als_g.p, *sol = (float *)c->als_sol.p;   // (sol: null and unused under nnls_sweeps)
    a.Hp = Hp;
    // the threshold of the plain Cholesky route, well below l2 <= lambda_min(H_i): its test (a Cholesky of H_i - pert I whose pivots
    // must exceed 4e-6 max H_jj) passes unless cond(H_i) is above ~2e5, where a float32 factorisation has nothing left to give
    const double pert = l2 / 16.0;
    for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
        const int64_t c0 = cuts[ci], c1 = cuts[ci + 1], nr = c1 - c0, row0 = r_begin + c0;
        const int64_t pbase = pl.first[(size_t)c0], np = pl.first[(size_t)c1] - pbase;
        a.pieces = dpieces + pbase;
        a.gp = Hp + std::max<int64_t>(1, max_pieces) * kk;
        int64_t nnz = 0;
        for (int64_t p = pbase; p < pbase + np; ++p) nnz += pl.pieces[(size_t)p].len;
        CHK(als_launch_normal(c, a, np, nnz));
        {
            Timed tm(c, CMF_K_ELEMWISE);
            hipLaunchKernelGGL(als_finish_kernel, dim3((unsigned)nr), dim3(256), 0, c->stream, (const float *)Hp, (const float *)a.gp, (const int64_t *)(dfirst + c0),
                               pbase, S, N ? N + row0 * kp : nullptr, (float)l2, c->k, kp, Hc, grad + row0 * kp);
            HIPCHK(hipGetLastError());
        }
        if (solve && nnls_sweeps) {
            // the gathered factors are the other ones: the chunks to come do not read the rows written here
            CHK(als_nnls_launch(c, Hc, grad + row0 * kp, c->F[f] + row0 * kp, S ? nullptr : dfirst + c0, nr, nnls_sweeps));
        } else if (solve) {
            // the plain Cholesky route of the per-row Newton sweeps; what it reads of the Newton step's state is put back
            const bool save_psd = c->hess_psd;
            const int64_t save_r1 = c->rank1_rows, save_eig = c->eig_clamp_rows;
            std::vector<int> save_bad;
            save_bad.swap(c->bad_host);
            c->hess_psd = true;
            const int rc = safe_solve_rows(c, Hc, grad + row0 * kp, sol + row0 * kp, nr, c->k, kp, pert);
            c->hess_psd = save_psd;
            c->rank1_rows = save_r1; c->eig_clamp_rows = save_eig;
            c->bad_host.swap(save_bad);
            CHK(rc);
        } else {
            if (host_H) HIPCHK(hipMemcpyAsync(host_H, Hc, (size_t)nr * kk * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            if (host_g) HIPCHK(hipMemcpyAsync(host_g, grad + row0 * kp, (size_t)nr * kp * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    return CMF_OK;
}

static int als_apply(cmf_ctx *c, int f, const float *sol, bool nn) {
    return launch_ew(c, cmfk::als_apply_kernel, c->frows[f] * c->kp, c->F[f], sol, c->frows[f], c->k, c->kp, nn ? 1 : 0);
}

static bool als_observed(const cmf_ctx *c, int f) {
    AlsRel rel[2];
    const int n = als_rels(f, rel);
    for (int s = 0; s < n; ++s)
        if (c->wm_kind[rel[s].which] == WM_CSR) return true;
    return false;
}

// a sweep whose relations are all full: F <- clamp(N (G + l2 I)^-1), the inverse formed once in float64
static int als_sweep_shared(cmf_ctx *c, int f, double l2, bool nn) {
    AlsRel rel[2];
    const int nrel = als_rels(f, rel);
    CHK(ensure_shared64(c));
    for (int s = 0; s < nrel; ++s) {
        CHK(gram64(c, c->F[rel[s].fb], c->frows_pad[rel[s].fb], (double *)(s == 0 ? c->g64a.p : c->g64b.p), nullptr));
        CHK(data_times(c, rel[s].which, rel[s].data_trans, c->F[rel[s].fb], c->num, s > 0));
    }
    CHK(launch_hess64(c, (const double *)c->g64a.p, 1.0, nrel > 1 ? (const double *)c->g64b.p : nullptr, 1.0, l2));
    const int rc = shared_inverse64(c, (const double *)c->h64.p, c->k, 0.5 * l2, true);
    if (rc == CMF_EUNSUPPORTED) return fail(CMF_EHIP, "cmf_als_step: the float64 inverse of G + l2 I failed (non-finite factors?)");
    CHK(rc);
    CHK(gemm(c, MODE_NN, c->num, c->kp, c->Hinv, c->kp, c->den, c->frows_pad[f], c->kp, c->kp));
    return als_apply(c, f, c->den, nn);
}

static int als_check(cmf_ctx *c, const char *what, double l2, int mask) {
    if (!(l2 > 0.0) || !std::isfinite(l2)) return fail(CMF_EINVAL, "%s: l2 must be positive (a row with fewer than k observations is singular otherwise), got %g", what, l2);
    if (mask <= 0 || mask > 7) return fail(CMF_EINVAL, "%s: update_mask must name at least one of U, V, Z (got %d)", what, mask);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: n_components <= 256 only (k_pad = %d)", what, c->kp);
    if (mask & (CMF_UPD_U | CMF_UPD_V)) CHK(als_relation_ok(c, what, 0));
    if (mask & (CMF_UPD_Z | CMF_UPD_V)) CHK(als_relation_ok(c, what, 1));
    return CMF_OK;
}

// a non-negative sweep whose relations are all full: N and G as cmf_hals_step forms them, `sweeps` passes of hals_sweep
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
#define ALS_CG_CASE(KP)                                                                                   \
    case KP:                                                                                              \
        CHK(allow_big_lds(c, (const void *)cmfk::als_cg_kernel<KP>, ALS_CG_LDS_TOTAL));                   \
        hipLaunchKernelGGL((cmfk::als_cg_kernel<KP>), grid, block, lds, c->stream, a);                    \
        break;
    switch (c->kp) {
    ALS_CG_CASE(32)
    ALS_CG_CASE(64)
    ALS_CG_CASE(128)
    ALS_CG_CASE(256)
    default: return fail(CMF_EUNSUPPORTED, "the conjugate-gradient row solve is built for n_components <= 256 (k_pad = %d)", c->kp);
    }
#undef ALS_CG_CASE
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// Rows [r_begin, r_end) of the sweep of factor f (which has an observed relation) by `steps` CG steps from the rows of c->F[f];
// row r goes to Fout + (r - out_row0) * k_pad (in place: Fout = c->F[f], out_row0 = 0 -- the gathered factors are the other ones).
// The rows are sorted into capacity classes by their stored entries: capacity / 8, / 4, / 2 and the whole capacity keep the
// gathered rows in LDS (shorter rows: more workgroups per CU), longer rows stream; one launch per class.
static int als_cg_rows(cmf_ctx *c, int f, double l2, int64_t r_begin, int64_t r_end, int steps, float *Fout, int64_t out_row0) {
    using namespace cmfk;
    AlsRel rel[2], obs[2];
    const int nrel = als_rels(f, rel);
    int nobs = 0;
    for (int s = 0; s < nrel; ++s)
        if (c->wm_kind[rel[s].which] == WM_CSR) obs[nobs++] = rel[s];
    const int kp = c->kp;
    const int64_t nrows = r_end - r_begin;
    AlsCgArgs a;
    memset(&a, 0, sizeof a);
    CHK(als_shared_terms(c, rel, nrel, &a.S, &a.N)); // as als_rows
    std::vector<int64_t> ip[2];
    for (int s = 0; s < nobs; ++s) {
        const WCsrDev &M = c->wm_sp[obs[s].which][obs[s].t];
        CHK(als_fetch_indptr(c, M, r_begin, r_end, ip[s]));
        AlsCgSide sd{M.indptr, M.idx, M.pv, als_side_weights(M), c->F[obs[s].fb]};
        if (s == 0) a.s0 = sd; else a.s1 = sd;
    }
    const int64_t cap_max = als_cg_lds_bytes(c) / als_cg_entry_bytes(kp);
    int64_t caps[ALS_CG_CLASSES + 1];
    for (int q = 0; q < ALS_CG_CLASSES; ++q) caps[q] = cap_max >> (ALS_CG_CLASSES - 1 - q);
    caps[ALS_CG_CLASSES] = 0;                                   // the streamed class
    std::vector<int64_t> list[ALS_CG_CLASSES + 1];
    int64_t nnz = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        int64_t len = 0;
        for (int s = 0; s < nobs; ++s) len += ip[s][(size_t)r + 1] - ip[s][(size_t)r];
        if (len > INT32_MAX) return fail(CMF_EUNSUPPORTED, "cmf_als_cg_step: a row with more than 2^31 - 1 stored entries");
        nnz += len;
        int q = 0;
        while (q < ALS_CG_CLASSES && len > caps[q]) ++q;
        list[q].push_back(r_begin + r);
    }
    std::vector<int64_t> all;
    all.reserve((size_t)nrows);
    for (int q = 0; q <= ALS_CG_CLASSES; ++q) all.insert(all.end(), list[q].begin(), list[q].end());
    CHK(kl_ensure(c, c->als_desc, std::max<size_t>(16, all.size() * sizeof(int64_t))));
    int64_t *drows = (int64_t *)c->als_desc.p;
    if (!all.empty()) HIPCHK(hipMemcpyAsync(drows, all.data(), all.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vector may go
    a.Fin = c->F[f];
    a.Fout = Fout;
    a.out_row0 = out_row0;
    a.l2 = (float)l2;
    a.k = c->k;
    a.steps = steps;
    Timed tm(c, CMF_K_ROWHESS, (4.0 * (double)nnz * c->k + (a.S ? 2.0 * (double)nrows * c->k * c->k : 0.0)) * (steps + 1));
    int64_t done = 0;
    for (int q = 0; q <= ALS_CG_CLASSES; ++q) {
        a.rows = drows + done;
        a.cap = (int)caps[q];
        CHK(als_cg_launch(c, a, (int64_t)list[q].size()));
        done += (int64_t)list[q].size();
    }
    return CMF_OK;
}

// sweeps == 0: the solved rows of the factors in nn_mask are projected; sweeps > 0: those factors are swept by coordinate descent;
// cg_steps > 0: a signed factor with an observed relation runs that many CG steps per row instead of the exact solves
static int als_step(cmf_ctx *c, double l2, int nn_mask, int mask, int sweeps, int cg_steps = 0) {
    DeviceGuard dg(c->device);
    const int bits[3] = {CMF_UPD_V, CMF_UPD_U, CMF_UPD_Z}, fs[3] = {CMF_V, CMF_U, CMF_Z}; // sweep order V, U, Z (cmf_solvers.py:248-263)
    const int nnb[3] = {CMF_NN_V, CMF_NN_U, CMF_NN_Z};
    for (int s = 0; s < 3; ++s) {
        if (!(mask & bits[s])) continue;
        const int f = fs[s];
        const bool nn = (nn_mask & nnb[s]) != 0;
        if (c->frows[f] <= 0) continue;
        if (!als_observed(c, f)) {
            if (nn && sweeps) CHK(als_nnls_sweep_shared(c, f, l2, sweeps));
            else CHK(als_sweep_shared(c, f, l2, nn));
            continue;
        }
        if (nn && sweeps) {
            CHK(als_rows(c, f, l2, 0, c->frows[f], true, nullptr, nullptr, sweeps));
            continue;
        }
        if (!nn && cg_steps) {
            CHK(als_cg_rows(c, f, l2, 0, c->frows[f], cg_steps, c->F[f], 0));
            continue;
        }
        CHK(als_rows(c, f, l2, 0, c->frows[f], true, nullptr, nullptr));
        CHK(als_apply(c, f, (const float *)c->als_sol.p, nn));
    }
    return CMF_OK;
}

extern "C" int cmf_als_step(cmf_ctx *c, double l2, int nn_mask, int mask) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_step", l2, mask));
    return als_step(c, l2, nn_mask, mask, 0);
}

static int als_nnls_sweeps_ok(const char *what, int sweeps) {
    if (sweeps < 1 || sweeps > 1024) return fail(CMF_EINVAL, "%s: sweeps must be 1 .. 1024, got %d", what, sweeps);
    return CMF_OK;
}

extern "C" int cmf_als_nnls_step(cmf_ctx *c, double l2, int nn_mask, int mask, int sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_nnls_step", l2, mask));
    CHK(als_nnls_sweeps_ok("cmf_als_nnls_step", sweeps));
    return als_step(c, l2, nn_mask, mask, sweeps);
}

static int als_cg_steps_ok(const char *what, int cg_steps) {
    if (cg_steps < 1 || cg_steps > 1024) return fail(CMF_EINVAL, "%s: cg_steps must be 1 .. 1024, got %d", what, cg_steps);
    return CMF_OK;
}

extern "C" int cmf_als_cg_step(cmf_ctx *c, double l2, int nn_mask, int mask, int cg_steps, int nn_sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_cg_step", l2, mask));
    CHK(als_cg_steps_ok("cmf_als_cg_step", cg_steps));
    if (nn_sweeps < 0 || nn_sweeps > 1024) return fail(CMF_EINVAL, "cmf_als_cg_step: nn_sweeps must be 0 .. 1024, got %d", nn_sweeps);
    return als_step(c, l2, nn_mask, mask, nn_sweeps, cg_steps);
}

// test entry: the rows the CG route would write for rows [row0, row0 + nrows) of sweep `which`; the factors are left alone
extern "C" int cmf_als_cg_rows(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, int cg_steps, float *host_f) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "cmf_als_cg_rows: bad factor selector");
    CHK(als_check(c, "cmf_als_cg_rows", l2, 1 << which));
    CHK(als_cg_steps_ok("cmf_als_cg_rows", cg_steps));
    if (row0 < 0 || nrows < 0 || row0 + nrows > c->frows[which]) return fail(CMF_EINVAL, "cmf_als_cg_rows: rows out of range");
    if (!als_observed(c, which)) return fail(CMF_EINVAL, "cmf_als_cg_rows: this sweep has no observed relation: one shared matrix, no per-row systems");
    if (nrows == 0) return CMF_OK;
    if (!host_f) return fail(CMF_EINVAL, "cmf_als_cg_rows: null output");
    DeviceGuard dg(c->device);
    const size_t bytes = (size_t)nrows * c->kp * sizeof(float);
    CHK(kl_ensure(c, c->als_cg_ws, bytes));
    HIPCHK(hipMemsetAsync(c->als_cg_ws.p, 0, bytes, c->stream));
    CHK(als_cg_rows(c, which, l2, row0, row0 + nrows, cg_steps, (float *)c->als_cg_ws.p, row0));
    HIPCHK(hipMemcpyAsync(host_f, c->als_cg_ws.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

// test entry: the kernel on the caller's systems (cmf_als_normal's layout), f in / out
extern "C" int cmf_als_nnls_rows(cmf_ctx *c, int64_t nrows, const float *host_H, const float *host_g, float *host_f, int sweeps) {
    NEED_PROBLEM(c);
    if (!host_H || !host_g || !host_f || nrows < 0) return fail(CMF_EINVAL, "cmf_als_nnls_rows: null pointer or negative row count");
    CHK(als_nnls_sweeps_ok("cmf_als_nnls_rows", sweeps));
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_als_nnls_rows: n_components <= 256 only (k_pad = %d)", c->kp);
    if (nrows == 0) return CMF_OK;
    DeviceGuard dg(c->device);
    const int64_t kp = c->kp, nh = nrows * kp * kp, nv = nrows * kp;
    CHK(kl_ensure(c, c->als_nnls_ws, (size_t)(nh + 2 * nv) * sizeof(float)));
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
    if (!als_observed(c, which)) return fail(CMF_EINVAL, "cmf_als_normal: this sweep has no observed relation: one shared matrix, no per-row systems");
    if (nrows == 0) return CMF_OK;
    DeviceGuard dg(c->device);
    return als_rows(c, which, l2, row0, row0 + nrows, false, host_H, host_g);
}

extern "C" int cmf_als_layout(cmf_ctx *c, int64_t *out4) {
    NEED_PROBLEM(c);
    if (!out4) return fail(CMF_EINVAL, "cmf_als_layout: null output");
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_als_layout: n_components <= 256 only (k_pad = %d)", c->kp);
    DeviceGuard dg(c->device);
    out4[0] = als_piece_len(c);
    const int fs[3] = {CMF_U, CMF_V, CMF_Z};
    for (int s = 0; s < 3; ++s) {
        AlsRel rel[2], obs[2];
        const int nrel = als_rels(fs[s], rel);
        int nobs = 0;
        for (int q = 0; q < nrel; ++q)
            if (c->wm_kind[rel[q].which] == WM_CSR) obs[nobs++] = rel[q];
        AlsPlan pl;
        if (nobs) CHK(als_plan(c, obs, nobs, 0, c->frows[fs[s]], pl));
        out4[1 + s] = (int64_t)pl.pieces.size();
    }
    return CMF_OK;
}

#endif // CMF_ALS_HOST
