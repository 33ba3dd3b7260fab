// cmf_als_dual.hip.h -- exact ALS rows of few stored entries in DUAL form (cmf_als_dual_step, cmf_als.hip.h)
// A row f_i of a swept factor whose sweep has no shared term (every relation observed, no background weight: S = N = null) and reads
// no logistic relation solves, on the exact route,
//   (A^T A + l2 I_k) f = A^T y,      a_e = sqrt(w_e) b_e  (A: n x k),    y_e = p_e / sqrt(w_e)  (0 where w_e = 0),
// over its n stored entries e (side 0 then side 1, stored order; p = w t as als_side_targets hands it, bias terms taken off).
// Because A^T (A A^T + l2 I_n)^-1 = (A^T A + l2 I_k)^-1 A^T the same row is
//   K = A A^T + l2 I_n,     K z = y,     f = A^T z:
// an n x n system instead of a k x k one.  lambda_min(K) >= l2, and cond(K) is bounded by that of the primal matrix.  With NP(n) the
// smallest of 32, 64, 128 that is >= n, a row goes dual when 1 <= n <= dual_max and NP(n) < k_pad (the dual system is strictly the
// smaller one); a row without a stored entry is zeros; every other row of the sweep takes the formed route of cmf_als.hip.h,
// restricted to those rows (als_list_rows below: the unchanged kernels on compact slots, then a scatter).
//
// als_dual_gram_kernel<KP, NP>: one 256-thread workgroup per row (NP = 32: four rows, one wave each).  The sqrt(w_e)-scaled gathered
//   rows are staged 64 columns of k at a time into ONE LDS image [NP][64 + 4] (16 lanes x f32x4 per gathered row, all loads of a
//   chunk in flight before the first store); the 32 x 32 blocks of K on or below the block diagonal are accumulated on
//   v_mfma_f32_32x32x2_f32 with BOTH operands read from that image (lane (l31, lh) reads 4 consecutive k of row 32 b + l31 by one
//   ds_read_b128, which serves 4 MFMAs; pitch 68: conflict-free).  Blocks per wave, wave-uniform:
//       NP = 128   wave 0: (0,0) (1,0) (1,1)   wave 1: (2,0) (2,1) (2,2)   wave 2: (3,0) (3,1)   wave 3: (3,2) (3,3)
//       NP = 64    wave 0: (0,0)   wave 1: (1,0)   wave 2: (1,1)
//       NP = 32    wave w: block (0,0) of the workgroup's row w
//   The k-chunks are added in ascending order.  K goes to scratch [row][NP][NP], both triangles (a block below the diagonal also
//   leaves transposed, f32x4 at a time), l2 on the WHOLE diagonal: a padding coordinate is l2 z = 0.  y goes to [row][NP], exact
//   zeros on padding entries and where w_e = 0.  Vector stores only, no atomics, no scratch memory.
// The solve is safe_solve_rows (cmf_newton.hip.h) on NP x NP matrices, as als_rows_solve calls it.
// als_dual_back_kernel<KP>: one wave per row: f = sum_e (sqrt(w_e) z_e) b_e over the entries in stored order, one accumulator chain
//   per coordinate (KP / 64 floats per lane, ALS_CG_U loads in flight): the sum order is the stored order whatever the launch shape.
//   Coordinates j < k only, max(., 0) for a projected non-negative factor; the padding is never written.
// Nothing is shared between rows: a row's result depends on that row alone, to the bit.
#pragma once
#include "cmf_kernels.hip.h"
#include "cmf_als_cg.hip.h"

namespace cmfk {

struct AlsDualArgs {
    AlsCgSide s0, s1;       // s1.indptr == nullptr: one side
    const int64_t *rows;    // the rows of this launch; slot q of the scratch belongs to rows[q]
    int64_t nrows;
    float *K, *y;           // [slot][NP][NP], [slot][NP]
    const float *z;         // [slot][NP]: the solved dual systems (back-product)
    float *Fout;            // where row r goes: Fout + (r - out_row0) * KP
    int64_t out_row0;
    float l2;
    int k, nn;
};

enum { ALS_DUAL_KC = 64, ALS_DUAL_PITCH = ALS_DUAL_KC + 4 };

template <int NP>
struct AlsDualCfg {
    static constexpr int RPW = NP == 32 ? 4 : 1;        // rows per workgroup
    static constexpr int GPR = 16 / RPW;                // 16-lane loader groups per row
    static constexpr int PASSES = NP / GPR;             // gathered rows per loader group and k-chunk
    static constexpr int MAXB = NP == 128 ? 3 : 1;      // blocks per wave
};

template <int KP, int NP>
__global__ __launch_bounds__(256) void als_dual_gram_kernel(AlsDualArgs g) {
    using C = AlsDualCfg<NP>;
    constexpr int P = ALS_DUAL_PITCH, KC = ALS_DUAL_KC;
    static_assert(KP % KC == 0 && NP < KP, "the dual system is the smaller one");
    __shared__ __attribute__((aligned(16))) float img[C::RPW * NP * P];
    __shared__ const float *esrc[C::RPW * NP];          // the gathered row of entry e (null past the end of the row)
    __shared__ float esq[C::RPW * NP];                  // sqrt(w_e)
    const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, lh = lane >> 5;
    const int uw = __builtin_amdgcn_readfirstlane(t >> 6);

    for (int i = t; i < C::RPW * NP; i += 256) {
        const int rs = i / NP, e = i % NP;
        const int64_t slot = (int64_t)blockIdx.x * C::RPW + rs;
        const float *src = nullptr;
        float sq = 0.f, yv = 0.f;
        if (slot < g.nrows) {
            const int64_t row = g.rows[slot];
            const int64_t b0 = g.s0.indptr[row], b1 = g.s1.indptr ? g.s1.indptr[row] : 0;
            const int n0 = (int)(g.s0.indptr[row + 1] - b0), n1 = g.s1.indptr ? (int)(g.s1.indptr[row + 1] - b1) : 0;
            if (e < n0 + n1) {
                const bool second = e >= n0;
                const int64_t q = second ? b1 + (e - n0) : b0 + e;
                const float w = (second ? g.s1.wv : g.s0.wv)[q];
                sq = sqrtf(w);
                if (w > 0.f) yv = (second ? g.s1.pv : g.s0.pv)[q] / sq;
                src = (second ? g.s1.B : g.s0.B) + (int64_t)(second ? g.s1.idx : g.s0.idx)[q] * KP;
            }
            g.y[slot * NP + e] = yv;
        }
        esrc[i] = src;
        esq[i] = sq;
    }

    // this wave's blocks (bi >= bj) of its row's K: wave-uniform
    int nb = 0, bi[C::MAXB], bj[C::MAXB], wrs = 0;
#pragma unroll
    for (int b = 0; b < C::MAXB; ++b) bi[b] = bj[b] = 0;
    if constexpr (NP == 128) {
        nb = uw < 2 ? 3 : 2;
        if (uw == 0) { bi[1] = 1; bi[2] = 1; bj[2] = 1; }
        else if (uw == 1) { bi[0] = bi[1] = bi[2] = 2; bj[1] = 1; bj[2] = 2; }
        else if (uw == 2) { bi[0] = bi[1] = 3; bj[1] = 1; }
        else { bi[0] = bi[1] = 3; bj[0] = 2; bj[1] = 3; }
    } else if constexpr (NP == 64) {
        nb = uw < 3 ? 1 : 0;
        bi[0] = uw >= 1 ? 1 : 0;
        bj[0] = uw == 2 ? 1 : 0;
    } else {
        nb = 1;
        wrs = uw;
    }
    f32x16 acc[C::MAXB];
#pragma unroll
    for (int b = 0; b < C::MAXB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;

    const int lg = t >> 4, tl = t & 15;                  // loader group, its 16-byte column of the chunk
    const int li0 = (lg / C::GPR) * NP + lg % C::GPR;    // entry of pass 0 (row slot * NP + e); pass p: + GPR p
    __syncthreads();
    for (int kc = 0; kc < KP; kc += KC) {
        f32x4 rr[C::PASSES];
#pragma unroll
        for (int p = 0; p < C::PASSES; ++p) {
            const float *src = esrc[li0 + C::GPR * p];
            rr[p] = src ? *reinterpret_cast<const f32x4 *>(src + kc + 4 * tl) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int p = 0; p < C::PASSES; ++p) {
            const int i = li0 + C::GPR * p;
            *reinterpret_cast<f32x4 *>(img + i * P + 4 * tl) = esq[i] * rr[p];
        }
        __syncthreads();
        const float *R = img + (wrs * NP + l31) * P + 4 * lh;
#pragma unroll
        for (int kq = 0; kq < KC; kq += 8) {
#pragma unroll
            for (int b = 0; b < C::MAXB; ++b) {
                if (b < nb) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4 *>(R + 32 * bi[b] * P + kq);
                    const f32x4 b4 = *reinterpret_cast<const f32x4 *>(R + 32 * bj[b] * P + kq);
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[s], b4[s], acc[b], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                 // the image is rewritten by the next chunk
    }

    // register r of a lane: row (r & 3) + 8 (r >> 2) + 4 lh of the block (the A fragment's rows), column l31 (the B fragment's)
    const int64_t slot = (int64_t)blockIdx.x * C::RPW + wrs;
    if (slot >= g.nrows) return;
    float *Kd = g.K + slot * NP * NP;
#pragma unroll
    for (int b = 0; b < C::MAXB; ++b) {
        if (b < nb) {
            const bool diag = bi[b] == bj[b];
            float *dst = Kd + (32 * bi[b] + 4 * lh) * NP + 32 * bj[b] + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int br = (r & 3) + 8 * (r >> 2);
                float v = acc[b][r];
                if (diag && br + 4 * lh == l31) v += g.l2;
                dst[br * NP] = v;
            }
            if (!diag) {
                float *mir = Kd + (32 * bj[b] + l31) * NP + 32 * bi[b] + 4 * lh;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<f32x4 *>(mir + 8 * q) = f32x4{acc[b][4 * q], acc[b][4 * q + 1], acc[b][4 * q + 2], acc[b][4 * q + 3]};
            }
        }
    }
}

// f = sum_e (sqrt(w_e) z_e) b_e: one wave per row, the entries in stored order
template <int KP>
__global__ __launch_bounds__(256) void als_dual_back_kernel(AlsDualArgs g, int np) {
    constexpr int VPL = KP / 64;
    static_assert(KP >= 64, "a dual row has k_pad >= 64");
    const int lane = threadIdx.x & 63;
    const int uw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t slot = (int64_t)blockIdx.x * 4 + uw;
    if (slot >= g.nrows) return;                         // wave-uniform; the kernel has no barrier
    const int64_t row = g.rows[slot];
    const int64_t b0 = g.s0.indptr[row], b1 = g.s1.indptr ? g.s1.indptr[row] : 0;
    const int n0 = (int)(g.s0.indptr[row + 1] - b0), n1 = g.s1.indptr ? (int)(g.s1.indptr[row + 1] - b1) : 0;
    const int n = n0 + n1;
    const float *z = g.z + slot * np;
    float acc[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) acc[v] = 0.f;
    for (int e0 = 0; e0 < n; e0 += ALS_CG_U) {
        float b[ALS_CG_U][VPL], coef[ALS_CG_U];
#pragma unroll
        for (int u = 0; u < ALS_CG_U; ++u) {
            const int e = e0 + u;                        // wave-uniform
#pragma unroll
            for (int v = 0; v < VPL; ++v) b[u][v] = 0.f;
            coef[u] = 0.f;
            if (e >= n) continue;
            const bool second = e >= n0;
            const int64_t q = second ? b1 + (e - n0) : b0 + e;
            coef[u] = sqrtf((second ? g.s1.wv : g.s0.wv)[q]) * z[e];
            const float *src = (second ? g.s1.B : g.s0.B) + (int64_t)(second ? g.s1.idx : g.s0.idx)[q] * KP + lane * VPL;
            if constexpr (VPL == 4) {
                const f32x4 x4 = *reinterpret_cast<const f32x4 *>(src);
                b[u][0] = x4[0]; b[u][1] = x4[1]; b[u][2] = x4[2]; b[u][3] = x4[3];
            } else if constexpr (VPL == 2) {
                const float2 x2 = *reinterpret_cast<const float2 *>(src);
                b[u][0] = x2.x; b[u][1] = x2.y;
            } else {
                b[u][0] = src[0];
            }
        }
#pragma unroll
        for (int u = 0; u < ALS_CG_U; ++u)
#pragma unroll
            for (int v = 0; v < VPL; ++v) acc[v] = fmaf(coef[u], b[u][v], acc[v]);
    }
    float *out = g.Fout + (row - g.out_row0) * KP + lane * VPL;
#pragma unroll
    for (int v = 0; v < VPL; ++v)
        if (lane * VPL + v < g.k) out[v] = g.nn ? fmaxf(acc[v], 0.f) : acc[v];
}

// row rows[q] of Fout <- the solved row of compact slot q (projected where asked) on the valid block; sol == nullptr: zeros
__global__ void als_dual_scatter_kernel(float *Fout, int64_t out_row0, const int64_t *rows, const float *sol, int64_t nrows, int k, int kp, int nn) {
    const int64_t n = nrows * kp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % kp);
        if (j >= k) continue;
        float v = sol ? sol[i] : 0.f;
        if (nn) v = fmaxf(v, 0.f);
        Fout[(rows[i / kp] - out_row0) * kp + j] = v;
    }
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als_bias.hip.h)
#ifdef CMF_ALS_DUAL_HOST

enum { ALS_DUAL_CLASSES = 3, ALS_DUAL_MAX = 128 };
static int als_dual_np(int64_t n) { return n <= 32 ? 32 : (n <= 64 ? 64 : 128); }

// why the sweep is not eligible for the dual route (null: it is): it must take ALS_ROWS_EXACT (the caller's test), every relation it
// reads must be observed without a background weight (als_shared_terms then gives S = N = null) and none may be logistic
static const char *als_dual_why_not(const cmf_ctx *c, const AlsSweep &sw) {
    if (!als_observed(sw)) return "no observed relation: one shared matrix, no per-row systems";
    for (int s = 0; s < sw.nrel; ++s)
        if (!sw.observed[s] || c->wm_bg[sw.rel[s].which] > 0.0) return "a shared term (a full relation or a background weight): the Woodbury form with a shared matrix is not built";
    if (als_logit_sweep(c, sw)) return "a logistic relation: reweighted dual rows are not built";
    return nullptr;
}

// The formed route over a row list: the systems of rows[0 .. n) (global rows of the sweep, which has S = N = null) by the unchanged
// als_normal_kernel / als_finish_kernel on compact slots, chunk by chunk, the unchanged safe_solve_rows, then the scatter.  pieces
// / first: the plan of the listed rows on the device (AlsPiece::row is the global row), hp / hfirst its host copy.  The pieces of a
// row, their order and the per-matrix solve are those of als_chunks: a listed row ends with the bits cmf_als_step gives it.
static int als_list_rows(cmf_ctx *c, const AlsSweep &sw, double l2, const int64_t *drows, int64_t n, const cmfk::AlsPiece *dpieces, const int64_t *dfirst,
                         const std::vector<cmfk::AlsPiece> &hp, const std::vector<int64_t> &hfirst, int64_t cap, bool nn, float *Fout, int64_t out_row0) {
    using namespace cmfk;
    if (n <= 0) return CMF_OK;
    const int kp = c->kp;
    const int64_t kk = (int64_t)kp * kp;
    int64_t max_rows = 0, max_pieces = 0;
    std::vector<int64_t> cuts{0};
    for (int64_t r = 0; r < n;) {                        // the chunk rule of als_chunks
        int64_t e = r;
        while (e < n && e - r < cap && (e == r || hfirst[(size_t)e + 1] - hfirst[(size_t)r] <= cap)) ++e;
        max_rows = std::max(max_rows, e - r);
        max_pieces = std::max(max_pieces, hfirst[(size_t)e] - hfirst[(size_t)r]);
        cuts.push_back(e);
        r = e;
    }
    CHK(ensure_scratch(c, c->als_h, (size_t)max_rows * kk * sizeof(float)));
    CHK(ensure_scratch(c, c->als_part, (size_t)std::max<int64_t>(1, max_pieces) * (kk + kp) * sizeof(float)));
    CHK(ensure_scratch(c, c->als_g, (size_t)max_rows * kp * sizeof(float)));
    CHK(ensure_scratch(c, c->als_sol, (size_t)max_rows * kp * sizeof(float)));
    AlsArgs a;
    memset(&a, 0, sizeof a);
    for (int s = 0; s < sw.nobs; ++s) {
        const WCsrDev &M = *sw.obs[s].M;
        (s == 0 ? a.s0 : a.s1) = AlsSide{M.idx, als_side_targets(M), als_side_weights(M), sw.obs[s].B};
    }
    float *Hc = (float *)c->als_h.p, *Hp = (float *)c->als_part.p, *grad = (float *)c->als_g.p, *sol = (float *)c->als_sol.p;
    a.Hp = Hp;
    a.gp = Hp + std::max<int64_t>(1, max_pieces) * kk;
    const double pert = l2 / 16.0;                       // als_rows_solve's threshold
    for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
        const int64_t c0 = cuts[ci], c1 = cuts[ci + 1], nr = c1 - c0;
        const int64_t pbase = hfirst[(size_t)c0], np = hfirst[(size_t)c1] - pbase;
        a.pieces = dpieces + pbase;
        int64_t nnz = 0;
        for (int64_t p = pbase; p < pbase + np; ++p) nnz += hp[(size_t)p].len;
        CHK(als_launch_normal(c, a, np, nnz, false));
        {
            Timed tm(c, CMF_K_ELEMWISE);
            hipLaunchKernelGGL(als_finish_kernel, dim3((unsigned)nr), dim3(256), 0, c->stream, (const float *)Hp, (const float *)a.gp, dfirst + c0, pbase,
                               (const float *)nullptr, (const float *)nullptr, (float)l2, c->k, kp, Hc, grad);
            HIPCHK(hipGetLastError());
        }
        {
            AlsNewtonStateGuard keep(c);
            c->hess_psd = true;
            CHK(safe_solve_rows(c, Hc, grad, sol, nr, c->k, kp, pert));
        }
        CHK(launch_ew(c, als_dual_scatter_kernel, nr * kp, Fout, out_row0, drows + c0, (const float *)sol, nr, c->k, kp, nn ? 1 : 0));
    }
    return CMF_OK;
}

template <int KP>
static int als_dual_launch_class(cmf_ctx *c, const cmfk::AlsDualArgs &a, int np) {
    using namespace cmfk;
    const dim3 block(256);
    if constexpr (KP > 32) {
        if (np == 32) hipLaunchKernelGGL((als_dual_gram_kernel<KP, 32>), dim3((unsigned)((a.nrows + 3) / 4)), block, 0, c->stream, a);
    }
    if constexpr (KP > 64) {
        if (np == 64) hipLaunchKernelGGL((als_dual_gram_kernel<KP, 64>), dim3((unsigned)a.nrows), block, 0, c->stream, a);
    }
    if constexpr (KP > 128) {
        if (np == 128) hipLaunchKernelGGL((als_dual_gram_kernel<KP, 128>), dim3((unsigned)a.nrows), block, 0, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// Rows [r_begin, r_end) of an ELIGIBLE sweep (als_dual_why_not is null) under the permission dual_max >= 1: the dual rows class by
// class (Gram, solve, back-product, in chunks of rows whose K scratch stays within the byte budget hessian_chunk_rows gives the
// exact route), zeros for the rows without a stored entry, the formed route for the rest.  Row r goes to Fout + (r - out_row0) k_pad.
// none_dual (a whole sweep): when no row of the plan goes dual nothing is launched and *none_dual is set -- the caller runs the
// exact sweep as it stands (the same bits: a formed row keeps them, a row without an entry solves l2 f = 0), without the row list.
static int als_dual_rows(cmf_ctx *c, const AlsSweep &sw, double l2, int64_t r_begin, int64_t r_end, int dual_max, bool nn, float *Fout, int64_t out_row0,
                         bool *none_dual = nullptr) {
    using namespace cmfk;
    const int kp = c->kp;
    const int64_t nrows = r_end - r_begin;
    std::vector<int64_t> ip[2];
    CHK(als_fetch_indptr(c, sw, r_begin, r_end, ip));
    const int64_t L = als_piece_len(c);
    if (none_dual) {   // a first pass that only counts: a sweep without a dual row builds no list and no piece
        int64_t n_dual = 0, n_zero = 0;
        for (int64_t r = 0; r < nrows; ++r) {
            int64_t len = 0;
            for (int s = 0; s < sw.nobs; ++s) len += ip[s][(size_t)r + 1] - ip[s][(size_t)r];
            n_zero += len == 0;
            n_dual += len > 0 && len <= dual_max && als_dual_np(len) < kp;
        }
        *none_dual = n_dual == 0;
        if (*none_dual) {
            c->als_dual_last[0] = c->als_dual_last[1] = c->als_dual_last[2] = 0;
            c->als_dual_last[3] = nrows - n_zero;
            c->als_dual_last[4] = n_zero;
            return CMF_OK;
        }
    }
    std::vector<int64_t> list[ALS_DUAL_CLASSES], zeros, formed, first{0};
    std::vector<AlsPiece> pieces;
    for (int64_t r = 0; r < nrows; ++r) {
        int64_t len = 0;
        for (int s = 0; s < sw.nobs; ++s) len += ip[s][(size_t)r + 1] - ip[s][(size_t)r];
        if (len == 0) { zeros.push_back(r_begin + r); continue; }
        if (len <= dual_max && als_dual_np(len) < kp) {
            list[als_dual_np(len) == 32 ? 0 : (als_dual_np(len) == 64 ? 1 : 2)].push_back(r_begin + r);
            continue;
        }
        formed.push_back(r_begin + r);
        for (int s = 0; s < sw.nobs; ++s) {              // the pieces of als_cut_rows: image by image
            const int64_t e = ip[s][(size_t)r + 1];
            for (int64_t q = ip[s][(size_t)r]; q < e; q += L) pieces.push_back(AlsPiece{q, (int32_t)std::min(L, e - q), s, r_begin + r});
        }
        first.push_back((int64_t)pieces.size());
    }
    for (int q = 0; q < ALS_DUAL_CLASSES; ++q) c->als_dual_last[q] = (int64_t)list[q].size();
    c->als_dual_last[3] = (int64_t)formed.size();
    c->als_dual_last[4] = (int64_t)zeros.size();

    // descriptors, once per sweep: the rows of the three classes | the zero rows | the formed rows | their first[] | their pieces
    std::vector<int64_t> all;
    all.reserve((size_t)nrows + first.size());
    for (int q = 0; q < ALS_DUAL_CLASSES; ++q) all.insert(all.end(), list[q].begin(), list[q].end());
    all.insert(all.end(), zeros.begin(), zeros.end());
    all.insert(all.end(), formed.begin(), formed.end());
    const size_t nlisted = all.size();
    all.insert(all.end(), first.begin(), first.end());
    const size_t abytes = all.size() * sizeof(int64_t);
    CHK(ensure_scratch(c, c->als_desc, abytes + std::max<size_t>(16, pieces.size() * sizeof(AlsPiece))));
    int64_t *drows = (int64_t *)c->als_desc.p;
    const int64_t *dfirst = drows + nlisted;
    AlsPiece *dpieces = (AlsPiece *)((char *)c->als_desc.p + abytes);
    HIPCHK(hipMemcpyAsync(drows, all.data(), abytes, hipMemcpyHostToDevice, c->stream));
    if (!pieces.empty()) HIPCHK(hipMemcpyAsync(dpieces, pieces.data(), pieces.size() * sizeof(AlsPiece), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vectors may go

    const int64_t cap_exact = hessian_chunk_rows(c, c->frows_pad[sw.f]);
    const int64_t budget = cap_exact * kp * kp;          // floats of K scratch a chunk may take: the exact route's
    AlsDualArgs a;
    memset(&a, 0, sizeof a);
    for (int s = 0; s < sw.nobs; ++s) {
        const WCsrDev &M = *sw.obs[s].M;
        (s == 0 ? a.s0 : a.s1) = AlsCgSide{M.indptr, M.idx, als_side_targets(M), als_side_weights(M), sw.obs[s].B};
    }
    a.Fout = Fout;
    a.out_row0 = out_row0;
    a.l2 = (float)l2;
    a.k = c->k;
    a.nn = nn ? 1 : 0;
    const double pert = l2 / 16.0;
    int64_t done = 0;
    for (int q = 0; q < ALS_DUAL_CLASSES; ++q) {
        const int np = 32 << q;
        const int64_t n = (int64_t)list[q].size(), per = (int64_t)np * np;
        const int64_t cap = std::max<int64_t>(4, budget / per / 4 * 4);
        for (int64_t r0 = 0; r0 < n; r0 += cap) {
            const int64_t nr = std::min(cap, n - r0);
            CHK(ensure_scratch(c, c->als_dual_ws, (size_t)nr * (per + 2 * np) * sizeof(float)));
            a.rows = drows + done + r0;
            a.nrows = nr;
            a.K = (float *)c->als_dual_ws.p;
            a.y = a.K + nr * per;
            float *z = a.y + nr * np;
            a.z = z;
            {
                Timed tm(c, CMF_K_ROWHESS, 2.0 * (double)nr * np * np * c->k);
                switch (kp) {
                case 64: CHK(als_dual_launch_class<64>(c, a, np)); break;
                case 128: CHK(als_dual_launch_class<128>(c, a, np)); break;
                case 256: CHK(als_dual_launch_class<256>(c, a, np)); break;
                default: return fail(CMF_EUNSUPPORTED, "the dual ALS rows are built for k_pad 64, 128 and 256 (k_pad = %d)", kp);
                }
            }
            {
                AlsNewtonStateGuard keep(c);
                c->hess_psd = true;
                CHK(safe_solve_rows(c, a.K, a.y, z, nr, np, np, pert));
            }
            {
                Timed tm(c, CMF_K_ELEMWISE);
                const dim3 grid((unsigned)((nr + 3) / 4)), block(256);
                switch (kp) {
                case 64: hipLaunchKernelGGL((als_dual_back_kernel<64>), grid, block, 0, c->stream, a, np); break;
                case 128: hipLaunchKernelGGL((als_dual_back_kernel<128>), grid, block, 0, c->stream, a, np); break;
                default: hipLaunchKernelGGL((als_dual_back_kernel<256>), grid, block, 0, c->stream, a, np); break;
                }
                HIPCHK(hipGetLastError());
            }
        }
        done += n;
    }
    if (!zeros.empty())
        CHK(launch_ew(c, als_dual_scatter_kernel, (int64_t)zeros.size() * kp, Fout, out_row0, (const int64_t *)(drows + done), (const float *)nullptr,
                      (int64_t)zeros.size(), c->k, kp, 0));
    done += (int64_t)zeros.size();
    return als_list_rows(c, sw, l2, drows + done, (int64_t)formed.size(), dpieces, dfirst, pieces, first, cap_exact, nn, Fout, out_row0);
}

static int als_dual_max_ok(const char *what, int dual_max) {
    if (dual_max < 0 || dual_max > ALS_DUAL_MAX) return fail(CMF_EINVAL, "%s: dual_max must be 0 .. %d, got %d", what, (int)ALS_DUAL_MAX, dual_max);
    return CMF_OK;
}

// the permission of als_step's exact row sweeps for the length of one entry point
struct AlsDualPermission {
    cmf_ctx *const c;
    const int before;
    AlsDualPermission(cmf_ctx *ctx, int dual_max) : c(ctx), before(ctx->als_dual_perm) { c->als_dual_perm = dual_max; }
    ~AlsDualPermission() { c->als_dual_perm = before; }
};

// als_step's hook (declared in cmf_als.hip.h): a sweep on ALS_ROWS_EXACT under a permission; *taken = false leaves it to the caller
static int als_dual_sweep(cmf_ctx *c, const AlsSweep &sw, double l2, bool nn, bool *taken) {
    *taken = c->als_dual_perm > 0 && c->kp > 32 && !als_dual_why_not(c, sw);   // (k_pad = 32: no class is below it)
    if (!*taken) return CMF_OK;
    bool none = false;
    CHK(als_dual_rows(c, sw, l2, 0, c->frows[sw.f], c->als_dual_perm, nn, c->F[sw.f], 0, &none));
    *taken = !none;
    return CMF_OK;
}

extern "C" int cmf_als_dual_step(cmf_ctx *c, double l2, int nn_mask, int mask, int dual_max, int nn_sweeps, int nn_cg_steps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_dual_step", l2, mask));
    CHK(als_dual_max_ok("cmf_als_dual_step", dual_max));
    CHK(als_count_ok("cmf_als_dual_step", "nn_sweeps", nn_sweeps, 0));
    CHK(als_count_ok("cmf_als_dual_step", "nn_cg_steps", nn_cg_steps, 0));
    if (nn_cg_steps && als_bias_any(c))
        return fail(CMF_EUNSUPPORTED, "cmf_als_dual_step: nn_cg_steps with biases bound is not built (cmf_als_nncg_step): pass nn_cg_steps = 0");
    AlsDualPermission perm(c, dual_max);
    if (nn_cg_steps) return cmf_als_nncg_step(c, l2, nn_mask, mask, 0, nn_cg_steps, nn_sweeps);
    if (als_bias_any(c)) return cmf_als_bias_step(c, l2, nn_mask, mask, 0, nn_sweeps);
    return nn_sweeps ? cmf_als_nnls_step(c, l2, nn_mask, mask, nn_sweeps) : cmf_als_step(c, l2, nn_mask, mask);
}

// test entry: the rows an eligible sweep `which` would write for rows [row0, row0 + nrows) under dual_max; the factors are left alone
extern "C" int cmf_als_dual_rows(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, int dual_max, float *host_f) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "cmf_als_dual_rows: bad factor selector");
    CHK(als_check(c, "cmf_als_dual_rows", l2, 1 << which));
    CHK(als_dual_max_ok("cmf_als_dual_rows", dual_max));
    if (row0 < 0 || nrows < 0 || row0 + nrows > c->frows[which]) return fail(CMF_EINVAL, "cmf_als_dual_rows: rows out of range");
    const AlsSweep sw = als_sweep(c, which);
    if (const char *why = als_dual_why_not(c, sw)) return fail(CMF_EINVAL, "cmf_als_dual_rows: this sweep is not eligible: %s", why);
    if (nrows == 0) return CMF_OK;
    if (!host_f) return fail(CMF_EINVAL, "cmf_als_dual_rows: null output");
    DeviceGuard dg(c->device);
    for (int s = 0; s < sw.nrel; ++s) CHK(als_bias_refresh(c, sw.rel[s].which));   // (written when the biases last changed: nothing to do)
    const size_t bytes = (size_t)nrows * c->kp * sizeof(float);
    CHK(ensure_scratch(c, c->als_cg_ws, bytes));
    HIPCHK(hipMemsetAsync(c->als_cg_ws.p, 0, bytes, c->stream));
    CHK(als_dual_rows(c, sw, l2, row0, row0 + nrows, dual_max, false, (float *)c->als_cg_ws.p, row0));
    HIPCHK(hipMemcpyAsync(host_f, c->als_cg_ws.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

// test entry: rows in class 32, 64 and 128, rows left to the formed route and rows written as zeros in the last dual sweep (or
// cmf_als_dual_rows call)
extern "C" int cmf_als_dual_last(cmf_ctx *c, int64_t *out5) {
    if (!c || !out5) return fail(CMF_EINVAL, "cmf_als_dual_last: null context or output");
    for (int q = 0; q < 5; ++q) out5[q] = c->als_dual_last[q];
    return CMF_OK;
}

#endif // CMF_ALS_DUAL_HOST
