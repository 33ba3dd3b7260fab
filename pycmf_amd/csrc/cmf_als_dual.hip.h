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
// restricted to those rows (a plan of listed rows through the one chunk loop: the unchanged kernels on compact slots, then a scatter).
// The planner is als_dual_rows (cmf_als_steps.hip.h); this file holds the kernels.
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
//   leaves transposed, f32x4 at a time), l2 (lambda_i = l2 * mult[row] under cmf_set_l2_rows) on the WHOLE diagonal: a padding coordinate is l2 z = 0.  y goes to [row][NP], exact
//   zeros on padding entries and where w_e = 0.  Vector stores only, no atomics, no scratch memory.
// The solve is the exact solve of the formed route (als_solve_rows: safe_solve_rows, cmf_newton.hip.h) on NP x NP matrices.
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
    const float *l2m;       // per-row multipliers of l2 (cmf_set_l2_rows), indexed by the row of the swept factor; null: the LR = false instance
};

enum { ALS_DUAL_KC = 64, ALS_DUAL_PITCH = ALS_DUAL_KC + 4 };

template <int NP>
struct AlsDualCfg {
    static constexpr int RPW = NP == 32 ? 4 : 1;        // rows per workgroup
    static constexpr int GPR = 16 / RPW;                // 16-lane loader groups per row
    static constexpr int PASSES = NP / GPR;             // gathered rows per loader group and k-chunk
    static constexpr int MAXB = NP == 128 ? 3 : 1;      // blocks per wave
};

template <int KP, int NP, bool LR>
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
    const float l2 = als_row_l2<LR>(g.l2, g.l2m, LR ? g.rows[slot] : 0);   // wave-uniform
#pragma unroll
    for (int b = 0; b < C::MAXB; ++b) {
        if (b < nb) {
            const bool diag = bi[b] == bj[b];
            float *dst = Kd + (32 * bi[b] + 4 * lh) * NP + 32 * bj[b] + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int br = (r & 3) + 8 * (r >> 2);
                float v = acc[b][r];
                if (diag && br + 4 * lh == l31) v += l2;
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
            als_lane_load<VPL>((second ? g.s1.B : g.s0.B) + (int64_t)(second ? g.s1.idx : g.s0.idx)[q] * KP + lane * VPL, b[u]);
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

