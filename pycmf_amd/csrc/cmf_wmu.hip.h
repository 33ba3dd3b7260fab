// cmf_wmu.hip.h -- multiplicative updates with per-entry weights on the Frobenius objective
//   1/2 |sqrt(Wx) .* (X - U V^T)|^2 + 1/2 |sqrt(Wy) .* (Y - V Z^T)|^2      (Wx, Wy >= 0, fixed; a 0/1 mask = observed entries only).
//
// The weighted update of a factor needs  D = (W .* (A B^T)) B : an element-wise product BETWEEN two products over the same tiles --
// the quotient pass of cmf_klmu.hip.h with  w s  in place of  t / s.  The m x d intermediate is never written to memory:
//
// wmu_pass_kernel<KP, TRANS, MODE>: the tile orientation, LDS layout, register staging and k pairing of kl_quotient_kernel (128
// owned rows of A in registers, B through 32 KB swizzled LDS tiles, shares of the streamed dimension leaving partial slabs).
//   WM_DEN   1. S^T = B_tile A_blk^T  2. the 16 registers times the 16 elements of W that face them (read as stored, TRANS = 0, or
//            transposed, TRANS = 1)  3. D^T += B_tile^T (W .* S)^T, the registers straight back as the B operand
//   WM_DEN1  W == 1: steps 1 and 3, no W loads (the unweighted relation of a weighted fit; no matrix of ones is ever allocated)
//   WM_NUM   step 3 alone, the registers loaded from P = W .* T (formed once when the weights are bound; for an unweighted
//            relation P is the data image itself): N = P B in the same tiles, shares and summation order as D
//   WM_RES / WM_RES1   step 1, then w (t - s)^2 (RES1: (t - s)^2) per valid element: every term in float32 in the DIRECT form,
//            per-lane float64 sums, one float64 partial per workgroup (summed by sum_doubles_kernel)
// A share whose slab already holds the other relation's contribution (V sweep: X^T side, then Y side) adds to it (acc_slabs).
// Every output element is one fma chain in an order fixed by this file and the share count; no floating-point atomics.
// Padding: rows and columns of W, T, A and B beyond the valid extent are zero and contribute exact zeros.
//
// wmu_csr_kernel<GL, CH>: weights held as CSR -- the loss runs over the stored pattern only.  One pattern, value arrays p = w t
// and w (and t on the row image, for the residual).  A group of GL lanes owns an output row; per stored entry the gathered row
// B_c serves the dot with the owned row (DPP group_sum), then den += (w dot) B_c and num += p B_c, in stored order.
// wmu_res_csr_kernel<GL, CH>: sum over the stored entries of w (t - A_r . B_c)^2.
// wmu_update_kernel: F <- F * (sum of the numerator slabs) / reg(sum of the denominator slabs, F)   (cmf_solvers.py:212-228, gamma = 1).
//
// No existing kernel is touched.  Reference counterpart: none -- its README lists "Add support for weight matrices on relations"
// as an open item.
#pragma once
#include "cmf_klmu.hip.h"

namespace cmfk {

enum { WM_DEN = 0, WM_DEN1 = 1, WM_NUM = 2, WM_RES = 3, WM_RES1 = 4 };

struct WmuArgs {
    const float *W;          // WM_DEN / WM_RES: dense weights; WM_NUM: the image P = W .* T
    const float *T;          // WM_RES / WM_RES1: dense data
    int64_t ldt;             // pitch of W, P and T (one relation: the same)
    const float *A;          // the factor that owns the output rows, pitch KP
    const float *B;          // the streamed factor, pitch KP
    int64_t cols_pad;        // streamed extent (multiple of 256)
    int64_t cols_per_share;  // multiple of 256
    int64_t rows_valid, cols_valid; // residual only
    float *out;              // [share][rows_pad][KP]
    int64_t slab_stride;
    int acc_slabs;           // shares below this one add to what their slab holds
    double *part;            // residual: one partial per workgroup
};

template <int KP, int TRANS, int MODE>
__device__ __forceinline__ void wmu_pass_body(const WmuArgs &g, f32x4 *tile) {
    constexpr bool RES = MODE == WM_RES || MODE == WM_RES1;
    constexpr bool HASW = MODE == WM_DEN || MODE == WM_NUM || MODE == WM_RES; // 16 elements through g.W per sub-tile
    constexpr bool DOT = MODE != WM_NUM;                                      // step 1 runs
    constexpr int CT = KL_TILE_FLOATS / KP;   // streamed rows per LDS tile (32 at KP = 256 ... 256 at KP = 32)
    constexpr int SLOTS = KP / 4;             // float4 slots per row
    constexpr int SW = (SLOTS < 16 ? SLOTS : 16) - 1; // slot ^ (row & SW): rows of one fragment read land on different banks
    constexpr int NCH = KP / 8;               // 8-deep k pieces: one float4 per lane half
    constexpr int KB = KP / 32;               // output accumulators per wave (32 columns each)
    constexpr int W = KB < 4 ? KB : 4;        // floats per LDS access of the second product
    constexpr int NJ = KB / W;
    constexpr int SUBS = CT / 32;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, li = lane & 31;
    const int64_t row = (int64_t)blockIdx.x * KL_RB + wave * 32 + li; // output row of this lane (rows_pad is a multiple of KL_RB)

    // the owned row in registers: piece c = floats 8 c + 4 h .. + 3
    f32x4 af[DOT ? NCH : 1];
    if constexpr (DOT) {
        const f32x4 *src = (const f32x4 *)(g.A + row * KP);
#pragma unroll
        for (int c = 0; c < NCH; ++c) af[c] = src[2 * c + h];
    }
    const int64_t c_begin = (int64_t)blockIdx.y * g.cols_per_share;
    const int64_t c_end = min(c_begin + g.cols_per_share, g.cols_pad);
    const int ntiles = c_end > c_begin ? (int)((c_end - c_begin) / CT) : 0;

    f32x16 nacc[RES ? 1 : KB];
#pragma unroll
    for (int kb = 0; kb < (RES ? 1 : KB); ++kb) nacc[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double dsum = 0.0;

    // staging: float4 number i * 256 + tid of the tile (8 per thread)
    f32x4 st[8];
    auto fetch = [&](int t) {
        const f32x4 *src = (const f32x4 *)(g.B + (c_begin + (int64_t)t * CT) * KP);
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = src[i * 256 + tid];
    };
    // the 16 elements of a relation-shaped image that face the accumulator registers of a sub-tile starting at streamed index cb
    auto fetch_e = [&](f32x4 *dst, const float *img, int64_t cb) {
        if constexpr (TRANS == 0) {
            const float *src = img + row * g.ldt + cb + 4 * h;
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q] = *(const f32x4 *)(src + 8 * q);
        } else {
            const float *src = img + (cb + 4 * h) * g.ldt + row;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) dst[q][j] = src[(int64_t)(8 * q + j) * g.ldt];
        }
    };
    f32x4 wv[4], wn[4], tv[4], tn[4];
    if (ntiles > 0) {
        fetch(0);
        if constexpr (HASW) fetch_e(wv, g.W, c_begin);
        if constexpr (RES) fetch_e(tv, g.T, c_begin);
    }

    for (int t = 0; t < ntiles; ++t) {
        __syncthreads(); // tile t - 1 has been read by every wave
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int gidx = i * 256 + tid, r = gidx / SLOTS, slot = gidx % SLOTS;
            tile[r * SLOTS + (slot ^ (r & SW))] = st[i];
        }
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1);

#pragma unroll 1
        for (int sub = 0; sub < SUBS; ++sub) {
            const int64_t cb = c_begin + (int64_t)t * CT + sub * 32;
            const bool more = sub + 1 < SUBS || t + 1 < ntiles;
            if (more) {
                if constexpr (HASW) fetch_e(wn, g.W, cb + 32);
                if constexpr (RES) fetch_e(tn, g.T, cb + 32);
            }
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            if constexpr (DOT) {
                const int trow = sub * 32 + li;
                const f32x4 *arow = tile + trow * SLOTS;
                const int sw = trow & SW;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const f32x4 a = arow[(2 * c + h) ^ sw];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], af[c][0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], af[c][1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], af[c][2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], af[c][3], acc, 0, 0, 0);
                    if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0); // fragment reads at most four pieces ahead: the owned rows need the registers
                }
            }
            // register r of the lane: streamed row (r & 3) + 8 (r >> 2) + 4 h of the 32, output row lane & 31
            if constexpr (RES) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t col = cb + 8 * (r >> 2) + 4 * h + (r & 3);
                    if (row < g.rows_valid && col < g.cols_valid) {
                        const float e = tv[r >> 2][r & 3] - acc[r];
                        float term = e * e;
                        if constexpr (MODE == WM_RES) term = wv[r >> 2][r & 3] * term;
                        dsum += (double)term;
                    }
                }
            } else {
                if constexpr (MODE == WM_DEN) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = wv[r >> 2][r & 3] * acc[r];
                } else if constexpr (MODE == WM_NUM) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = wv[r >> 2][r & 3];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int brow = sub * 32 + 8 * (r >> 2) + 4 * h + (r & 3); // the streamed row register r stands for in this lane half
                    const float *bp = (const float *)(tile + brow * SLOTS);
                    const int sw2 = brow & SW;
#pragma unroll
                    for (int jj = 0; jj < NJ; ++jj) {
                        const int fo = W * (li + 32 * jj);                     // first of the W columns of this lane
                        const float *p = bp + ((((fo >> 2) ^ sw2) << 2) | (fo & 3));
                        if constexpr (W == 4) {
                            const f32x4 b = *(const f32x4 *)p;
#pragma unroll
                            for (int e = 0; e < 4; ++e) nacc[jj * 4 + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[e], acc[r], nacc[jj * 4 + e], 0, 0, 0);
                        } else if constexpr (W == 2) {
                            const f32x2 b = *(const f32x2 *)p;
                            nacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[0], acc[r], nacc[0], 0, 0, 0);
                            nacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[1], acc[r], nacc[1], 0, 0, 0);
                        } else {
                            nacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(*p, acc[r], nacc[0], 0, 0, 0);
                        }
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if constexpr (HASW) wv[q] = wn[q];
                    if constexpr (RES) tv[q] = tn[q];
                }
            }
        }
    }

    if constexpr (RES) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) dsum += __shfl_down(dsum, off, 64);
        double *red = (double *)tile;
        __syncthreads(); // the last tile has been read
        if (lane == 0) red[wave] = dsum;
        __syncthreads();
        if (tid == 0) g.part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    } else {
        // accumulator kb = jj W + e, register r2: column W (i + 32 jj) + e with i = (r2 & 3) + 8 (r2 >> 2) + 4 h; row = this lane's
        float *dst = g.out + (int64_t)blockIdx.y * g.slab_stride + row * KP;
        const bool add = (int)blockIdx.y < g.acc_slabs;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) {
                const int i = (r2 & 3) + 8 * (r2 >> 2) + 4 * h;
                float *p = dst + W * (i + 32 * jj);
                if constexpr (W == 4) {
                    f32x4 v = f32x4{nacc[jj * 4][r2], nacc[jj * 4 + 1][r2], nacc[jj * 4 + 2][r2], nacc[jj * 4 + 3][r2]};
                    if (add) v += *(const f32x4 *)p;
                    *(f32x4 *)p = v;
                } else if constexpr (W == 2) {
                    f32x2 v = f32x2{nacc[0][r2], nacc[1][r2]};
                    if (add) v += *(const f32x2 *)p;
                    *(f32x2 *)p = v;
                } else {
                    float v = nacc[0][r2];
                    if (add) v += *p;
                    *p = v;
                }
            }
    }
}

template <int KP, int TRANS, int MODE>
__global__ __launch_bounds__(256, KP >= 128 ? 1 : 2) void wmu_pass_kernel(WmuArgs g) {
    __shared__ __attribute__((aligned(16))) f32x4 wm_tile[KL_TILE_FLOATS / 4];
    wmu_pass_body<KP, TRANS, MODE>(g, wm_tile);
}
template <int KP, int MODE>
__global__ __launch_bounds__(256, KP == 256 ? 1 : 2) void wmu_res_kernel(WmuArgs g) {
    __shared__ __attribute__((aligned(16))) f32x4 wm_tile[KL_TILE_FLOATS / 4];
    wmu_pass_body<KP, 0, MODE>(g, wm_tile);
}

// ------------------------------------------------------------------ weights held as CSR
struct WCsrView {
    const int64_t *indptr;
    const int32_t *idx;
    const float *pv, *wv, *tv; // p = w t, w, t (tv: row image only)
    int64_t rows;
};

// num[r, :] (+)= sum over the stored (r, c) of p B_c,  den[r, :] (+)= sum of (w A_r . B_c) B_c;  rows beyond T.rows count as empty.
// GL = lanes per row group = KP / 4 (CH = 1 for every supported width, as in kl_quotient_csr_kernel)
template <int GL, int CH>
__global__ __launch_bounds__(256) void wmu_csr_kernel(WCsrView T, const float *A, const float *B, int kp, int64_t rows_pad, float *num, float *den, int add) {
    constexpr int RPW = 64 / GL;
    const int lane = threadIdx.x & 63;
    const int gl = lane % GL, gsub = lane / GL;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t row = wave * RPW + gsub;
    if (row >= rows_pad) return;
    f32x4 nu[CH], de[CH], a[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) nu[c] = de[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < T.rows) {
#pragma unroll
        for (int c = 0; c < CH; ++c) a[c] = *reinterpret_cast<const f32x4 *>(A + row * kp + 4 * (gl + GL * c));
        const int64_t beg = T.indptr[row], end = T.indptr[row + 1];
        int64_t q = beg;
        for (; q + 2 <= end; q += 2) { // two independent gathers in flight; the entries still enter the sums in stored order
            const int32_t j0 = T.idx[q], j1 = T.idx[q + 1];
            const float p0 = T.pv[q], p1 = T.pv[q + 1], w0 = T.wv[q], w1 = T.wv[q + 1];
            f32x4 b0[CH], b1[CH];
            float d0 = 0.f, d1 = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                b0[c] = *reinterpret_cast<const f32x4 *>(B + (int64_t)j0 * kp + 4 * (gl + GL * c));
                b1[c] = *reinterpret_cast<const f32x4 *>(B + (int64_t)j1 * kp + 4 * (gl + GL * c));
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                d0 += a[c][0] * b0[c][0] + a[c][1] * b0[c][1] + a[c][2] * b0[c][2] + a[c][3] * b0[c][3];
                d1 += a[c][0] * b1[c][0] + a[c][1] * b1[c][1] + a[c][2] * b1[c][2] + a[c][3] * b1[c][3];
            }
            d0 = w0 * group_sum<GL>(d0);
            d1 = w1 * group_sum<GL>(d1);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                de[c] += d0 * b0[c];
                nu[c] += p0 * b0[c];
                de[c] += d1 * b1[c];
                nu[c] += p1 * b1[c];
            }
        }
        if (q < end) {
            const int32_t j0 = T.idx[q];
            const float p0 = T.pv[q], w0 = T.wv[q];
            f32x4 b0[CH];
            float d0 = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                b0[c] = *reinterpret_cast<const f32x4 *>(B + (int64_t)j0 * kp + 4 * (gl + GL * c));
                d0 += a[c][0] * b0[c][0] + a[c][1] * b0[c][1] + a[c][2] * b0[c][2] + a[c][3] * b0[c][3];
            }
            d0 = w0 * group_sum<GL>(d0);
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                de[c] += d0 * b0[c];
                nu[c] += p0 * b0[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        f32x4 *pn = reinterpret_cast<f32x4 *>(num + row * kp + 4 * (gl + GL * c));
        f32x4 *pd = reinterpret_cast<f32x4 *>(den + row * kp + 4 * (gl + GL * c));
        if (add) {
            nu[c] += *pn;
            de[c] += *pd;
        }
        *pn = nu[c];
        *pd = de[c];
    }
}

// sum over the stored entries of  w (t - A_r . B_c)^2, every term in float32, one float64 partial per workgroup
template <int GL, int CH>
__global__ __launch_bounds__(256) void wmu_res_csr_kernel(WCsrView T, const float *A, const float *B, int kp, double *partials) {
    constexpr int RPW = 64 / GL;
    const int lane = threadIdx.x & 63;
    const int gl = lane % GL, gsub = lane / GL;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t row = wave * RPW + gsub;
    double acc = 0.0;
    if (row < T.rows) {
        f32x4 a[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) a[c] = *reinterpret_cast<const f32x4 *>(A + row * kp + 4 * (gl + GL * c));
        const int64_t beg = T.indptr[row], end = T.indptr[row + 1];
        for (int64_t q = beg; q < end; ++q) {
            const int32_t j = T.idx[q];
            const float t = T.tv[q], w = T.wv[q];
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const f32x4 b = *reinterpret_cast<const f32x4 *>(B + (int64_t)j * kp + 4 * (gl + GL * c));
                d += a[c][0] * b[0] + a[c][1] * b[1] + a[c][2] * b[2] + a[c][3] * b[3];
            }
            d = group_sum<GL>(d);
            const float e = t - d;
            if (gl == 0) acc += (double)(w * (e * e));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double red[4];
    if (lane == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------ P = W .* T and the update
__global__ void wmu_mul_kernel(float *P, const float *W, const float *T, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<f32x4 *>(P)[i] = reinterpret_cast<const f32x4 *>(W)[i] * reinterpret_cast<const f32x4 *>(T)[i];
}

// F <- F * num / reg(den, F), num / den = the sums of nslab slabs each in slab order;
// reg(den, F) = den + l1 + l2 F, then den == 0 -> eps   (MUSolver._regularized_delta, cmf_solvers.py:212-228)
__global__ void wmu_update_kernel(float *F, const float *num, const float *den, int nslab, int64_t stride, int64_t n4, float l1, float l2, float eps) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 f = reinterpret_cast<f32x4 *>(F)[i];
        f32x4 nu = reinterpret_cast<const f32x4 *>(num)[i];
        f32x4 de = reinterpret_cast<const f32x4 *>(den)[i];
        for (int s = 1; s < nslab; ++s) {
            nu += reinterpret_cast<const f32x4 *>(num + (int64_t)s * stride)[i];
            de += reinterpret_cast<const f32x4 *>(den + (int64_t)s * stride)[i];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float d = de[e];
            if (l1 > 0.f) d += l1;
            if (l2 > 0.f) d = d + l2 * f[e];
            if (d == 0.f) d = eps;
            f[e] = f[e] * (nu[e] / d);
        }
        reinterpret_cast<f32x4 *>(F)[i] = f;
    }
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx)
#ifdef CMF_WMU_HOST

enum { WM_NONE = 0, WM_DENSE = 1, WM_CSR = 2 }; // how the weights of a relation are held (cmf_ctx::wm_kind)

struct WmPass { int which; bool trans; int fa, fb; }; // relation X | Y (transposed), owner factor, streamed factor
static const WmPass WM_U{0, false, CMF_U, CMF_V}, WM_VX{0, true, CMF_V, CMF_U}, WM_VY{1, false, CMF_V, CMF_Z}, WM_Z{1, true, CMF_Z, CMF_V};

static float *wm_data(const cmf_ctx *c, int which) { return which == 0 ? c->X : c->Y; }

static void wm_free_side(cmf_ctx *c, int which) {
    als_bias_free(c, which);   // biases (cmf_als_bias.hip.h) go with the weights they were set on, as a background weight does
    dev_free(c, c->wm_w[which]); dev_free(c, c->wm_p[which]);
    c->wm_w[which] = c->wm_p[which] = nullptr;
    for (int t = 0; t < 2; ++t) {
        WCsrDev &M = c->wm_sp[which][t];
        dev_free(c, M.indptr); dev_free(c, M.idx); dev_free(c, M.pv); dev_free(c, M.wv); dev_free(c, M.tv); dev_free(c, M.ev);
        M = WCsrDev();
    }
    c->wm_kind[which] = WM_NONE;
    c->wm_bg[which] = 0.0;   // a background weight (cmf_als_bg.hip.h) goes with the weights it was set on
}

// kl_plan's share rule for the dense passes (option "wmu_split" forces the count); S = 1 for weights held as CSR
static void wm_plan(const cmf_ctx *c, const WmPass &ps, int64_t *S, int64_t *per) {
    if (c->wm_kind[ps.which] == WM_CSR) { *S = 1; *per = 0; return; }
    const int64_t nblk = c->frows_pad[ps.fa] / KL_RB, cblocks = c->frows_pad[ps.fb] / 256;
    int64_t s = c->opt_wmu_split > 0 ? c->opt_wmu_split : (nblk >= c->num_cu ? 1 : (c->num_cu + nblk - 1) / nblk);
    s = std::max<int64_t>(1, std::min<int64_t>(s, cblocks));
    *per = (cblocks + s - 1) / s * 256;
    *S = (c->frows_pad[ps.fb] + *per - 1) / *per;
}

// scratch of a step: numerator and denominator slabs of the widest sweep (the two passes of the V sweep share their slabs)
static int64_t wm_sweep_slabs(const cmf_ctx *c, int f) {
    int64_t S, S2 = 0, per;
    if (f == CMF_V) { wm_plan(c, WM_VX, &S, &per); wm_plan(c, WM_VY, &S2, &per); }
    else wm_plan(c, f == CMF_U ? WM_U : WM_Z, &S, &per);
    return std::max(S, S2);
}
static size_t wm_slab_bytes(const cmf_ctx *c, int mask) {
    size_t need = 0;
    const int bits[3] = {CMF_UPD_U, CMF_UPD_V, CMF_UPD_Z};
    for (int f = 0; f < 3; ++f)
        if (mask & bits[f]) need = std::max(need, (size_t)2 * wm_sweep_slabs(c, f) * c->frows_pad[f] * c->kp * sizeof(float));
    return need;
}

static int wm_check(cmf_ctx *c, const char *what) {
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: k_pad = %d (n_components above 256) is not supported by the weighted passes", what, c->kp);
    return CMF_OK;
}
// a relation can take part: weights held as CSR carry their own data; otherwise the dense image is needed
static int wm_side_ok(cmf_ctx *c, const char *what, int which) {
    if (c->wm_kind[which] == WM_CSR) return CMF_OK;
    if (!have_data(c, which)) return fail(CMF_EINVAL, "%s: %s has not been set", what, which == 0 ? "X" : "Y");
    if (!wm_data(c, which))
        return fail(CMF_EUNSUPPORTED, "%s: %s is held as native CSR without weights; an unweighted relation beside a weighted one needs its dense image "
                                      "(sparse_mode 1), or bind it through cmf_set_weighted_csr", what, which == 0 ? "X" : "Y");
    return CMF_OK;
}

template <int MODE>
static int wm_launch_dense(cmf_ctx *c, const WmPass &ps, const WmuArgs &a, dim3 grid) {
#define CMF_WMQ(KP_)                                                                                                      \
    do {                                                                                                                  \
        if (ps.trans) hipLaunchKernelGGL((wmu_pass_kernel<KP_, 1, MODE>), grid, dim3(256), 0, c->stream, a);               \
        else hipLaunchKernelGGL((wmu_pass_kernel<KP_, 0, MODE>), grid, dim3(256), 0, c->stream, a);                        \
    } while (0)
    switch (c->kp) {
    case 32: CMF_WMQ(32); break;
    case 64: CMF_WMQ(64); break;
    case 128: CMF_WMQ(128); break;
    default: CMF_WMQ(256); break;
    }
#undef CMF_WMQ
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// numerator and denominator slabs of one pass (slab stride = rows_pad * k_pad); the first `have` slabs hold the sweep's other
// pass and are added to; *nslab = how many slabs this pass touched
static int wm_pass(cmf_ctx *c, const WmPass &ps, float *num, float *den, int have, int *nslab) {
    const int64_t rows_pad = c->frows_pad[ps.fa];
    const float *A = c->F[ps.fa], *B = c->F[ps.fb];
    if (c->wm_kind[ps.which] == WM_CSR) {
        const WCsrDev &M = c->wm_sp[ps.which][ps.trans ? 1 : 0];
        WCsrView v{M.indptr, M.idx, M.pv, M.wv, M.tv, M.rows};
        Timed tm(c, CMF_K_KLMU, 6.0 * (double)M.nnz * (double)c->kp);
        const int gl = c->kp / 4, rpw = 64 / gl;
        const unsigned blocks = (unsigned)(rows_pad / (4 * rpw));
        const int add = have > 0 ? 1 : 0;
        switch (c->kp) {
        case 32: hipLaunchKernelGGL((wmu_csr_kernel<8, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, num, den, add); break;
        case 64: hipLaunchKernelGGL((wmu_csr_kernel<16, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, num, den, add); break;
        case 128: hipLaunchKernelGGL((wmu_csr_kernel<32, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, num, den, add); break;
        default: hipLaunchKernelGGL((wmu_csr_kernel<64, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, num, den, add); break;
        }
        HIPCHK(hipGetLastError());
        *nslab = 1;
        return CMF_OK;
    }
    int64_t S, per;
    wm_plan(c, ps, &S, &per);
    const bool weighted = c->wm_kind[ps.which] == WM_DENSE;
    WmuArgs a;
    memset(&a, 0, sizeof a);
    a.ldt = ps.which == 0 ? c->dp : c->pp;
    a.A = A; a.B = B;
    a.cols_pad = c->frows_pad[ps.fb];
    a.cols_per_share = per;
    a.rows_valid = c->frows[ps.fa]; a.cols_valid = c->frows[ps.fb];
    a.slab_stride = rows_pad * c->kp;
    a.acc_slabs = have;
    const dim3 grid((unsigned)(rows_pad / KL_RB), (unsigned)S);
    const double cells = (double)c->frows[ps.fa] * (double)c->frows[ps.fb];
    {
        Timed tm(c, CMF_K_KLMU, 4.0 * cells * (double)c->k);
        a.W = c->wm_w[ps.which];
        a.out = den;
        if (weighted) CHK(wm_launch_dense<WM_DEN>(c, ps, a, grid));
        else CHK(wm_launch_dense<WM_DEN1>(c, ps, a, grid));
    }
    {
        Timed tm(c, ps.trans ? CMF_K_GEMM_TN : CMF_K_GEMM_NN, 2.0 * cells * (double)c->k);
        a.W = weighted ? c->wm_p[ps.which] : wm_data(c, ps.which);
        a.out = num;
        CHK(wm_launch_dense<WM_NUM>(c, ps, a, grid));
    }
    *nslab = (int)S;
    return CMF_OK;
}

static int wm_update(cmf_ctx *c, int f, const float *num, const float *den, int nslab, double l1, double l2) {
    const int64_t n4 = c->frows_pad[f] * c->kp / 4;
    Timed tm(c, CMF_K_ELEMWISE);
    const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 4096);
    hipLaunchKernelGGL(wmu_update_kernel, dim3(blocks), dim3(256), 0, c->stream, c->F[f], num, den, nslab, c->frows_pad[f] * c->kp, n4, (float)l1, (float)l2,
                       CMF_KL_EPS);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

extern "C" int cmf_mu_weighted_step(cmf_ctx *c, double l1, double l2, int mask) {
    NEED_PROBLEM(c);
    CHK(wm_check(c, "cmf_mu_weighted_step"));
    if (mask & (CMF_UPD_U | CMF_UPD_V)) CHK(wm_side_ok(c, "cmf_mu_weighted_step", 0));
    if (mask & (CMF_UPD_Z | CMF_UPD_V)) CHK(wm_side_ok(c, "cmf_mu_weighted_step", 1));
    for (int w = 0; w < 2; ++w)
        if (c->wm_bg[w] > 0.0 && (mask & ((w == 0 ? CMF_UPD_U : CMF_UPD_Z) | CMF_UPD_V)))
            return fail(CMF_EUNSUPPORTED, "cmf_mu_weighted_step: %s has a background weight bound, which only the ALS steps honour; "
                                          "clear it with cmf_set_background_weight(ctx, %d, 0)", w == 0 ? "X" : "Y", w);
    for (int w = 0; w < 2; ++w)
        if (c->als_bias[w].on && (mask & ((w == 0 ? CMF_UPD_U : CMF_UPD_Z) | CMF_UPD_V)))
            return fail(CMF_EUNSUPPORTED, "cmf_mu_weighted_step: %s has biases bound, which only cmf_als_bias_step honours; "
                                          "clear them with cmf_set_biases(ctx, %d, 0, 0, 0)", w == 0 ? "X" : "Y", w);
    DeviceGuard dg(c->device);
    CHK(kl_ensure(c, c->wm_slab, wm_slab_bytes(c, mask)));
    float *base = (float *)c->wm_slab.p;
    const int bits[3] = {CMF_UPD_V, CMF_UPD_U, CMF_UPD_Z}, fs[3] = {CMF_V, CMF_U, CMF_Z}; // sweep order V, U, Z (cmf_solvers.py:248-263)
    for (int s = 0; s < 3; ++s) {
        if (!(mask & bits[s])) continue;
        const int f = fs[s];
        float *num = base, *den = base + wm_sweep_slabs(c, f) * c->frows_pad[f] * c->kp;
        int n1 = 0, n2 = 0;
        if (f == CMF_V) {
            CHK(wm_pass(c, WM_VX, num, den, 0, &n1));
            CHK(wm_pass(c, WM_VY, num, den, n1, &n2));
        } else
            CHK(wm_pass(c, f == CMF_U ? WM_U : WM_Z, num, den, 0, &n1));
        CHK(wm_update(c, f, num, den, std::max(n1, n2), l1, l2));
    }
    return CMF_OK;
}

// sum of w (t - s)^2 over one relation into *out
// (targets: what the CSR pass reads as t -- the adjusted targets of a biased relation for cmf_als_residual_sq; null: t itself)
static int wm_residual_side(cmf_ctx *c, int which, double *out, const float *targets = nullptr) {
    const int fa = which == 0 ? CMF_U : CMF_V, fb = which == 0 ? CMF_V : CMF_Z;
    const float *A = c->F[fa], *B = c->F[fb];
    CHK(kl_ensure(c, c->wm_small, 64));
    double *sum = (double *)c->wm_small.p;
    if (c->wm_kind[which] == WM_CSR) {
        const WCsrDev &M = c->wm_sp[which][0];
        WCsrView v{M.indptr, M.idx, M.pv, M.wv, targets ? targets : M.tv, M.rows};
        const int gl = c->kp / 4, rpw = 64 / gl;
        const unsigned blocks = (unsigned)std::max<int64_t>(1, ((M.rows + rpw - 1) / rpw + 3) / 4);
        CHK(kl_ensure(c, c->wm_part, (size_t)blocks * sizeof(double)));
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
        double *part = (double *)c->wm_part.p;
        switch (c->kp) {
        case 32: hipLaunchKernelGGL((wmu_res_csr_kernel<8, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, part); break;
        case 64: hipLaunchKernelGGL((wmu_res_csr_kernel<16, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, part); break;
        case 128: hipLaunchKernelGGL((wmu_res_csr_kernel<32, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, part); break;
        default: hipLaunchKernelGGL((wmu_res_csr_kernel<64, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, part); break;
        }
        hipLaunchKernelGGL(sum_doubles_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)part, (int64_t)blocks, sum);
        HIPCHK(hipGetLastError());
    } else {
        const WmPass ps = which == 0 ? WM_U : WM_VY;
        int64_t S, per;
        wm_plan(c, ps, &S, &per);
        const int64_t rows_pad = c->frows_pad[fa];
        const dim3 grid((unsigned)(rows_pad / KL_RB), (unsigned)S);
        const int64_t nparts = (int64_t)grid.x * grid.y;
        CHK(kl_ensure(c, c->wm_part, (size_t)nparts * sizeof(double)));
        WmuArgs a;
        memset(&a, 0, sizeof a);
        a.W = c->wm_w[which];
        a.T = wm_data(c, which);
        a.ldt = which == 0 ? c->dp : c->pp;
        a.A = A; a.B = B;
        a.cols_pad = c->frows_pad[fb];
        a.cols_per_share = per;
        a.rows_valid = c->frows[fa]; a.cols_valid = c->frows[fb];
        a.part = (double *)c->wm_part.p;
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)c->frows[fa] * (double)c->frows[fb] * (double)c->k);
#define CMF_WMR(KP_)                                                                                                         \
    do {                                                                                                                     \
        if (c->wm_kind[which] == WM_DENSE) hipLaunchKernelGGL((wmu_res_kernel<KP_, WM_RES>), grid, dim3(256), 0, c->stream, a); \
        else hipLaunchKernelGGL((wmu_res_kernel<KP_, WM_RES1>), grid, dim3(256), 0, c->stream, a);                            \
    } while (0)
        switch (c->kp) {
        case 32: CMF_WMR(32); break;
        case 64: CMF_WMR(64); break;
        case 128: CMF_WMR(128); break;
        default: CMF_WMR(256); break;
        }
#undef CMF_WMR
        hipLaunchKernelGGL(sum_doubles_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)a.part, nparts, sum);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_weighted_residual_sq(cmf_ctx *c, double *ex, double *ey) {
    NEED_PROBLEM(c);
    CHK(wm_check(c, "cmf_weighted_residual_sq"));
    if (ex) CHK(wm_side_ok(c, "cmf_weighted_residual_sq", 0));
    if (ey) CHK(wm_side_ok(c, "cmf_weighted_residual_sq", 1));
    DeviceGuard dg(c->device);
    if (ex) CHK(wm_residual_side(c, 0, ex));
    if (ey) CHK(wm_residual_side(c, 1, ey));
    return CMF_OK;
}

extern "C" int cmf_mu_weighted_layout(cmf_ctx *c, int64_t *out4) {
    NEED_PROBLEM(c);
    if (!out4) return fail(CMF_EINVAL, "cmf_mu_weighted_layout: null output");
    CHK(wm_check(c, "cmf_mu_weighted_layout"));
    out4[0] = wm_sweep_slabs(c, CMF_U);
    out4[1] = wm_sweep_slabs(c, CMF_V);
    out4[2] = wm_sweep_slabs(c, CMF_Z);
    out4[3] = (int64_t)(wm_slab_bytes(c, CMF_UPD_U | CMF_UPD_V | CMF_UPD_Z) + 64);
    return CMF_OK;
}

// P = W .* T behind a (re)written dense W image
static int wm_form_p(cmf_ctx *c, int which, int64_t rp, int64_t cp) {
    if (!c->wm_p[which]) CHK(dev_alloc(c, (void **)&c->wm_p[which], (size_t)rp * cp * sizeof(float), false));
    const int64_t n4 = rp * cp / 4;
    Timed tm(c, CMF_K_ELEMWISE);
    const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 8192);
    hipLaunchKernelGGL(wmu_mul_kernel, dim3(blocks), dim3(256), 0, c->stream, c->wm_p[which], (const float *)c->wm_w[which], (const float *)wm_data(c, which), n4);
    HIPCHK(hipGetLastError());
    c->wm_kind[which] = WM_DENSE;
    return CMF_OK;
}
// the relation's dense image must exist; a zeroed W image of its padded shape
static int wm_dense_begin(cmf_ctx *c, const char *what, int which, int64_t *r, int64_t *cc, int64_t *rp, int64_t *cp) {
    float **slot;
    CHK(data_dims(c, which, r, cc, rp, cp, &slot));
    if (!*slot) return fail(CMF_EINVAL, "%s: dense weights need the dense image of %s: set the data first (a native CSR relation takes cmf_set_weighted_csr)",
                            what, which == 0 ? "X" : "Y");
    HIPCHK(hipStreamSynchronize(c->stream));
    wm_free_side(c, which);
    CHK(dev_alloc(c, (void **)&c->wm_w[which], (size_t)*rp * *cp * sizeof(float)));
    return CMF_OK;
}

template <typename T>
static int wm_set_weight(cmf_ctx *c, int which, const T *ptr, int64_t rs, int64_t cs) {
    NEED_PROBLEM(c);
    if (!ptr) return fail(CMF_EINVAL, "null weight pointer");
    DeviceGuard dg(c->device);
    int64_t r, cc, rp, cp;
    CHK(wm_dense_begin(c, "cmf_set_weight", which, &r, &cc, &rp, &cp));
    CHK(upload_strided<T>(c, c->wm_w[which], cp, r, cc, ptr, rs, cs));
    return wm_form_p(c, which, rp, cp);
}
extern "C" int cmf_set_weight_f64(cmf_ctx *c, int which, const double *ptr, int64_t rs, int64_t cs) { return wm_set_weight<double>(c, which, ptr, rs, cs); }
extern "C" int cmf_set_weight_f32(cmf_ctx *c, int which, const float *ptr, int64_t rs, int64_t cs) { return wm_set_weight<float>(c, which, ptr, rs, cs); }

extern "C" int cmf_fill_weight_synthetic(cmf_ctx *c, int which, uint64_t seed, double density) {
    NEED_PROBLEM(c);
    if (!(density >= 0.0 && density <= 1.0)) return fail(CMF_EINVAL, "cmf_fill_weight_synthetic: density must lie in [0, 1]");
    DeviceGuard dg(c->device);
    int64_t r, cc, rp, cp;
    CHK(wm_dense_begin(c, "cmf_fill_weight_synthetic", which, &r, &cc, &rp, &cp));
    CHK(launch_fill(c, c->wm_w[which], cp, r, cc, seed, 0, 0, (float)density, 2));
    return wm_form_p(c, which, rp, cp);
}

extern "C" int cmf_get_weight_block_f32(cmf_ctx *c, int which, int64_t row0, int64_t nrows, int64_t col0, int64_t ncols, float *dst) {
    NEED_PROBLEM(c);
    DeviceGuard dg(c->device);
    int64_t r, cc, rp, cp; float **slot;
    CHK(data_dims(c, which, &r, &cc, &rp, &cp, &slot));
    if (!dst || row0 < 0 || col0 < 0 || nrows < 0 || ncols < 0 || row0 + nrows > r || col0 + ncols > cc) return fail(CMF_EINVAL, "block out of range");
    if (c->wm_kind[which] != WM_DENSE) return fail(CMF_EINVAL, "%s has no dense weight image", which == 0 ? "X" : "Y");
    if (nrows == 0 || ncols == 0) return CMF_OK;
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)ncols * sizeof(float), c->wm_w[which] + row0 * cp + col0, (size_t)cp * sizeof(float), (size_t)ncols * sizeof(float),
                            (size_t)nrows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_clear_weight(cmf_ctx *c, int which) {
    NEED_PROBLEM(c);
    if (which != 0 && which != 1) return fail(CMF_EINVAL, "which must be 0 (X) or 1 (Y)");
    DeviceGuard dg(c->device);
    HIPCHK(hipStreamSynchronize(c->stream));
    wm_free_side(c, which);
    return CMF_OK;
}

static int wm_csr_upload(cmf_ctx *c, WCsrDev &dst, const std::vector<int64_t> &indptr, const std::vector<int32_t> &idx, const std::vector<float> &p,
                         const std::vector<float> &w, const std::vector<float> *t, int64_t rows, int64_t cols) {
    const int64_t nnz = (int64_t)idx.size();
    dst.rows = rows; dst.cols = cols; dst.nnz = nnz;
    auto up = [&](void **dptr, const void *src, size_t bytes) -> int {
        CHK(dev_alloc(c, dptr, std::max<size_t>(bytes, 16), false));
        if (bytes) HIPCHK(hipMemcpyAsync(*dptr, src, bytes, hipMemcpyHostToDevice, c->stream));
        return CMF_OK;
    };
    CHK(up((void **)&dst.indptr, indptr.data(), (size_t)(rows + 1) * sizeof(int64_t)));
    CHK(up((void **)&dst.idx, idx.data(), (size_t)nnz * sizeof(int32_t)));
    CHK(up((void **)&dst.pv, p.data(), (size_t)nnz * sizeof(float)));
    CHK(up((void **)&dst.wv, w.data(), (size_t)nnz * sizeof(float)));
    if (t) CHK(up((void **)&dst.tv, t->data(), (size_t)nnz * sizeof(float)));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vectors may go
    return CMF_OK;
}

extern "C" int cmf_set_weighted_csr(cmf_ctx *c, int which, const int64_t *indptr, const int32_t *indices, const double *t_values, const double *w_values) {
    NEED_PROBLEM(c);
    DeviceGuard dg(c->device);
    int64_t r, cc, rp, cp; float **slot;
    CHK(data_dims(c, which, &r, &cc, &rp, &cp, &slot));
    if (!indptr) return fail(CMF_EINVAL, "null CSR pointer");
    if (indptr[0] != 0) return fail(CMF_EINVAL, "CSR indptr[0] must be 0");
    for (int64_t i = 0; i < r; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(CMF_EINVAL, "CSR indptr is not monotonic at row %lld", (long long)i);
    const int64_t nnz = indptr[r];
    if (nnz > 0 && (!indices || !t_values || !w_values)) return fail(CMF_EINVAL, "null CSR pointer");
    for (int64_t q = 0; q < nnz; ++q) {
        if (indices[q] < 0 || indices[q] >= cc) return fail(CMF_EINVAL, "CSR column index out of range");
        if (!(w_values[q] >= 0.0) || !std::isfinite(w_values[q])) return fail(CMF_EINVAL, "weights must be finite and non-negative");
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    wm_free_side(c, which);
    std::vector<int64_t> ip(indptr, indptr + r + 1), ipt((size_t)cc + 1, 0);
    std::vector<int32_t> ix(indices, indices + nnz), ixt((size_t)nnz);
    std::vector<float> t((size_t)nnz), w((size_t)nnz), p((size_t)nnz), pt((size_t)nnz), wt((size_t)nnz);
    for (int64_t q = 0; q < nnz; ++q) {
        t[q] = (float)t_values[q];
        w[q] = (float)w_values[q];
        p[q] = w[q] * t[q];
    }
    // the transposed image: counting sort by column, rows ascending inside a column (stored order of the transpose)
    for (int64_t q = 0; q < nnz; ++q) ipt[(size_t)ix[q] + 1]++;
    for (int64_t j = 0; j < cc; ++j) ipt[(size_t)j + 1] += ipt[(size_t)j];
    {
        std::vector<int64_t> pos(ipt.begin(), ipt.end() - 1);
        for (int64_t i = 0; i < r; ++i)
            for (int64_t q = ip[i]; q < ip[i + 1]; ++q) {
                const int64_t o = pos[(size_t)ix[q]]++;
                ixt[o] = (int32_t)i; pt[o] = p[q]; wt[o] = w[q];
            }
    }
    CHK(wm_csr_upload(c, c->wm_sp[which][0], ip, ix, p, w, &t, r, cc));
    CHK(wm_csr_upload(c, c->wm_sp[which][1], ipt, ixt, pt, wt, nullptr, cc, r));
    c->wm_kind[which] = WM_CSR;
    return CMF_OK;
}
#endif // CMF_WMU_HOST
