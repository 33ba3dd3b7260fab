// cmf_klmu.hip.h -- multiplicative updates for the generalised Kullback-Leibler objective  D(X || U V^T) + D(Y || V Z^T).
//
// The KL update of a factor needs  N = (T ./ max(A B^T, EPS)) B : an element-wise quotient BETWEEN two products over the same tiles
// (sklearn's _multiplicative_update_w / _h with beta_loss = 1, applied to each block of the collective model).  The quotient tile
// is never written to memory:
//
// kl_quotient_kernel<KP, TRANS>: one 256-thread workgroup (4 waves, one per SIMD) owns KL_RB = 128 output rows -- wave w the rows
// 32 w .. 32 w + 31 of A, resident in KP / 2 registers per lane as in topk_scan_kernel -- and one share of the streamed rows of B,
// which pass through LDS in tiles of 8192 / KP rows (32 KB, register-staged: the loads of tile t + 1 travel under the MFMAs of
// tile t).  For each 32 x 32 sub-tile:
//   1. S^T = B_tile A_blk^T on v_mfma_f32_32x32x2_f32 with the STREAMED rows as the A operand and the owned rows as the B operand:
//      lane l holds 16 entries of ONE output row (l & 31); register r of lane half h = l >> 5 is streamed index
//      8 (r >> 2) + 4 h + (r & 3) of the 32.
//   2. the 16 registers become quotients in place, q = t * rcp(max(s, EPS)), against the matching elements of T (read as stored,
//      TRANS = 0: T[row][streamed], or transposed, TRANS = 1: T[streamed][row]).  A zero of T gives an exact zero.
//   3. N^T += B_tile^T Q^T: register r goes straight back as the B operand of the second product (k = lane half), and the A
//      operand is read from the SAME LDS tile at the row register r stands for in that lane half -- the pairing of step 1.  The
//      k_pad columns are dealt to the MFMA rows so that a lane reads W = min(4, KP / 32) consecutive floats per LDS access:
//      accumulator kb = jj W + e, MFMA row i holds column W (i + 32 jj) + e.
// Every output element is ONE fma chain in an order fixed by this file, the share it belongs to and nothing else; the shares of
// an output block (few output rows, long stream) leave partial slabs that the update kernel sums in slab order.  No atomics.
// Padding: rows and columns of T, A and B beyond the valid extent are zero, so they contribute exact zeros (0 * rcp(EPS)).
//
// kl_div_kernel<KP>: step 1 of the same structure, then  t log(t / s) - t + s  (t = 0: s; s = 0: EPS in the quotient) over the valid rows and columns,
// per-lane float64 sums, one float64 partial per workgroup (summed by sum_doubles_kernel).
// kl_quotient_csr_kernel<GL, CH> / kl_div_csr_kernel<GL, CH>: the same for a native CSR T -- a group of GL lanes owns an output
// row and uses the gathered row of B twice per stored entry: for the dot with its own row (DPP group_sum) and for the update.
// kl_colsum_*: column sums of a factor in a fixed order (partials per row chunk, then one pass over the partials).
// kl_update_kernel: F <- F * (sum of the numerator slabs) / reg(colsum, F)   (cmf_solvers.py:212-228 with gamma = 1).
//
// No existing kernel is touched.  Reference counterpart: none -- pycmf/cmf.py:245-247 documents beta_loss='kullback-leibler' and
// states that it is not implemented.
#pragma once
#include "cmf_kernels.hip.h"
#include "cmf_sparse.hip.h"

namespace cmfk {

enum { KL_RB = 128, KL_TILE_FLOATS = 8192 };
#define CMF_KL_EPS 1.1920928955078125e-07f // 2^-23: the reference's EPSILON

struct KlArgs {
    const float *T;          // dense image of X or Y
    int64_t ldt;
    const float *A;          // the factor that owns the output rows, pitch KP
    const float *B;          // the streamed factor, pitch KP
    int64_t cols_pad;        // streamed extent (multiple of 256)
    int64_t cols_per_share;  // multiple of 256
    int64_t rows_valid, cols_valid; // divergence only
    float *out;              // [share][rows_pad][KP]
    int64_t slab_stride;
    double *part;            // divergence: one partial per workgroup
};

template <int KP, int TRANS, int DIV>
__device__ __forceinline__ void kl_pass_body(const KlArgs &g, f32x4 *tile) {
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
    f32x4 af[NCH];
    {
        const f32x4 *src = (const f32x4 *)(g.A + row * KP);
#pragma unroll
        for (int c = 0; c < NCH; ++c) af[c] = src[2 * c + h];
    }
    const int64_t c_begin = (int64_t)blockIdx.y * g.cols_per_share;
    const int64_t c_end = min(c_begin + g.cols_per_share, g.cols_pad);
    const int ntiles = c_end > c_begin ? (int)((c_end - c_begin) / CT) : 0;

    f32x16 nacc[DIV ? 1 : KB];
#pragma unroll
    for (int kb = 0; kb < (DIV ? 1 : KB); ++kb) nacc[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double dsum = 0.0;

    // staging: float4 number i * 256 + tid of the tile (8 per thread)
    f32x4 st[8];
    auto fetch = [&](int t) {
        const f32x4 *src = (const f32x4 *)(g.B + (c_begin + (int64_t)t * CT) * KP);
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = src[i * 256 + tid];
    };
    // the 16 elements of T that face the accumulator registers of a sub-tile starting at streamed index cb
    f32x4 tv[4], tn[4];
    auto fetch_t = [&](f32x4 *dst, int64_t cb) {
        if constexpr (TRANS == 0) {
            const float *src = g.T + row * g.ldt + cb + 4 * h;
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q] = *(const f32x4 *)(src + 8 * q);
        } else {
            const float *src = g.T + (cb + 4 * h) * g.ldt + row;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) dst[q][j] = src[(int64_t)(8 * q + j) * g.ldt];
        }
    };
    if (ntiles > 0) {
        fetch(0);
        fetch_t(tv, c_begin);
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
            if (more) fetch_t(tn, cb + 32);
            const int trow = sub * 32 + li;
            const f32x4 *arow = tile + trow * SLOTS;
            const int sw = trow & SW;
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const f32x4 a = arow[(2 * c + h) ^ sw];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], af[c][0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], af[c][1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], af[c][2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], af[c][3], acc, 0, 0, 0);
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0); // fragment reads at most four pieces ahead: the owned rows need the registers
            }
            // register r of the lane: streamed row (r & 3) + 8 (r >> 2) + 4 h of the 32, output row lane & 31
            if constexpr (DIV) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float tt = tv[r >> 2][r & 3];
                    const float s = acc[r];
                    const int64_t col = cb + 8 * (r >> 2) + 4 * h + (r & 3);
                    if (row < g.rows_valid && col < g.cols_valid) {
                        double e = (double)s;
                        if (tt > 0.f) e += (double)(tt * logf(tt / (s > 0.f ? s : CMF_KL_EPS))) - (double)tt; // s = 0: EPS, as sklearn's _beta_divergence
                        dsum += e;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = tv[r >> 2][r & 3] * __builtin_amdgcn_rcpf(fmaxf(acc[r], CMF_KL_EPS));
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
                for (int q = 0; q < 4; ++q) tv[q] = tn[q];
            }
        }
    }

    if constexpr (DIV) {
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
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
            for (int r2 = 0; r2 < 16; ++r2) {
                const int i = (r2 & 3) + 8 * (r2 >> 2) + 4 * h;
                float *p = dst + W * (i + 32 * jj);
                if constexpr (W == 4) *(f32x4 *)p = f32x4{nacc[jj * 4][r2], nacc[jj * 4 + 1][r2], nacc[jj * 4 + 2][r2], nacc[jj * 4 + 3][r2]};
                else if constexpr (W == 2) *(f32x2 *)p = f32x2{nacc[0][r2], nacc[1][r2]};
                else *p = nacc[0][r2];
            }
    }
}

template <int KP, int TRANS>
__global__ __launch_bounds__(256, KP >= 128 ? 1 : 2) void kl_quotient_kernel(KlArgs g) {
    __shared__ __attribute__((aligned(16))) f32x4 kl_tile[KL_TILE_FLOATS / 4];
    kl_pass_body<KP, TRANS, 0>(g, kl_tile);
}
template <int KP>
__global__ __launch_bounds__(256, KP == 256 ? 1 : 2) void kl_div_kernel(KlArgs g) {
    __shared__ __attribute__((aligned(16))) f32x4 kl_tile[KL_TILE_FLOATS / 4];
    kl_pass_body<KP, 0, 1>(g, kl_tile);
}

// ------------------------------------------------------------------ native CSR
// out[r, :] = sum over the stored (r, c, t) of  t / max(A_r . B_c, EPS)  B_c ; rows beyond T.rows (padding) are written as zeros.
// GL = lanes per row group = KP / 4 (CH = 1 for every supported width; the parameter mirrors spmm_csr_kernel)
template <int GL, int CH>
__global__ __launch_bounds__(256) void kl_quotient_csr_kernel(CsrView T, const float *A, const float *B, int kp, int64_t rows_pad, float *out) {
    constexpr int RPW = 64 / GL;
    const int lane = threadIdx.x & 63;
    const int gl = lane % GL, gsub = lane / GL;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t row = wave * RPW + gsub;
    if (row >= rows_pad) return;
    f32x4 acc[CH], a[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < T.rows) {
#pragma unroll
        for (int c = 0; c < CH; ++c) a[c] = *reinterpret_cast<const f32x4 *>(A + row * kp + 4 * (gl + GL * c));
        const int64_t beg = T.indptr[row], end = T.indptr[row + 1];
        int64_t q = beg;
        for (; q + 2 <= end; q += 2) { // two independent gathers in flight; the entries still enter the sum in stored order
            const int32_t j0 = T.idx[q], j1 = T.idx[q + 1];
            const float v0 = T.val[q], v1 = T.val[q + 1];
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
            d0 = group_sum<GL>(d0);
            d1 = group_sum<GL>(d1);
            const float w0 = v0 * __builtin_amdgcn_rcpf(fmaxf(d0, CMF_KL_EPS));
            const float w1 = v1 * __builtin_amdgcn_rcpf(fmaxf(d1, CMF_KL_EPS));
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                acc[c] += w0 * b0[c];
                acc[c] += w1 * b1[c];
            }
        }
        if (q < end) {
            const int32_t j0 = T.idx[q];
            const float v0 = T.val[q];
            f32x4 b0[CH];
            float d0 = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                b0[c] = *reinterpret_cast<const f32x4 *>(B + (int64_t)j0 * kp + 4 * (gl + GL * c));
                d0 += a[c][0] * b0[c][0] + a[c][1] * b0[c][1] + a[c][2] * b0[c][2] + a[c][3] * b0[c][3];
            }
            d0 = group_sum<GL>(d0);
            const float w0 = v0 * __builtin_amdgcn_rcpf(fmaxf(d0, CMF_KL_EPS));
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c] += w0 * b0[c];
        }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) *reinterpret_cast<f32x4 *>(out + row * kp + 4 * (gl + GL * c)) = acc[c];
}

// sum over the stored entries of  t log(t / (A_r . B_c)) - t  (t > 0; a zero product counts as EPS), one float64 partial per workgroup
template <int GL, int CH>
__global__ __launch_bounds__(256) void kl_div_csr_kernel(CsrView T, const float *A, const float *B, int kp, double *partials) {
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
            const float v = T.val[q];
            float d = 0.f;
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                const f32x4 b = *reinterpret_cast<const f32x4 *>(B + (int64_t)j * kp + 4 * (gl + GL * c));
                d += a[c][0] * b[0] + a[c][1] * b[1] + a[c][2] * b[2] + a[c][3] * b[3];
            }
            d = group_sum<GL>(d);
            if (gl == 0 && v > 0.f) acc += (double)(v * logf(v / (d > 0.f ? d : CMF_KL_EPS))) - (double)v;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double red[4];
    if (lane == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------ column sums and the update
// part[b][col] = sum of F[r][col] over the rows of chunk b: thread (sub, col) walks every (256 / kp)-th row, the subs are added in order
template <typename ACC>
__global__ __launch_bounds__(256) void kl_colsum_partial_kernel(const float *F, int kp, int64_t rows, int64_t chunk, ACC *part) {
    __shared__ ACC red[256];
    const int tid = threadIdx.x, col = tid % kp, sub = tid / kp, nsub = 256 / kp;
    const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = min(rows, r0 + chunk);
    ACC s = 0;
    for (int64_t r = r0 + sub; r < r1; r += nsub) s += (ACC)F[r * kp + col];
    red[tid] = s;
    __syncthreads();
    if (tid < kp) {
        ACC t = 0;
        for (int u = 0; u < nsub; ++u) t += red[u * kp + tid];
        part[(int64_t)blockIdx.x * kp + tid] = t;
    }
}
template <typename ACC>
__global__ __launch_bounds__(256) void kl_colsum_reduce_kernel(const ACC *part, int kp, int nblk, ACC *out) {
    const int col = threadIdx.x;
    if (col >= kp) return;
    ACC s = 0;
    for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * kp + col];
    out[col] = s;
}

// F <- F * num / reg(colsum, F), num = the sum of the nslab numerator slabs in slab order;
// reg(den, F) = den + l1 + l2 F, then den == 0 -> eps   (MUSolver._regularized_delta, cmf_solvers.py:212-228)
__global__ void kl_update_kernel(float *F, const float *slabs, int nslab, int64_t stride, const float *colsum, int kp, int64_t n4,
                                 float l1, float l2, float eps) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 f = reinterpret_cast<f32x4 *>(F)[i];
        f32x4 nu = reinterpret_cast<const f32x4 *>(slabs)[i];
        for (int s = 1; s < nslab; ++s) nu += reinterpret_cast<const f32x4 *>(slabs + (int64_t)s * stride)[i];
        const f32x4 de = *reinterpret_cast<const f32x4 *>(colsum + (4 * i) % kp);
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
#ifdef CMF_KLMU_HOST

// grow-only buffer of this file's own: unlike ensure() it leaves the captured graphs of the Frobenius steps alone (nothing of
// theirs points into it)
static int kl_ensure(cmf_ctx *c, DevBuf &b, size_t bytes) {
    if (b.bytes >= bytes) return CMF_OK;
    if (b.p) {
        HIPCHK(hipStreamSynchronize(c->stream));
        dev_free(c, b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    CHK(dev_alloc(c, &b.p, bytes, false));
    b.bytes = bytes;
    return CMF_OK;
}

struct KlPass { int which; bool trans; int fa, fb; }; // T = X | Y (transposed), owner factor, streamed factor
static const KlPass KL_U{0, false, CMF_U, CMF_V}, KL_VX{0, true, CMF_V, CMF_U}, KL_VY{1, false, CMF_V, CMF_Z}, KL_Z{1, true, CMF_Z, CMF_V};

static bool kl_native(const cmf_ctx *c, int which) { return c->sparse[which] && !(which == 0 ? c->X : c->Y); }

// Share rule of the dense pass: a sweep with fewer 128-row blocks than CUs cuts the stream into as many shares as bring the
// grid up to one workgroup per CU (at most one share per 256 streamed rows); option "kl_split" forces the count.  S = 1 for CSR.
static void kl_plan(const cmf_ctx *c, const KlPass &ps, int64_t *S, int64_t *per) {
    if (kl_native(c, ps.which)) { *S = 1; *per = 0; return; }
    const int64_t nblk = c->frows_pad[ps.fa] / KL_RB, cblocks = c->frows_pad[ps.fb] / 256;
    int64_t s = c->opt_kl_split > 0 ? c->opt_kl_split : (nblk >= c->num_cu ? 1 : (c->num_cu + nblk - 1) / nblk);
    s = std::max<int64_t>(1, std::min<int64_t>(s, cblocks));
    *per = (cblocks + s - 1) / s * 256;
    *S = (c->frows_pad[ps.fb] + *per - 1) / *per;
}

static int64_t kl_colsum_blocks(int64_t rows) { return (rows + 511) / 512; }

// scratch of a step: the numerator slabs of the widest sweep + column-sum partials and sums
static size_t kl_small_bytes(const cmf_ctx *c) {
    const int64_t rmax = std::max(c->mp + c->pp, c->dp);
    return (size_t)(2 * kl_colsum_blocks(rmax) + 4) * c->kp * sizeof(double) + 64;
}
static size_t kl_slab_bytes(const cmf_ctx *c, int mask) {
    int64_t S, per, S2;
    size_t need = 0;
    const size_t kp4 = (size_t)c->kp * sizeof(float);
    if (mask & CMF_UPD_V) { kl_plan(c, KL_VX, &S, &per); kl_plan(c, KL_VY, &S2, &per); need = std::max(need, (size_t)(S + S2) * c->dp * kp4); }
    if (mask & CMF_UPD_U) { kl_plan(c, KL_U, &S, &per); need = std::max(need, (size_t)S * c->mp * kp4); }
    if (mask & CMF_UPD_Z) { kl_plan(c, KL_Z, &S, &per); need = std::max(need, (size_t)S * c->pp * kp4); }
    return need;
}

static int kl_check(cmf_ctx *c, const char *what) {
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: k_pad = %d (n_components above 256) is not supported by the Kullback-Leibler passes", what, c->kp);
    return CMF_OK;
}

// numerator slabs of one pass into `slabs` (slab stride = rows_pad * k_pad); *nslab = how many it wrote
static int kl_quotient_pass(cmf_ctx *c, const KlPass &ps, float *slabs, int *nslab) {
    if (!have_data(c, ps.which)) return fail(CMF_EINVAL, "cmf_mu_kl_step: %s has not been set", ps.which == 0 ? "X" : "Y");
    const int64_t rows_pad = c->frows_pad[ps.fa];
    const float *A = c->F[ps.fa], *B = c->F[ps.fb];
    if (kl_native(c, ps.which)) {
        const CsrDev &M = c->sp[ps.which][ps.trans ? 1 : 0];
        CsrView v{M.indptr, M.idx, M.val, M.rows};
        Timed tm(c, CMF_K_KLMU, 4.0 * (double)M.nnz * (double)c->kp);
        const int gl = c->kp / 4, rpw = 64 / gl;
        const unsigned blocks = (unsigned)(rows_pad / (4 * rpw));
        switch (c->kp) {
        case 32: hipLaunchKernelGGL((kl_quotient_csr_kernel<8, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, slabs); break;
        case 64: hipLaunchKernelGGL((kl_quotient_csr_kernel<16, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, slabs); break;
        case 128: hipLaunchKernelGGL((kl_quotient_csr_kernel<32, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, slabs); break;
        default: hipLaunchKernelGGL((kl_quotient_csr_kernel<64, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, rows_pad, slabs); break;
        }
        HIPCHK(hipGetLastError());
        *nslab = 1;
        return CMF_OK;
    }
    int64_t S, per;
    kl_plan(c, ps, &S, &per);
    KlArgs a;
    a.T = ps.which == 0 ? c->X : c->Y;
    a.ldt = ps.which == 0 ? c->dp : c->pp;
    a.A = A; a.B = B;
    a.cols_pad = c->frows_pad[ps.fb];
    a.cols_per_share = per;
    a.rows_valid = c->frows[ps.fa]; a.cols_valid = c->frows[ps.fb];
    a.out = slabs; a.slab_stride = rows_pad * c->kp;
    a.part = nullptr;
    Timed tm(c, CMF_K_KLMU, 4.0 * (double)c->frows[ps.fa] * (double)c->frows[ps.fb] * (double)c->k);
    const dim3 grid((unsigned)(rows_pad / KL_RB), (unsigned)S);
#define CMF_KLQ(KP_)                                                                                              \
    do {                                                                                                          \
        if (ps.trans) hipLaunchKernelGGL((kl_quotient_kernel<KP_, 1>), grid, dim3(256), 0, c->stream, a);          \
        else hipLaunchKernelGGL((kl_quotient_kernel<KP_, 0>), grid, dim3(256), 0, c->stream, a);                   \
    } while (0)
    switch (c->kp) {
    case 32: CMF_KLQ(32); break;
    case 64: CMF_KLQ(64); break;
    case 128: CMF_KLQ(128); break;
    default: CMF_KLQ(256); break;
    }
#undef CMF_KLQ
    HIPCHK(hipGetLastError());
    *nslab = (int)S;
    return CMF_OK;
}

// out[k_pad] = column sums of F (rows x k_pad); `part` holds the partials
template <typename ACC>
static int kl_colsum(cmf_ctx *c, const float *F, int64_t rows, ACC *part, ACC *out) {
    const int64_t nblk = kl_colsum_blocks(rows);
    Timed tm(c, CMF_K_ELEMWISE);
    hipLaunchKernelGGL((kl_colsum_partial_kernel<ACC>), dim3((unsigned)nblk), dim3(256), 0, c->stream, F, c->kp, rows, (int64_t)512, part);
    hipLaunchKernelGGL((kl_colsum_reduce_kernel<ACC>), dim3(1), dim3(256), 0, c->stream, (const ACC *)part, c->kp, (int)nblk, out);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

static int kl_update(cmf_ctx *c, int f, const float *slabs, int nslab, const float *colsum, double l1, double l2) {
    const int64_t n4 = c->frows_pad[f] * c->kp / 4;
    Timed tm(c, CMF_K_ELEMWISE);
    const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 4096);
    hipLaunchKernelGGL(kl_update_kernel, dim3(blocks), dim3(256), 0, c->stream, c->F[f], slabs, nslab, c->frows_pad[f] * c->kp, colsum, c->kp, n4,
                       (float)l1, (float)l2, CMF_KL_EPS);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

extern "C" int cmf_mu_kl_step(cmf_ctx *c, double l1, double l2, int mask) {
    NEED_PROBLEM(c);
    CHK(kl_check(c, "cmf_mu_kl_step"));
    if ((mask & (CMF_UPD_U | CMF_UPD_V)) && !have_data(c, 0)) return fail(CMF_EINVAL, "cmf_mu_kl_step: X has not been set");
    if ((mask & (CMF_UPD_Z | CMF_UPD_V)) && !have_data(c, 1)) return fail(CMF_EINVAL, "cmf_mu_kl_step: Y has not been set");
    DeviceGuard dg(c->device);
    CHK(kl_ensure(c, c->kl_slab, kl_slab_bytes(c, mask)));
    CHK(kl_ensure(c, c->kl_small, kl_small_bytes(c)));
    float *slabs = (float *)c->kl_slab.p;
    float *cs = (float *)c->kl_small.p, *cpart = cs + c->kp;
    int n1 = 0, n2 = 0;
    if (mask & CMF_UPD_V) { // V <- V .* [Q(X,U,V)^T U + Q(Y,V,Z) Z] ./ reg(colsum U + colsum Z, V): U and Z are one stacked block
        CHK(kl_quotient_pass(c, KL_VX, slabs, &n1));
        CHK(kl_quotient_pass(c, KL_VY, slabs + (int64_t)n1 * c->dp * c->kp, &n2));
        CHK(kl_colsum<float>(c, c->F[CMF_U], c->mp + c->pp, cpart, cs));
        CHK(kl_update(c, CMF_V, slabs, n1 + n2, cs, l1, l2));
    }
    if (mask & (CMF_UPD_U | CMF_UPD_Z)) CHK(kl_colsum<float>(c, c->F[CMF_V], c->dp, cpart, cs));
    if (mask & CMF_UPD_U) {
        CHK(kl_quotient_pass(c, KL_U, slabs, &n1));
        CHK(kl_update(c, CMF_U, slabs, n1, cs, l1, l2));
    }
    if (mask & CMF_UPD_Z) {
        CHK(kl_quotient_pass(c, KL_Z, slabs, &n1));
        CHK(kl_update(c, CMF_Z, slabs, n1, cs, l1, l2));
    }
    return CMF_OK;
}

// D(T || A B^T) of one side into *out
static int kl_divergence_side(cmf_ctx *c, int which, double *out) {
    const int fa = which == 0 ? CMF_U : CMF_V, fb = which == 0 ? CMF_V : CMF_Z;
    const float *A = c->F[fa], *B = c->F[fb];
    double *small = (double *)c->kl_small.p; // [0] the sum, [1 .. 1 + 2 k_pad) column sums, then partials
    if (kl_native(c, which)) { // sum over the stored entries + sum of all s = colsum(A) . colsum(B): no dense image
        const CsrDev &M = c->sp[which][0];
        CsrView v{M.indptr, M.idx, M.val, M.rows};
        const int gl = c->kp / 4, rpw = 64 / gl;
        const unsigned blocks = (unsigned)std::max<int64_t>(1, ((M.rows + rpw - 1) / rpw + 3) / 4);
        CHK(kl_ensure(c, c->kl_part, (size_t)blocks * sizeof(double)));
        {
            Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
            double *part = (double *)c->kl_part.p;
            switch (c->kp) {
            case 32: hipLaunchKernelGGL((kl_div_csr_kernel<8, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, part); break;
            case 64: hipLaunchKernelGGL((kl_div_csr_kernel<16, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, part); break;
            case 128: hipLaunchKernelGGL((kl_div_csr_kernel<32, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, part); break;
            default: hipLaunchKernelGGL((kl_div_csr_kernel<64, 1>), dim3(blocks), dim3(256), 0, c->stream, v, A, B, c->kp, part); break;
            }
            hipLaunchKernelGGL(sum_doubles_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)part, (int64_t)blocks, small);
            HIPCHK(hipGetLastError());
        }
        double *cpart = small + 1 + 2 * c->kp;
        CHK(kl_colsum<double>(c, A, c->frows_pad[fa], cpart, small + 1));
        CHK(kl_colsum<double>(c, B, c->frows_pad[fb], cpart, small + 1 + c->kp));
        std::vector<double> h(1 + 2 * (size_t)c->kp);
        HIPCHK(hipMemcpyAsync(h.data(), small, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        double d = h[0];
        for (int t = 0; t < c->kp; ++t) d += h[1 + t] * h[1 + c->kp + t];
        *out = d;
        return CMF_OK;
    }
    const KlPass ps = which == 0 ? KL_U : KL_VY;
    int64_t S, per;
    kl_plan(c, ps, &S, &per);
    const int64_t rows_pad = c->frows_pad[fa];
    const dim3 grid((unsigned)(rows_pad / KL_RB), (unsigned)S);
    const int64_t nparts = (int64_t)grid.x * grid.y;
    CHK(kl_ensure(c, c->kl_part, (size_t)nparts * sizeof(double)));
    KlArgs a;
    a.T = which == 0 ? c->X : c->Y;
    a.ldt = which == 0 ? c->dp : c->pp;
    a.A = A; a.B = B;
    a.cols_pad = c->frows_pad[fb];
    a.cols_per_share = per;
    a.rows_valid = c->frows[fa]; a.cols_valid = c->frows[fb];
    a.out = nullptr; a.slab_stride = 0;
    a.part = (double *)c->kl_part.p;
    {
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)c->frows[fa] * (double)c->frows[fb] * (double)c->k);
        switch (c->kp) {
        case 32: hipLaunchKernelGGL((kl_div_kernel<32>), grid, dim3(256), 0, c->stream, a); break;
        case 64: hipLaunchKernelGGL((kl_div_kernel<64>), grid, dim3(256), 0, c->stream, a); break;
        case 128: hipLaunchKernelGGL((kl_div_kernel<128>), grid, dim3(256), 0, c->stream, a); break;
        default: hipLaunchKernelGGL((kl_div_kernel<256>), grid, dim3(256), 0, c->stream, a); break;
        }
        hipLaunchKernelGGL(sum_doubles_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)a.part, nparts, small);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, small, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_kl_divergence(cmf_ctx *c, double *dx, double *dy) {
    NEED_PROBLEM(c);
    CHK(kl_check(c, "cmf_kl_divergence"));
    if (dx && !have_data(c, 0)) return fail(CMF_EINVAL, "cmf_kl_divergence: X has not been set");
    if (dy && !have_data(c, 1)) return fail(CMF_EINVAL, "cmf_kl_divergence: Y has not been set");
    DeviceGuard dg(c->device);
    CHK(kl_ensure(c, c->kl_small, kl_small_bytes(c)));
    if (dx) CHK(kl_divergence_side(c, 0, dx));
    if (dy) CHK(kl_divergence_side(c, 1, dy));
    return CMF_OK;
}

extern "C" int cmf_mu_kl_layout(cmf_ctx *c, int64_t *out4) {
    NEED_PROBLEM(c);
    if (!out4) return fail(CMF_EINVAL, "cmf_mu_kl_layout: null output");
    CHK(kl_check(c, "cmf_mu_kl_layout"));
    int64_t S, S2, per;
    kl_plan(c, KL_U, &S, &per);
    out4[0] = S;
    kl_plan(c, KL_VX, &S, &per);
    kl_plan(c, KL_VY, &S2, &per);
    out4[1] = std::max(S, S2);
    kl_plan(c, KL_Z, &S, &per);
    out4[2] = S;
    out4[3] = (int64_t)(kl_slab_bytes(c, CMF_UPD_U | CMF_UPD_V | CMF_UPD_Z) + kl_small_bytes(c));
    return CMF_OK;
}
#endif // CMF_KLMU_HOST
