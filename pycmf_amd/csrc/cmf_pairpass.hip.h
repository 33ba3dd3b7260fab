// cmf_pairpass.hip.h -- the fused two-product pass  out = f(A B^T, images) B  and its reduction  sum g(A B^T, images),  shared by
// the solvers whose update needs an element-wise operation BETWEEN two products over the same tiles (cmf_klmu.hip.h: the quotient
// t / s; cmf_wmu.hip.h: the product w s).  The m x d intermediate is never written to memory.  Included by those two files only.
//
// pairpass_kernel<KP, TRANS, P> / pairpass_reduce_kernel<KP, P>: one 256-thread workgroup (4 waves, one per SIMD) owns PP_RB = 128
// output rows -- wave w the rows 32 w .. 32 w + 31 of A, resident in KP / 2 registers per lane as in topk_scan_kernel -- and one
// share of the streamed rows of B, which pass through LDS in tiles of 8192 / KP rows (32 KB, register-staged: the loads of tile
// t + 1 travel under the MFMAs of tile t).  For each 32 x 32 sub-tile:
//   1. S^T = B_tile A_blk^T on v_mfma_f32_32x32x2_f32 with the STREAMED rows as the A operand and the owned rows as the B operand:
//      lane l holds 16 entries of ONE output row (l & 31); register r of lane half h = l >> 5 is streamed index
//      8 (r >> 2) + 4 h + (r & 3) of the 32.
//   2. the 16 registers meet the matching elements of up to two relation-shaped images (read as stored, TRANS = 0:
//      img[row][streamed], or transposed, TRANS = 1: img[streamed][row]; prefetched one sub-tile ahead).  The pass maps each
//      register in place; the reduction adds one float64 term per valid element.
//   3. (pass) out^T += B_tile^T R^T: register r goes straight back as the B operand of the second product (k = lane half), and the
//      A operand is read from the SAME LDS tile at the row register r stands for in that lane half -- the pairing of step 1.  The
//      k_pad columns are dealt to the MFMA rows so that a lane reads W = min(4, KP / 32) consecutive floats per LDS access:
//      accumulator kb = jj W + e, MFMA row i holds column W (i + 32 jj) + e.
// Every output element is ONE fma chain in an order fixed by this file, the share it belongs to and nothing else; the shares of
// an output block (few output rows, long stream) leave partial slabs that the update kernel sums in slab order; a share whose
// slab already holds another pass's contribution adds to it (acc_slabs).  No atomics.  The reduction keeps per-lane float64 sums
// and leaves one float64 partial per workgroup (summed by sum_doubles_kernel).
// Padding: rows and columns of the images, A and B beyond the valid extent are zero; a policy's map must send them to exact zeros.
//
// A policy P is a type with
//   static constexpr bool DOT      step 1 runs (false: the registers start at zero and no owned rows are loaded)
//   static constexpr int IMAGES    relation-shaped images prefetched per sub-tile: 0, 1 or 2 (PairPassArgs::img0, img1)
//   static float map(s, x0, x1)    pass: what a register becomes before step 3 (x0, x1: the facing elements of img0, img1)
//   static double term(s, x0, x1)  reduction: what one valid element adds to the float64 sum
//   static constexpr bool ADDS     pass: a share may add to a slab another pass of the sweep wrote (acc_slabs is honoured); a
//                                  policy whose solver keeps the passes of a sweep in slabs of their own says false
// and optionally (absent: 1 and false -- every instantiation without them compiles to what it compiled to before they existed)
//   static constexpr int OUTPUTS   2: the DUAL-OUTPUT pass.  static void map2(s, x0, param, float *n, float *d) turns a register into
//                                  a PAIR; in step 3 every fragment b read from LDS is the A operand of two MFMAs, nacc += b n_r and
//                                  dacc += b d_r, and the epilogue writes a second slab set (PairPassArgs::out2) laid out like the
//                                  first.  A B^T is formed once for both products.  IMAGES <= 1, ADDS = false.
//   static constexpr bool PARAM    map / term take PairPassArgs::param as their third argument instead of x1 (IMAGES <= 1)
// Arithmetic lives in the policies in a literal form each: the library is built with the compiler's default contraction, so a
// reshaped expression can round differently.
//
// The CSR counterparts share csr_row_pairs / csr_row_each (a group of GL = KP / 4 lanes owns an output row and dots it with each
// gathered row of B by DPP group_sum) and the reduction body csr_reduce; block_sum64 is the float64 epilogue of every reduction here.
#pragma once
#include "cmf_kernels.hip.h"
#include "cmf_sparse.hip.h"

namespace cmfk {

enum { PP_RB = 128, PP_TILE_FLOATS = 8192 };
#define CMF_MU_EPS 1.1920928955078125e-07f // 2^-23: the reference's EPSILON

struct PairPassArgs {
    const float *img0;       // the first relation-shaped image of the policy
    int64_t ldt;             // pitch of the images
    const float *A;          // the factor that owns the output rows, pitch KP
    const float *B;          // the streamed factor, pitch KP
    int64_t cols_pad;        // streamed extent (multiple of 256)
    int64_t cols_per_share;  // multiple of 256
    int64_t rows_valid, cols_valid; // reduction only
    float *out;              // [share][rows_pad][KP]
    int64_t slab_stride;
    double *part;            // reduction: one partial per workgroup
    // what only some policies read comes last
    const float *img1;       // the second image (IMAGES = 2)
    int acc_slabs;           // ADDS: shares below this one add to what their slab holds
    float *out2;             // OUTPUTS = 2: the second slab set, [share][rows_pad][KP]
    float param;             // PARAM / OUTPUTS = 2: the policy's float parameter (cmf_betamu.hip.h: beta)
};

template <class P, class = void> struct pp_outputs { static constexpr int value = 1; };
template <class P> struct pp_outputs<P, std::void_t<decltype(P::OUTPUTS)>> { static constexpr int value = P::OUTPUTS; };
template <class P, class = void> struct pp_param { static constexpr bool value = false; };
template <class P> struct pp_param<P, std::void_t<decltype(P::PARAM)>> { static constexpr bool value = P::PARAM; };

// sum of v over a 256-thread workgroup in a fixed order (lanes by the shuffle ladder, then the four waves); red: 4 doubles of LDS,
// which may have held something else until now
__device__ __forceinline__ double block_sum64(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads(); // every wave is done with what red held
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <int KP, int TRANS, class P, bool REDUCE>
__device__ __forceinline__ void pairpass_body(const PairPassArgs &g, f32x4 *tile) {
    constexpr int NIMG = P::IMAGES;
    constexpr bool DUAL = !REDUCE && pp_outputs<P>::value == 2;
    constexpr bool PARAM = pp_param<P>::value;
    static_assert(!(DUAL || PARAM) || NIMG <= 1, "a dual-output or parameterised policy reads at most one image");
    constexpr int CT = PP_TILE_FLOATS / KP;   // streamed rows per LDS tile (32 at KP = 256 ... 256 at KP = 32)
    constexpr int SLOTS = KP / 4;             // float4 slots per row
    constexpr int SW = (SLOTS < 16 ? SLOTS : 16) - 1; // slot ^ (row & SW): rows of one fragment read land on different banks
    constexpr int NCH = KP / 8;               // 8-deep k pieces: one float4 per lane half
    constexpr int KB = KP / 32;               // output accumulators per wave (32 columns each)
    constexpr int W = KB < 4 ? KB : 4;        // floats per LDS access of the second product
    constexpr int NJ = KB / W;
    constexpr int SUBS = CT / 32;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, li = lane & 31;
    const int64_t row = (int64_t)blockIdx.x * PP_RB + wave * 32 + li; // output row of this lane (rows_pad is a multiple of PP_RB)

    // the owned row in registers: piece c = floats 8 c + 4 h .. + 3
    f32x4 af[P::DOT ? NCH : 1];
    if constexpr (P::DOT) {
        const f32x4 *src = (const f32x4 *)(g.A + row * KP);
#pragma unroll
        for (int c = 0; c < NCH; ++c) af[c] = src[2 * c + h];
    }
    const int64_t c_begin = (int64_t)blockIdx.y * g.cols_per_share;
    const int64_t c_end = min(c_begin + g.cols_per_share, g.cols_pad);
    const int ntiles = c_end > c_begin ? (int)((c_end - c_begin) / CT) : 0;

    f32x16 nacc[REDUCE ? 1 : KB];
#pragma unroll
    for (int kb = 0; kb < (REDUCE ? 1 : KB); ++kb) nacc[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 dacc[DUAL ? KB : 1]; // the second product of a dual-output pass
    if constexpr (DUAL) {
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) dacc[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    }
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
    f32x4 x0[4], x0n[4], x1[4], x1n[4]; // of img0 and img1: this sub-tile's and the next one's
    if (ntiles > 0) {
        fetch(0);
        if constexpr (NIMG > 0) fetch_e(x0, g.img0, c_begin);
        if constexpr (NIMG > 1) fetch_e(x1, g.img1, c_begin);
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
                if constexpr (NIMG > 0) fetch_e(x0n, g.img0, cb + 32);
                if constexpr (NIMG > 1) fetch_e(x1n, g.img1, cb + 32);
            }
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            if constexpr (P::DOT) {
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
            if constexpr (REDUCE) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t col = cb + 8 * (r >> 2) + 4 * h + (r & 3);
                    if (row < g.rows_valid && col < g.cols_valid) {
                        if constexpr (PARAM) dsum += P::term(acc[r], NIMG > 0 ? x0[r >> 2][r & 3] : 0.f, g.param);
                        else dsum += P::term(acc[r], NIMG > 0 ? x0[r >> 2][r & 3] : 0.f, NIMG > 1 ? x1[r >> 2][r & 3] : 0.f);
                    }
                }
            } else {
                f32x16 acc2; // DUAL: the registers of the second product
                if constexpr (DUAL) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        float n, d;
                        P::map2(acc[r], NIMG > 0 ? x0[r >> 2][r & 3] : 0.f, g.param, &n, &d);
                        acc[r] = n;
                        acc2[r] = d;
                    }
                } else if constexpr (PARAM) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = P::map(acc[r], NIMG > 0 ? x0[r >> 2][r & 3] : 0.f, g.param);
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = P::map(acc[r], NIMG > 0 ? x0[r >> 2][r & 3] : 0.f, NIMG > 1 ? x1[r >> 2][r & 3] : 0.f);
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
                            for (int e = 0; e < 4; ++e) {
                                nacc[jj * 4 + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[e], acc[r], nacc[jj * 4 + e], 0, 0, 0);
                                if constexpr (DUAL) dacc[jj * 4 + e] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[e], acc2[r], dacc[jj * 4 + e], 0, 0, 0);
                            }
                        } else if constexpr (W == 2) {
                            const f32x2 b = *(const f32x2 *)p;
                            nacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[0], acc[r], nacc[0], 0, 0, 0);
                            nacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[1], acc[r], nacc[1], 0, 0, 0);
                            if constexpr (DUAL) {
                                dacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[0], acc2[r], dacc[0], 0, 0, 0);
                                dacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[1], acc2[r], dacc[1], 0, 0, 0);
                            }
                        } else {
                            nacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(*p, acc[r], nacc[0], 0, 0, 0);
                            if constexpr (DUAL) dacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(*p, acc2[r], dacc[0], 0, 0, 0);
                        }
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if constexpr (NIMG > 0) x0[q] = x0n[q];
                    if constexpr (NIMG > 1) x1[q] = x1n[q];
                }
            }
        }
    }

    if constexpr (REDUCE) {
        const double s = block_sum64(dsum, (double *)tile);
        if (tid == 0) g.part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    } else {
        // accumulator kb = jj W + e, register r2: column W (i + 32 jj) + e with i = (r2 & 3) + 8 (r2 >> 2) + 4 h; row = this lane's
        float *dst = g.out + (int64_t)blockIdx.y * g.slab_stride + row * KP;
        const bool add = P::ADDS && (int)blockIdx.y < g.acc_slabs;
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
        if constexpr (DUAL) { // the second slab set: the same map, no adding (a dual policy keeps the passes of a sweep apart)
            float *dst2 = g.out2 + (int64_t)blockIdx.y * g.slab_stride + row * KP;
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj)
#pragma unroll
                for (int r2 = 0; r2 < 16; ++r2) {
                    const int i = (r2 & 3) + 8 * (r2 >> 2) + 4 * h;
                    float *p = dst2 + W * (i + 32 * jj);
                    if constexpr (W == 4) *(f32x4 *)p = f32x4{dacc[jj * 4][r2], dacc[jj * 4 + 1][r2], dacc[jj * 4 + 2][r2], dacc[jj * 4 + 3][r2]};
                    else if constexpr (W == 2) *(f32x2 *)p = f32x2{dacc[0][r2], dacc[1][r2]};
                    else *p = dacc[0][r2];
                }
        }
    }
}

// (a dual-output policy at KP = 64 holds two accumulator sets beside the transposed image's addresses: it takes the whole register
// file of a SIMD, as every policy does from KP = 128 on; the single-output instantiations keep their bounds)
template <int KP, int TRANS, class P>
__global__ __launch_bounds__(256, KP >= 128 || (KP == 64 && pp_outputs<P>::value == 2) ? 1 : 2) void pairpass_kernel(PairPassArgs g) {
    __shared__ __attribute__((aligned(16))) f32x4 pp_tile[PP_TILE_FLOATS / 4];
    pairpass_body<KP, TRANS, P, false>(g, pp_tile);
}
template <int KP, class P>
__global__ __launch_bounds__(256, KP == 256 ? 1 : 2) void pairpass_reduce_kernel(PairPassArgs g) {
    __shared__ __attribute__((aligned(16))) f32x4 pp_tile[PP_TILE_FLOATS / 4];
    pairpass_body<KP, 0, P, true>(g, pp_tile);
}

// ------------------------------------------------------------------ CSR: a group of GL = KP / 4 lanes owns a row
// a CSR pattern with the value arrays its kernels read: p = w t, w and t (each may be null where no kernel of the caller reads it)
struct PairCsrView {
    const int64_t *indptr;
    const int32_t *idx;
    const float *pv, *wv, *tv;
    int64_t rows;
};

// the row of this lane's group (256-thread workgroups of 64 / GL rows per wave) and the lane's place in it
template <int GL>
__device__ __forceinline__ int64_t csr_group_row(int *gl) {
    const int lane = threadIdx.x & 63;
    *gl = lane % GL;
    return ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (64 / GL) + lane / GL;
}
__device__ __forceinline__ f32x4 csr_lane4(const float *F, int64_t r, int kp, int gl) { return *reinterpret_cast<const f32x4 *>(F + r * kp + 4 * gl); }
template <int GL>
__device__ __forceinline__ float csr_group_dot(const f32x4 &a, const f32x4 &b) {
    float d = 0.f;
    d += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    return group_sum<GL>(d);
}

// entry(v, A_row . B_c, the lane's four floats of B_c) for the stored entries q of `row`, in stored order, two independent gathers
// in flight; v[n] = val[n][q], n < NV, loaded ahead of the gathers
template <int GL, int NV, class F>
__device__ __forceinline__ void csr_row_pairs(const int64_t *indptr, const int32_t *idx, const float *const *val, const float *A, const float *B, int kp, int64_t row,
                                              int gl, F &&entry) {
    const f32x4 a = csr_lane4(A, row, kp, gl);
    const int64_t end = indptr[row + 1];
    int64_t q = indptr[row];
    for (; q + 2 <= end; q += 2) {
        const int32_t j0 = idx[q], j1 = idx[q + 1];
        float v0[NV], v1[NV];
#pragma unroll
        for (int n = 0; n < NV; ++n) v0[n] = val[n][q], v1[n] = val[n][q + 1];
        const f32x4 b0 = csr_lane4(B, j0, kp, gl), b1 = csr_lane4(B, j1, kp, gl);
        const float d0 = csr_group_dot<GL>(a, b0), d1 = csr_group_dot<GL>(a, b1);
        entry(v0, d0, b0);
        entry(v1, d1, b1);
    }
    if (q < end) {
        const int32_t j0 = idx[q];
        float v0[NV];
#pragma unroll
        for (int n = 0; n < NV; ++n) v0[n] = val[n][q];
        const f32x4 b0 = csr_lane4(B, j0, kp, gl);
        entry(v0, csr_group_dot<GL>(a, b0), b0);
    }
}
// entry(v, A_row . B_c) for the stored entries of `row`, one gather at a time
template <int GL, int NV, class F>
__device__ __forceinline__ void csr_row_each(const int64_t *indptr, const int32_t *idx, const float *const *val, const float *A, const float *B, int kp, int64_t row,
                                             int gl, F &&entry) {
    const f32x4 a = csr_lane4(A, row, kp, gl);
    const int64_t end = indptr[row + 1];
    for (int64_t q = indptr[row]; q < end; ++q) {
        const int32_t j = idx[q];
        float v[NV];
#pragma unroll
        for (int n = 0; n < NV; ++n) v[n] = val[n][q];
        entry(v, csr_group_dot<GL>(a, csr_lane4(B, j, kp, gl)));
    }
}

// The body of a reduction kernel (256 threads): P::NS float64 sums over the stored entries, P::add(v, A_r . B_c, acc) once per
// entry, v[0] = t and (P::NV = 2) v[1] = w; partials[s * gridDim.x + b] = the share of sum s of workgroup b (summed in slot order
// by sum_doubles_kernel)
template <int GL, class P>
__device__ __forceinline__ void csr_reduce(const PairCsrView &T, const float *A, const float *B, int kp, double *partials) {
    static_assert(P::NV >= 1 && P::NV <= 2, "a reduction policy reads t, or t and w");
    int gl;
    const int64_t row = csr_group_row<GL>(&gl);
    double acc[P::NS] = {};
    const float *val[2] = {T.tv, T.wv};
    if (row < T.rows)
        csr_row_each<GL, P::NV>(T.indptr, T.idx, val, A, B, kp, row, gl, [&](const float *v, float d) {
            if (gl == 0) P::add(v, d, acc);
        });
    __shared__ double red[P::NS][4];
#pragma unroll
    for (int s = 0; s < P::NS; ++s) {
        const double v = block_sum64(acc[s], red[s]);
        if (threadIdx.x == 0) partials[(int64_t)s * gridDim.x + blockIdx.x] = v;
    }
}

// ------------------------------------------------------------------ the update
// F <- F * num / reg(den, F), num = the sum of the nslab numerator slabs in slab order; den = the column sums `den[k_pad]`
// broadcast over the rows (DEN_COLSUM) or the sum of nslab denominator slabs in slab order (DEN_SLABS);
// reg(den, F) = den + l1 + l2 F, then den == 0 -> eps   (MUSolver._regularized_delta, cmf_solvers.py:212-228)
// POW (the beta-divergence update, cmf_betamu.hip.h): F <- F * (num / reg(den, F))^gamma for gamma != 1 -- sqrtf at gamma = 1/2,
// otherwise exp2(gamma log2(q)) on the raw v_log_f32 / v_exp_f32 (q = 0 gives an exact 0 either way)
enum { DEN_COLSUM = 0, DEN_SLABS = 1 };
template <int DEN, bool POW = false>
__global__ void pairpass_update_kernel(float *F, const float *num, const float *den, int nslab, int64_t stride, int kp, int64_t n4, float l1, float l2, float eps,
                                       float gamma = 1.f) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 f = reinterpret_cast<f32x4 *>(F)[i];
        f32x4 nu = reinterpret_cast<const f32x4 *>(num)[i];
        f32x4 de = DEN == DEN_SLABS ? reinterpret_cast<const f32x4 *>(den)[i] : *reinterpret_cast<const f32x4 *>(den + (4 * i) % kp);
        for (int s = 1; s < nslab; ++s) {
            nu += reinterpret_cast<const f32x4 *>(num + (int64_t)s * stride)[i];
            if constexpr (DEN == DEN_SLABS) de += reinterpret_cast<const f32x4 *>(den + (int64_t)s * stride)[i];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float d = de[e];
            if (l1 > 0.f) d += l1;
            if (l2 > 0.f) d = d + l2 * f[e];
            if (d == 0.f) d = eps;
            if constexpr (POW) {
                float q = nu[e] / d;
                if (gamma == 0.5f) q = sqrtf(q);
                else if (gamma != 1.f) q = __builtin_amdgcn_exp2f(gamma * __builtin_amdgcn_logf(q));
                f[e] = f[e] * q;
            } else
                f[e] = f[e] * (nu[e] / d);
        }
        reinterpret_cast<f32x4 *>(F)[i] = f;
    }
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx)
#ifdef CMF_PAIRPASS_HOST

struct PairPass { int which; bool trans; int fa, fb; }; // relation X | Y (transposed), owner factor, streamed factor
static const PairPass PP_U{0, false, CMF_U, CMF_V}, PP_VX{0, true, CMF_V, CMF_U}, PP_VY{1, false, CMF_V, CMF_Z}, PP_Z{1, true, CMF_Z, CMF_V};

// Share rule of the dense pass: a sweep with fewer 128-row blocks than CUs cuts the stream into as many shares as bring the
// grid up to one workgroup per CU (at most one share per 256 streamed rows); forced > 0 fixes the count.  S = 1 for CSR.
static void pp_plan(const cmf_ctx *c, const PairPass &ps, int forced, bool csr, int64_t *S, int64_t *per) {
    if (csr) { *S = 1; *per = 0; return; }
    const int64_t nblk = c->frows_pad[ps.fa] / PP_RB, cblocks = c->frows_pad[ps.fb] / 256;
    int64_t s = forced > 0 ? forced : (nblk >= c->num_cu ? 1 : (c->num_cu + nblk - 1) / nblk);
    s = std::max<int64_t>(1, std::min<int64_t>(s, cblocks));
    *per = (cblocks + s - 1) / s * 256;
    *S = (c->frows_pad[ps.fb] + *per - 1) / *per;
}

// the arguments of a dense pass that follow from the pass alone; the caller adds the images and where the result goes
static PairPassArgs pp_args(const cmf_ctx *c, const PairPass &ps, int64_t per) {
    PairPassArgs a;
    memset(&a, 0, sizeof a);
    a.ldt = ps.which == 0 ? c->dp : c->pp;
    a.A = c->F[ps.fa]; a.B = c->F[ps.fb];
    a.cols_pad = c->frows_pad[ps.fb];
    a.cols_per_share = per;
    a.rows_valid = c->frows[ps.fa]; a.cols_valid = c->frows[ps.fb];
    a.slab_stride = c->frows_pad[ps.fa] * c->kp;
    return a;
}
static dim3 pp_grid(const cmf_ctx *c, const PairPass &ps, int64_t S) { return dim3((unsigned)(c->frows_pad[ps.fa] / PP_RB), (unsigned)S); }

template <class P>
static int pp_launch_pass(cmf_ctx *c, const PairPass &ps, const PairPassArgs &a, int64_t S) {
    const dim3 grid = pp_grid(c, ps, S);
    with_kp(c->kp, [&](auto kp) {
        if (ps.trans) hipLaunchKernelGGL((pairpass_kernel<decltype(kp)::value, 1, P>), grid, dim3(256), 0, c->stream, a);
        else hipLaunchKernelGGL((pairpass_kernel<decltype(kp)::value, 0, P>), grid, dim3(256), 0, c->stream, a);
    });
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// sum of P::term over the relation of `ps` into *sum (device): a.part holds one partial per workgroup of the S shares
template <class P>
static int pp_launch_reduce(cmf_ctx *c, const PairPass &ps, const PairPassArgs &a, int64_t S, double *sum) {
    const dim3 grid = pp_grid(c, ps, S);
    with_kp(c->kp, [&](auto kp) { hipLaunchKernelGGL((pairpass_reduce_kernel<decltype(kp)::value, P>), grid, dim3(256), 0, c->stream, a); });
    hipLaunchKernelGGL(sum_doubles_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)a.part, (int64_t)grid.x * grid.y, sum);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// workgroups of a CSR reduction kernel over `rows` rows
static unsigned csr_reduce_blocks(const cmf_ctx *c, int64_t rows) {
    const int rpw = 64 / (c->kp / 4);
    return (unsigned)std::max<int64_t>(1, ((rows + rpw - 1) / rpw + 3) / 4);
}
// launch(GL as an integral_constant, grid) starts a reduction kernel that leaves NS * blocks partials in `part`; their NS sums
// into sum[0 .. NS) (device)
template <int NS, class L>
static int csr_launch_reduce(cmf_ctx *c, int64_t rows, double *part, double *sum, L &&launch) {
    const unsigned blocks = csr_reduce_blocks(c, rows);
    with_kp(c->kp, [&](auto kp) { launch(std::integral_constant<int, decltype(kp)::value / 4>(), dim3(blocks)); });
    for (int s = 0; s < NS; ++s)
        hipLaunchKernelGGL(sum_doubles_kernel, dim3(1), dim3(256), 0, c->stream, (const double *)(part + (size_t)s * blocks), (int64_t)blocks, sum + s);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// F[f] <- F[f] * num / reg(den, F[f])   (pairpass_update_kernel; den: k_pad column sums, or nslab slabs like num; POW: the
// quotient raised to gamma)
template <int DEN, bool POW = false>
static int pp_update(cmf_ctx *c, int f, const float *num, const float *den, int nslab, double l1, double l2, double gamma = 1.0) {
    const int64_t n4 = c->frows_pad[f] * c->kp / 4;
    Timed tm(c, CMF_K_ELEMWISE);
    const unsigned blocks = (unsigned)std::min<int64_t>((n4 + 255) / 256, 4096);
    hipLaunchKernelGGL((pairpass_update_kernel<DEN, POW>), dim3(blocks), dim3(256), 0, c->stream, c->F[f], num, den, nslab, c->frows_pad[f] * c->kp, c->kp, n4, (float)l1,
                       (float)l2, CMF_MU_EPS, (float)gamma);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}
#endif // CMF_PAIRPASS_HOST
