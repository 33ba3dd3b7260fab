// cmf_als_cg.hip.h -- matrix-free conjugate-gradient row solves of the ALS solver (cmf_als_cg_step, cmf_als.hip.h)
// Every row f_i of a signed swept factor with an observed relation runs `steps` steps of plain CG on the system of cmf_als.hip.h
//   H_i f = g_i,    H_i = sum_{e in O_i} w_e b_e b_e^T + S + l2 I,    g_i = sum_{e in O_i} w_e t_e b_e + N_i
// from the row it has, without ever forming H_i: one product is one pass over the row's gathered factor rows,
//   H_i x = sum_e w_e b_e (b_e . x) + S x + l2 x,
// O(nnz k) per step instead of O(nnz k^2) for the normal equations plus k^3 / 3 for the Cholesky solve.
//     r = g - H f,  p = r;   per step:  q = H p,  alpha = (r.r) / (p.q),  f += alpha p,  r -= alpha q,  beta = (r'.r') / (r.r),  p = r' + beta p
// with true divisions.  A row stops when r.r or p.q is not a positive finite number and keeps what it has.
//
// als_cg_kernel<KP>: one 256-thread workgroup per row, all steps inside the one launch, nothing shared between workgroups, no
// atomics: the result of a row depends on that row alone and is deterministic to the bit.
//   * A pass with vector x: the entries of side 0, then of side 1, in stored order.  Wave (e mod 4) takes entry e and holds b_e in
//     registers, KP / 64 consecutive floats per lane (k_pad = 32: the upper half-wave holds zeros).  d_e = b_e . x by in-lane FMAs
//     and a butterfly over the 64 lanes (offsets 32 .. 1: every lane ends with the same bits); acc += (w_e d_e) b_e goes into
//     the wave's own accumulator.  The four accumulators are added through LDS in wave order by thread j < KP,
//     which then adds (S x)_j = sum_c S[c][j] x_c for c ascending (x broadcast from LDS, the row of S coalesced and served by L2)
//     and l2 x_j on the first k coordinates (LR = true: lambda_i x_j with the row's own lambda_i = l2 * mult[row], als_row_l2).
//     Padding coordinates stay exact zeros and are never written to the factor.
//   * The first pass fuses the right-hand side: its coefficient is pv_e - w_e (b_e . f), so it yields r = g - H f directly.  A row
//     is read steps + 1 times.
//   * r.r and p.q: a butterfly inside each wave, the four wave sums added in wave order.
//   * LDS residency: a row of at most `cap` entries keeps its gathered rows (and weights) in dynamic LDS after the first pass; a
//     longer one gathers them again every pass.  Both forms run the same arithmetic in the same order on the same values, so the
//     capacity class the host sorts a row into changes no bit of its result.
// Vector stores only; no scratch.
//
// Long rows (hot columns): a row with more than L stored entries ("als_cg_piece") leaves that kernel.  Its entries, side 0 then
// side 1 in stored order, are cut into pieces of L consecutive entries (the last one shorter; a piece may straddle the two sides),
// and one product H x becomes two plain launches, all long rows of the sweep together:
//   als_cg_piece_kernel<KP>    one 256-thread workgroup per piece: the entry pass over the piece's entries (wave e mod 4
//                              takes entry e of the piece, four in flight, b_e in registers, the butterfly dot, acc += coef b_e),
//                              the four wave accumulators added in wave order, the piece's partial [KP] to its own slot.  x comes
//                              from the row's state (f in the first pass, p afterwards), each lane its KP / 64 floats straight into
//                              registers.  Pieces always stream; 4 KP floats of static LDS.  A piece of a row that has stopped
//                              returns at once.  The non-negative rows (cmf_als_nncg.hip.h) launch this kernel too.
//   als_cg_combine_kernel<KP>  one workgroup per long row: thread j < KP adds the row's partials in piece order, then (S x)_j for c
//                              ascending and l2 x_j as `pass` does; the first launch forms r = g - H f (+ N), p = r, r.r, the later
//                              ones one CG step each with the formulas and the stop rule above; the last one writes f.
// The sum across workgroups is the kernel boundary: no atomics, no grid barrier, no workgroup waits for another.  The state
// (f, r, p [KP], r.r and an alive flag per long row) and the partials live in a scratch buffer of their own.  A long row's result
// depends on that row and on L alone.
//
// Shared with cmf_als_nncg.hip.h and cmf_als_dual.hip.h: als_lane_load / als_lane_store (a lane's KP / 64 floats),
// als_row_pass_accumulate (the entry pass of als_nncg_kernel and of the piece kernel; als_cg_kernel keeps its own copy of the loop,
// whose code object is the one it had before the fold), als_wg_sum (r.r and p.q here), als_long_row_product (both combine kernels).
#pragma once
#include "cmf_kernels.hip.h"

namespace cmfk {

struct AlsCgSide {
    const int64_t *indptr;  // of the whole image (indexed by the row of the swept factor)
    const int32_t *idx;
    const float *pv, *wv;   // p = w t, w
    const float *B;         // the gathered factor, pitch KP
};
struct AlsCgArgs {
    AlsCgSide s0, s1;       // s1.indptr == nullptr: one side
    const int64_t *rows;    // the rows of this launch (one per workgroup)
    const float *S, *N;     // full side: Gram [KP][KP] and T B [rows][KP]; or null
    const float *Fin;       // the swept factor, pitch KP (start of the iteration)
    float *Fout;            // where row r goes: Fout + (r - out_row0) * KP
    int64_t out_row0;
    float l2;
    int k, steps;
    int cap;                // entries a row may keep resident in this launch's dynamic LDS (0: every row streams)
    const float *l2m;       // per-row multipliers of l2 (cmf_set_l2_rows), indexed by the row of the swept factor; null: the LR = false instance
};

enum { ALS_CG_U = 4 };      // entries in flight per wave

// dynamic LDS: x [KP] | wave accumulators [4][KP] | wave sums [16] | resident rows [cap][KP] | resident weights [cap]
__host__ __device__ constexpr int als_cg_fixed_floats(int kp) { return 5 * kp + 16; }
__host__ __device__ constexpr int als_cg_entry_bytes(int kp) { return 4 * kp + 4; }

// lambda_i of a row.  LR = false (no multipliers bound): l2, and the instance is the kernel without any of this.  LR = true: the ONE
// float32 product l2 * mult[row], never fused into the addition that takes it: a row under a multiplier v has the bits of the same
// row under the scalar fl(l2 v).  The flag is a template argument of every kernel that reads a row's l2, as LG is of
// als_normal_kernel: with a run-time test of the pointer the row kernels of this file and of cmf_als_nncg.hip.h took one VGPR more
// and als_nncg_kernel<256> fell from 8 to 7 waves per SIMD.
template <bool LR>
__device__ __forceinline__ float als_row_l2(float l2, [[maybe_unused]] const float *mult, [[maybe_unused]] int64_t row) {
    if constexpr (LR) {   // (every caller's row is wave-uniform: the product is handed on in a scalar register)
#pragma clang fp contract(off)
        const float lam = l2 * mult[row];
        return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lam)));
    } else {
        return l2;
    }
}

__device__ __forceinline__ float als_cg_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over the workgroup of va (TWO: and of vb, which goes to *sb), zero in threads >= KP; the same bits in every thread: a butterfly
// inside each wave, the four wave sums through ws (4 floats, TWO: 8) and added in wave order.  One barrier.  The callers alternate
// between two such buffers, so that one is rewritten only after a barrier has passed since its last read.
template <bool TWO = false>
__device__ __forceinline__ float als_wg_sum(float *ws, int uw, int lane, float va, [[maybe_unused]] float vb = 0.f, [[maybe_unused]] float *sb = nullptr) {
    va = als_cg_wave_sum(va);
    if constexpr (TWO) vb = als_cg_wave_sum(vb);
    if (lane == 0) {
        ws[uw] = va;
        if constexpr (TWO) ws[4 + uw] = vb;
    }
    __syncthreads();
    if constexpr (TWO) *sb = ((ws[4] + ws[5]) + ws[6]) + ws[7];
    return ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// the VPL = 4 | 2 | 1 consecutive floats of one lane by one load or store, in global memory or LDS (p aligned to 4 VPL bytes)
template <int VPL>
__device__ __forceinline__ void als_lane_load(const float *p, float (&v)[VPL]) {
    static_assert(VPL == 4 || VPL == 2 || VPL == 1, "k_pad <= 256");
    if constexpr (VPL == 4) {
        const f32x4 x4 = *reinterpret_cast<const f32x4 *>(p);
        v[0] = x4[0]; v[1] = x4[1]; v[2] = x4[2]; v[3] = x4[3];
    } else if constexpr (VPL == 2) {
        const float2 x2 = *reinterpret_cast<const float2 *>(p);
        v[0] = x2.x; v[1] = x2.y;
    } else {
        v[0] = p[0];
    }
}
template <int VPL>
__device__ __forceinline__ void als_lane_store(float *p, const float (&v)[VPL]) {
    static_assert(VPL == 4 || VPL == 2 || VPL == 1, "k_pad <= 256");
    if constexpr (VPL == 4) *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]};
    else if constexpr (VPL == 2) *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    else p[0] = v[0];
}

// The entry pass of als_nncg_kernel (cmf_als_nncg.hip.h) and of als_cg_piece_kernel: acc += sum_e coef_e b_e over entries
// [e_begin, e_begin + n) of the row (side 0 then side 1 concatenated), wave uw taking every fourth of them, ALS_CG_U in flight:
// d_e = b_e . x by in-lane FMAs for v ascending and the butterfly, coef_e = w_e d_e, or FIRST: pv_e - w_e d_e.  resident: the
// gathered rows and weights are kept in res / resw by FIRST and read from there afterwards (written and read by the same wave).
// The loop of `pass` in als_cg_kernel below is the same loop, kept inline there.
template <int KP, bool FIRST, int VPL>
__device__ __forceinline__ void als_row_pass_accumulate(const AlsCgSide s0, const AlsCgSide s1, int64_t b0, int64_t b1, int n0, int e_begin, int n,
                                                        bool resident, float *res, float *resw, const float (&xr)[VPL], float (&acc)[VPL],
                                                        int uw, int lane, bool holds) {
    for (int e0 = uw; e0 < n; e0 += 4 * ALS_CG_U) {
        float b[ALS_CG_U][VPL], w[ALS_CG_U], pv[ALS_CG_U];
#pragma unroll
        for (int u = 0; u < ALS_CG_U; ++u) {
            const int e = e0 + 4 * u;                    // wave-uniform
#pragma unroll
            for (int v = 0; v < VPL; ++v) b[u][v] = 0.f;
            w[u] = pv[u] = 0.f;
            if (e >= n) continue;
            if (FIRST || !resident) {
                const int ge = e_begin + e;              // entry of the row
                const bool second = ge >= n0;
                const int64_t q = second ? b1 + (ge - n0) : b0 + ge;
                w[u] = (second ? s1.wv : s0.wv)[q];
                if (FIRST) pv[u] = (second ? s1.pv : s0.pv)[q];
                if (holds) {
                    als_lane_load<VPL>((second ? s1.B : s0.B) + (int64_t)(second ? s1.idx : s0.idx)[q] * KP + lane * VPL, b[u]);
                }
                if (FIRST && resident) {
                    if (holds) {
                        als_lane_store<VPL>(res + (int64_t)e * KP + lane * VPL, b[u]);
                    }
                    if (lane == 0) resw[e] = w[u];
                }
            } else {                                     // written by this same wave in the first pass
                w[u] = resw[e];
                if (holds) {
                    als_lane_load<VPL>(res + (int64_t)e * KP + lane * VPL, b[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ALS_CG_U; ++u) {
            float d = 0.f;
#pragma unroll
            for (int v = 0; v < VPL; ++v) d = fmaf(b[u][v], xr[v], d);
            d = als_cg_wave_sum(d);
            const float coef = FIRST ? pv[u] - w[u] * d : w[u] * d;
#pragma unroll
            for (int v = 0; v < VPL; ++v) acc[v] = fmaf(coef, b[u][v], acc[v]);
        }
    }
}

__device__ __forceinline__ bool als_cg_positive_finite(float v) { return v > 0.f && v <= 3.402823466e38f; }

template <int KP, bool LR>
__global__ __launch_bounds__(256) void als_cg_kernel(AlsCgArgs g) {
    constexpr int VPL = KP >= 64 ? KP / 64 : 1;     // floats of a gathered row per lane
    extern __shared__ __attribute__((aligned(16))) float als_cg_lds[];
    float *xs = als_cg_lds, *part = xs + KP, *wsum = part + 4 * KP, *res = wsum + 16;
    const int t = threadIdx.x, lane = t & 63;
    const int uw = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool holds = lane * VPL < KP;              // k_pad = 32: lanes 32 .. 63 carry zeros
    const int64_t row = g.rows[blockIdx.x];
    const int64_t b0 = g.s0.indptr[row], b1 = g.s1.indptr ? g.s1.indptr[row] : 0;
    const int n0 = (int)(g.s0.indptr[row + 1] - b0), n1 = g.s1.indptr ? (int)(g.s1.indptr[row + 1] - b1) : 0;
    const int n = n0 + n1;
    float *out = g.Fout + (row - g.out_row0) * KP;
    if (n == 0 && !g.S) {                            // a row without information
        if (t < g.k) out[t] = 0.f;
        return;
    }
    const bool resident = n <= g.cap;
    float *resw = res + (int64_t)g.cap * KP;
    const int k = g.k;

    // one pass: thread j < KP returns (sum_e coef_e b_e)_j + (S x)_j + l2 x_j with coef_e = w_e (b_e . x), or on the first pass
    // (x = f) the negative of that plus sum_e pv_e b_e: coef_e = pv_e - w_e (b_e . f)
    auto pass = [&](bool first) -> float {
        float xr[VPL], acc[VPL];
#pragma unroll
        for (int v = 0; v < VPL; ++v) {
            xr[v] = holds ? xs[lane * VPL + v] : 0.f;
            acc[v] = 0.f;
        }
        for (int e0 = uw; e0 < n; e0 += 4 * ALS_CG_U) {
            float b[ALS_CG_U][VPL], w[ALS_CG_U], pv[ALS_CG_U];
#pragma unroll
            for (int u = 0; u < ALS_CG_U; ++u) {
                const int e = e0 + 4 * u;            // wave-uniform
#pragma unroll
                for (int v = 0; v < VPL; ++v) b[u][v] = 0.f;
                w[u] = pv[u] = 0.f;
                if (e >= n) continue;
                if (first || !resident) {
                    const bool second = e >= n0;
                    const int64_t q = second ? b1 + (e - n0) : b0 + e;
                    w[u] = (second ? g.s1.wv : g.s0.wv)[q];
                    if (first) pv[u] = (second ? g.s1.pv : g.s0.pv)[q];
                    if (holds) {
                        als_lane_load<VPL>((second ? g.s1.B : g.s0.B) + (int64_t)(second ? g.s1.idx : g.s0.idx)[q] * KP + lane * VPL, b[u]);
                    }
                    if (first && resident) {
                        if (holds) {
                            als_lane_store<VPL>(res + (int64_t)e * KP + lane * VPL, b[u]);
                        }
                        if (lane == 0) resw[e] = w[u];
                    }
                } else {                             // written by this same wave in the first pass
                    w[u] = resw[e];
                    if (holds) {
                        als_lane_load<VPL>(res + (int64_t)e * KP + lane * VPL, b[u]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < ALS_CG_U; ++u) {
                float d = 0.f;
#pragma unroll
                for (int v = 0; v < VPL; ++v) d = fmaf(b[u][v], xr[v], d);
                d = als_cg_wave_sum(d);
                const float coef = first ? pv[u] - w[u] * d : w[u] * d;
#pragma unroll
                for (int v = 0; v < VPL; ++v) acc[v] = fmaf(coef, b[u][v], acc[v]);
            }
        }
        if (holds) {
#pragma unroll
            for (int v = 0; v < VPL; ++v) part[uw * KP + lane * VPL + v] = acc[v];
        }
        __syncthreads();
        float o = 0.f;
        if (t < KP) {
            o = ((part[t] + part[KP + t]) + part[2 * KP + t]) + part[3 * KP + t];
            float sx = 0.f;
            if (g.S) {
                for (int c = 0; c < k; ++c) sx = fmaf(g.S[c * KP + t], xs[c], sx);
            }
            if (t < k) sx += als_row_l2<LR>(g.l2, g.l2m, row) * xs[t];   // (wave-uniform)
            o = first ? o - sx : o + sx;
        }
        return o;
    };
    // sum over the workgroup of v (zero in threads >= KP), the same bits in every thread; `slot` 0 | 1 alternates so that a
    // buffer is rewritten only after a barrier has passed since its last read
    auto dot = [&](float v, int slot) -> float {
        return als_wg_sum(wsum + 4 * slot, uw, lane, v);
    };

    float f = 0.f, r = 0.f, p = 0.f;
    if (t < KP) {
        f = g.Fin[row * KP + t];
        xs[t] = f;
    }
    __syncthreads();
    r = pass(true);
    if (t < KP && g.N) r += g.N[row * KP + t];
    p = r;
    float rr = dot(r * r, 0);
    for (int s = 0; s < g.steps; ++s) {
        if (!(rr > 0.f) || !(rr <= 3.402823466e38f)) break;     // zero, or not finite: the row keeps what it has
        if (t < KP) xs[t] = p;
        __syncthreads();
        const float q = pass(false);
        const float pq = dot(p * q, 1);
        if (!(pq > 0.f) || !(pq <= 3.402823466e38f)) break;
        const float alpha = rr / pq;
        f = fmaf(alpha, p, f);
        r = fmaf(-alpha, q, r);
        const float rn = dot(r * r, 0);
        const float beta = rn / rr;
        p = fmaf(beta, p, r);
        rr = rn;
    }
    if (t < k) out[t] = f;
}

// ------------------------------------------------------------------ long rows, cut into pieces
struct AlsCgPiece {
    int32_t slot;           // the long row (index into AlsCgPieceArgs::rows) this piece belongs to
    int32_t first, count;   // entries [first, first + count) of the row, side 0 then side 1 concatenated
    int32_t pad;
};
struct AlsCgLongRow {
    int64_t row;            // of the swept factor
    int32_t first, pieces;  // its partial slots [first, first + pieces)
};
// What als_cg_piece_kernel reads, of the signed rows and of the non-negative ones (cmf_als_nncg.hip.h) alike; the combine kernels
// find the rows, their state and the partials here too.
struct AlsCgPieceArgs {
    AlsCgSide s0, s1;       // s1.indptr == nullptr: one side
    const AlsCgPiece *pieces;
    const AlsCgLongRow *rows;
    const float *Fin;       // the swept factor: x of the first pass
    float *state;           // [long row][state_vecs][KP]: f, r, the next vector (x of the later passes), ...
    float *partial;         // [piece][KP]
    const int32_t *takes;   // a row takes a later launch's pass when takes[slot * takes_stride] == takes_value (words the combines write)
    int state_vecs, takes_stride, takes_value;
    int first;              // the first pass: x = the factor row (clamp: max(., 0) of it), coefficient pv_e - w_e (b_e . x), every row takes it
    int clamp;
};

// One 256-thread workgroup per piece: the entry pass over the piece's entries, the four wave accumulators added in wave order, the
// piece's partial [KP] to its own slot.  Pieces always stream; 4 KP floats of static LDS.
template <int KP>
__global__ __launch_bounds__(256) void als_cg_piece_kernel(AlsCgPieceArgs g) {
    constexpr int VPL = KP >= 64 ? KP / 64 : 1;
    __shared__ __attribute__((aligned(16))) float part[4 * KP];
    const int t = threadIdx.x, lane = t & 63;
    const int uw = __builtin_amdgcn_readfirstlane(t >> 6);
    const bool holds = lane * VPL < KP;
    const AlsCgPiece pc = g.pieces[blockIdx.x];
    const bool first = g.first != 0;
    if (!first && g.takes[(int64_t)pc.slot * g.takes_stride] != g.takes_value) return;   // workgroup-uniform
    const int64_t row = g.rows[pc.slot].row;
    const int64_t b0 = g.s0.indptr[row], b1 = g.s1.indptr ? g.s1.indptr[row] : 0;
    const int n0 = (int)(g.s0.indptr[row + 1] - b0);
    const float *x = first ? g.Fin + row * KP : g.state + ((int64_t)pc.slot * g.state_vecs + 2) * KP;
    float xr[VPL], acc[VPL];
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
        xr[v] = holds ? x[lane * VPL + v] : 0.f;
        if (first && g.clamp) xr[v] = fmaxf(xr[v], 0.f);
        acc[v] = 0.f;
    }
    if (first) als_row_pass_accumulate<KP, true, VPL>(g.s0, g.s1, b0, b1, n0, pc.first, pc.count, false, nullptr, nullptr, xr, acc, uw, lane, holds);
    else als_row_pass_accumulate<KP, false, VPL>(g.s0, g.s1, b0, b1, n0, pc.first, pc.count, false, nullptr, nullptr, xr, acc, uw, lane, holds);
    if (holds) als_lane_store<VPL>(part + uw * KP + lane * VPL, acc);
    __syncthreads();
    if (t < KP) g.partial[(int64_t)blockIdx.x * KP + t] = ((part[t] + part[KP + t]) + part[2 * KP + t]) + part[3 * KP + t];
}

// thread t < KP of a combine kernel: the partials of its long row added in piece order, then -+ ((S x)_t + lambda_i x_t) with x in
// xs (LDS): S x for c ascending, lambda_i x_t on the first k coordinates, as `pass` of the row kernels adds them
template <int KP, bool LR>
__device__ __forceinline__ float als_long_row_product(const AlsCgPieceArgs &p, const AlsCgLongRow lr, const float *S, const float *xs, int k,
                                                      float l2, const float *l2m, bool first, int t) {
    float o = 0.f;
    const float *pp = p.partial + (int64_t)lr.first * KP + t;
    for (int q = 0; q < lr.pieces; ++q) o += pp[(int64_t)q * KP];
    float sx = 0.f;
    if (S) {
        for (int c = 0; c < k; ++c) sx = fmaf(S[c * KP + t], xs[c], sx);
    }
    if (t < k) sx += als_row_l2<LR>(l2, l2m, lr.row) * xs[t];   // (the row is wave-uniform)
    return first ? o - sx : o + sx;
}

struct AlsCgLongArgs {
    AlsCgPieceArgs p;       // state: [long row][3][KP]: f, r, p; takes: alive
    const float *S, *N;
    float *Fout;
    int64_t out_row0;
    float *rr;              // [long row]
    int32_t *alive;         // [long row]; p.takes points at the same words (the piece kernel only reads them): move both together
    float l2;
    int k;
    int phase;              // 0: the first pass / its combine; 1: a step; 2: the last step (f goes to Fout)
    const float *l2m;       // as AlsCgArgs (the combine finds its row through AlsCgLongRow::row)
};

template <int KP, bool LR>
__global__ __launch_bounds__(256) void als_cg_combine_kernel(AlsCgLongArgs g) {
    __shared__ float xs[KP], wsum[8];
    const int t = threadIdx.x, lane = t & 63;
    const int uw = __builtin_amdgcn_readfirstlane(t >> 6);
    const int slot = blockIdx.x, k = g.k;
    const AlsCgLongRow lr = g.p.rows[slot];
    float *st = g.p.state + (int64_t)slot * 3 * KP;
    float *out = g.Fout + (lr.row - g.out_row0) * KP;
    const bool first = g.phase == 0, last = g.phase == 2;
    if (!first && !g.alive[slot]) {                      // stopped earlier: the row keeps what it has
        if (last && t < k) out[t] = st[t];
        return;
    }
    float f = 0.f, r = 0.f, p = 0.f, o = 0.f;
    if (t < KP) {
        f = first ? g.p.Fin[lr.row * KP + t] : st[t];
        if (!first) {
            r = st[KP + t];
            p = st[2 * KP + t];
        }
        xs[t] = first ? f : p;
    }
    __syncthreads();
    if (t < KP) o = als_long_row_product<KP, LR>(g.p, lr, g.S, xs, k, g.l2, g.l2m, first, t);
    if (first) {
        r = o;
        if (t < KP && g.N) r += g.N[lr.row * KP + t];
        const float rr = als_wg_sum(wsum, uw, lane, r * r);
        if (t < KP) {
            st[t] = f;
            st[KP + t] = r;
            st[2 * KP + t] = r;
        }
        if (t == 0) {
            g.rr[slot] = rr;
            g.alive[slot] = als_cg_positive_finite(rr) ? 1 : 0;
        }
        return;
    }
    const float rr = g.rr[slot];
    const float pq = als_wg_sum(wsum + 4, uw, lane, p * o);
    if (!als_cg_positive_finite(pq)) {
        if (t == 0) g.alive[slot] = 0;
        if (last && t < k) out[t] = f;
        return;
    }
    const float alpha = rr / pq;
    f = fmaf(alpha, p, f);
    r = fmaf(-alpha, o, r);
    const float rn = als_wg_sum(wsum, uw, lane, r * r);
    const float beta = rn / rr;
    p = fmaf(beta, p, r);
    if (last) {
        if (t < k) out[t] = f;
        return;
    }
    if (t < KP) {
        st[t] = f;
        st[KP + t] = r;
        st[2 * KP + t] = p;
    }
    if (t == 0) {
        g.rr[slot] = rn;
        g.alive[slot] = als_cg_positive_finite(rn) ? 1 : 0;
    }
}

} // namespace cmfk
