// cmf_als_nnls.hip.h -- the non-negative row solve of the ALS sweeps: cyclic coordinate descent on
//   min_{f >= 0}  1/2 f^T H_i f - g_i^T f
// for the finished per-row systems of cmf_als.hip.h (H_i symmetric to the bit, H_i >= l2 I, 1 on the padding diagonal), warm-started
// from the row of the factor and updated in place.  One sweep of a row:
//   r = g - H f                                   (formed anew for every sweep, never carried across sweeps)
//   for j = 0 .. k - 1:   new = max(0, f_j + r_j / H_jj)   (a true division);   delta = new - f_j;   f_j = new;   r -= delta H[j, :]
// Every step is the exact minimiser along coordinate j, so the row objective never rises.  Column j of H is read as ROW j.
//
// als_nnls_kernel<KP>: one wave per row, four rows per 256-thread workgroup, no LDS and no barrier.  Lane l holds the V = KP / 64
// (KP = 32: 1, on 32 lanes) consecutive coordinates V l .. V l + V - 1 of f, of r and of the row of H in flight, so a row of H is
// one coalesced load of up to 16 B per lane.  The values a step needs (f_j, r_j, H_jj) come from the owner lane j / V by a
// wave-uniform lane read; every lane then computes the same new, delta: no reduction in the sequential chain.
// The rows of H are streamed, 8 at a time, one block of 8 ahead of the chain (the addresses do not depend on the data; the block
// after the last one of a pass is the first one of the next pass).  So that H is read ONCE per sweep, the residual of the next
// sweep is formed during this one from the same registers:  rn = g - sum_j new_j H[j, :], which is g - H f of the swept row.  Only
// the residual of the warm start costs a pass of its own: sweeps + 1 reads of H_i per call.
// A step with delta == 0 skips its update of r, one with new == 0 its update of rn (wave-uniform branches; from a start far from
// the minimiser most coordinates are clipped).  A row whose whole sweep moved nothing stops: further sweeps would be no-ops.
// Coordinates >= k are neither pivots nor written: the padding of F stays zero.  A row without information (no piece and no full
// side: first[row] == first[row + 1], H = l2 I, g = 0) is set to exact zeros without a sweep.
// The result of a row depends on its own H, g, f and `sweeps` only: no atomics, nothing depends on the grid or on the chunk.
#pragma once
#include "cmf_kernels.hip.h"

namespace cmfk {

enum { NNLS_WAVES = 4, NNLS_PF = 8 };

struct NnlsArgs {
    const float *H;        // [nrows][KP][KP]
    const float *g;        // [nrows][KP]
    float *F;              // [nrows][KP]: warm start in, swept rows out
    const int64_t *first;  // [nrows + 1] piece slots of the rows, or null: every row carries information
    int64_t nrows;
    int k, sweeps;
};

template <int KP>
__global__ __launch_bounds__(64 * NNLS_WAVES) void als_nnls_kernel(NnlsArgs a) {
    constexpr int V = KP >= 64 ? KP / 64 : 1, LA = KP / V, PF = NNLS_PF;
    static_assert(PF % V == 0 && KP % PF == 0, "a block of rows holds whole lanes of pivots");
    const int lane = threadIdx.x & 63, ll = lane % LA;   // KP = 32: lanes 32 .. 63 shadow lanes 0 .. 31 and store nothing
    const int64_t row = (int64_t)blockIdx.x * NNLS_WAVES + (threadIdx.x >> 6);
    if (row >= a.nrows) return;
    const int k = a.k, c0 = V * ll;
    float *fp = a.F + row * KP + c0;
    if (a.first && a.first[row] == a.first[row + 1]) {
        if (lane < LA)
#pragma unroll
            for (int q = 0; q < V; ++q)
                if (c0 + q < k) fp[q] = 0.f;
        return;
    }
    const float *Hr = a.H + row * (int64_t)KP * KP + c0;
    float fv[V], gv[V], rv[V], rn[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
        fv[q] = fp[q];
        gv[q] = a.g[row * KP + c0 + q];
        rv[q] = gv[q];
    }
    auto rl = [](float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); };
    float cur[PF][V], nxt[PF][V];
    auto load = [&](int b, float (&dst)[PF][V]) {   // rows 8 b .. 8 b + 7 of H_i: below KP, whatever k
        const float *src = Hr + (int64_t)(PF * b) * KP;
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            if constexpr (V == 4) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(src + i * KP);
                dst[i][0] = v[0]; dst[i][1] = v[1]; dst[i][2] = v[2]; dst[i][3] = v[3];
            } else if constexpr (V == 2) {
                const f32x2 v = *reinterpret_cast<const f32x2 *>(src + i * KP);
                dst[i][0] = v[0]; dst[i][1] = v[1];
            } else {
                dst[i][0] = src[i * KP];
            }
        }
    };
    const int nb = (k + PF - 1) / PF;
    load(0, nxt);
    // the residual of the warm start: r = g - sum_j f_j H[j, :]
    for (int b = 0; b < nb; ++b) {
#pragma unroll
        for (int i = 0; i < PF; ++i)
#pragma unroll
            for (int q = 0; q < V; ++q) cur[i][q] = nxt[i][q];
        load(b + 1 < nb ? b + 1 : 0, nxt);
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            if (PF * b + i >= k) break;
            const float fj = rl(fv[i % V], (PF / V) * b + i / V);
#pragma unroll
            for (int q = 0; q < V; ++q) rv[q] = fmaf(-fj, cur[i][q], rv[q]);
        }
    }
    for (int s = 0; s < a.sweeps; ++s) {
        const bool last = s + 1 == a.sweeps;
        bool moved = false;
#pragma unroll
        for (int q = 0; q < V; ++q) rn[q] = gv[q];
        for (int b = 0; b < nb; ++b) {
#pragma unroll
            for (int i = 0; i < PF; ++i)
#pragma unroll
                for (int q = 0; q < V; ++q) cur[i][q] = nxt[i][q];
            load(b + 1 < nb ? b + 1 : 0, nxt);
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                if (PF * b + i >= k) break;
                const int ol = (PF / V) * b + i / V;     // the lane that owns coordinate j = 8 b + i, in its register i % V
                const float fj = rl(fv[i % V], ol), rj = rl(rv[i % V], ol), hjj = rl(cur[i][i % V], ol);
                const float nw = fmaxf(0.f, fj + rj / hjj);
                const float dl = nw - fj;
                fv[i % V] = lane == ol ? nw : fv[i % V];
                if (dl != 0.f) {
                    moved = true;
#pragma unroll
                    for (int q = 0; q < V; ++q) rv[q] = fmaf(-dl, cur[i][q], rv[q]);
                }
                if (!last && nw != 0.f) {
#pragma unroll
                    for (int q = 0; q < V; ++q) rn[q] = fmaf(-nw, cur[i][q], rn[q]);
                }
            }
        }
        if (!moved) break;
#pragma unroll
        for (int q = 0; q < V; ++q) rv[q] = rn[q];
    }
    if (lane < LA)
#pragma unroll
        for (int q = 0; q < V; ++q)
            if (c0 + q < k) fp[q] = fv[q];
}

} // namespace cmfk
