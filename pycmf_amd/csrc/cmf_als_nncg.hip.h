// cmf_als_nncg.hip.h -- matrix-free NON-NEGATIVE row solves of the ALS solver (cmf_als_nncg_step, cmf_als.hip.h)
// Every row f_i >= 0 of a non-negative swept factor with an observed relation runs `steps` steps of projected conjugate gradients
// on the quadratic of cmf_als_cg.hip.h,  q(f) = 1/2 f^T H_i f - g_i^T f,  with the product of that file and never H_i itself:
//   H_i x = sum_e w_e b_e (b_e . x) + S x + l2 x.
//     f <- max(f, 0);  r = g - H f  (the first pass, right-hand side fused);  p = none
//     per step:  free_j = f_j > 0 or r_j > 0;  z = r on free, 0 elsewhere;  rho = z.z;  stop unless rho is positive and finite
//                p = z + (rho / rho_old) p  if the step before was a free step and left the same free set,  else p = z
//                q = H p;  pq = p.q;  stop unless positive and finite;  alpha = (p.r) / pq;  t = f + alpha p
//                no t_j < 0:  the FREE step       f = t,  r -= alpha q,  rho_old = rho,  free_old = free
//                otherwise    the PROJECTED step  f+ = max(t, 0),  d = f+ - f,  hd = H d (a second pass),  dr = d.r,  dhd = d.hd;
//                             stop unless both are positive and finite;  theta = dr / dhd;
//                             theta >= 1:  f = f+ (exact zeros),  r -= hd;   else  f = max(f + theta d, 0),  r -= theta hd;   p = none
// A stopped row keeps what it has; a row without information becomes exact zeros; padding coordinates are never free and stay
// exact zeros.  Every step is a line search along a descent direction of q that stops at or before the exact minimiser of the line
// and leaves the row feasible, so q never rises.  One or two passes per step: a row is read at most
// 2 steps + 1 times.
//
// als_nncg_kernel<KP>: als_cg_kernel's shape -- one 256-thread workgroup per row, all steps in the one launch, the same pass (wave
// e mod 4 takes entry e, b_e in registers, butterfly dot: als_row_pass_accumulate of cmf_als_cg.hip.h; four wave accumulators added
// in wave order, then S x and l2 x), the same LDS residency classes (a class changes no bit), no atomics, vector stores only, no
// scratch.  The vector algebra runs in thread j < KP; the decisions every thread must take alike (any t_j < 0, free == free_old, the
// stop tests) come from values every thread reads the same bits of: sums combined through LDS in wave order, and __syncthreads_or
// of the flags.  The kernel's code object is the one it had before the pass was shared.
//
// Long rows (more than "als_cg_piece" entries) take the form of cmf_als_cg.hip.h's long rows, a state machine over launches:
//   als_cg_piece_kernel<KP>      that file's: one workgroup per piece, the partial sum of H x over the piece's entries to its own
//                                slot; x is max(f, 0) of the factor (stage 0, `clamp`), p (stage 1) or d (stage 2) from the row's
//                                state.  A piece of a row whose record's mode does not ask for this stage's pass (stopped, or a
//                                free step in stage 2) returns at once.
//   als_nncg_combine_kernel<KP>  one workgroup per long row: the partials added in piece order, S x and l2 x, then the algebra of
//                                the stage: 0 forms r and prepares the first step (free set, rho, p); 1 (A) takes the step if it
//                                is free and prepares the next, or leaves d as the next vector; 2 (B) finishes a projected step
//                                and prepares the next; the last B writes f and the passes the row ran.
// launches per sweep: 2 for r, then piece, A, piece, B per step.  The sums across workgroups are kernel boundaries.  The result of
// a long row depends on that row and on the piece length alone.
#pragma once
#include "cmf_als_cg.hip.h"

namespace cmfk {

struct AlsNncgArgs {
    AlsCgArgs a;            // as als_cg_kernel reads it
    int32_t *passes;        // passes row r ran go to passes[r - a.out_row0]
};

enum { ALS_NNCG_ROW_STOPPED = 0, ALS_NNCG_ROW_STEP = 1, ALS_NNCG_ROW_PROJECT = 2, ALS_NNCG_ROW_SKIP = 3 };
struct AlsNncgRow {         // a long row between launches
    float rho, rho_old;
    int32_t conj_ok;        // the step before was a free step: p may be continued
    int32_t mode;           // STOPPED | STEP: p is the next vector | PROJECT: d is | SKIP: p is, and stage 2 has nothing to do
    int32_t passes, pad;
};
struct AlsNncgLongArgs {
    AlsCgPieceArgs p;       // state: [long row][5][KP]: f, r, the next vector (p | d), f+, free_old (0 | 1); takes: the mode of info
    const float *S, *N;
    float *Fout;
    int64_t out_row0;
    AlsNncgRow *info;       // [long row]; p.takes points at the mode of the first record (the piece kernel only reads it): move both together
    int32_t *passes;        // as AlsNncgArgs
    float l2;
    int k;
    int stage;              // 0: r = g - H f; 1: the pass with p / combine A; 2: the pass with d / combine B
    int last;               // stage 2 of the last step: f and the passes go out
    const float *l2m;       // as AlsCgArgs
};

template <int KP, bool LR>
__global__ __launch_bounds__(256) void als_nncg_kernel(AlsNncgArgs ga) {
    constexpr int VPL = KP >= 64 ? KP / 64 : 1;     // floats of a gathered row per lane
    const AlsCgArgs &g = ga.a;
    extern __shared__ __attribute__((aligned(16))) float als_nncg_lds[];    // als_cg_kernel's layout
    float *xs = als_nncg_lds, *part = xs + KP, *wsum = part + 4 * KP, *res = wsum + 16;
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
        if (t == 0) ga.passes[row - g.out_row0] = 0;
        return;
    }
    const bool resident = n <= g.cap;
    float *resw = res + (int64_t)g.cap * KP;
    const int k = g.k;

    // one pass with the vector in xs: thread j < KP returns (H x)_j, or on the first pass (g - H x)_j without N
    auto pass = [&](auto first_c) -> float {
        constexpr bool first = decltype(first_c)::value;
        float xr[VPL], acc[VPL];
#pragma unroll
        for (int v = 0; v < VPL; ++v) {
            xr[v] = holds ? xs[lane * VPL + v] : 0.f;
            acc[v] = 0.f;
        }
        als_row_pass_accumulate<KP, first, VPL>(g.s0, g.s1, b0, b1, n0, 0, n, resident, res, resw, xr, acc, uw, lane, holds);
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
    // sums over the workgroup of va and vb (zero in threads >= KP), the same bits in every thread.  The two halves of wsum
    // alternate, so that one is rewritten only after a barrier has passed since its last read.
    int par = 0;
    auto dot2 = [&](float va, float vb, float &sb) -> float {
        va = als_cg_wave_sum(va);
        vb = als_cg_wave_sum(vb);
        float *ws = wsum + 8 * par;
        par ^= 1;
        if (lane == 0) {
            ws[uw] = va;
            ws[4 + uw] = vb;
        }
        __syncthreads();
        sb = ((ws[4] + ws[5]) + ws[6]) + ws[7];
        return ((ws[0] + ws[1]) + ws[2]) + ws[3];
    };

    float f = 0.f, r = 0.f, p = 0.f, rho_old = 0.f, unused;
    bool free_old = false, conj_ok = false;
    int passes = 1;
    if (t < KP) {
        f = fmaxf(g.Fin[row * KP + t], 0.f);
        xs[t] = f;
    }
    __syncthreads();
    r = pass(std::true_type());
    if (t < KP && g.N) r += g.N[row * KP + t];
    for (int s = 0; s < g.steps; ++s) {             // (a barrier of dot2 stands between every pass's reads of xs and the next write)
        const bool fr = t < KP && (f > 0.f || r > 0.f);
        const float z = fr ? r : 0.f;
        const float rho = dot2(z * z, 0.f, unused);
        if (!als_cg_positive_finite(rho)) break;     // the row keeps what it has
        const bool conj = !__syncthreads_or(fr != free_old) && conj_ok;
        p = conj ? fmaf(rho / rho_old, p, z) : z;
        if (t < KP) xs[t] = p;
        __syncthreads();
        const float q = pass(std::false_type());
        ++passes;
        float pr;
        const float pq = dot2(p * q, p * r, pr);
        if (!als_cg_positive_finite(pq)) break;
        const float alpha = pr / pq;
        const float tt = fmaf(alpha, p, f);
        if (!__syncthreads_or(tt < 0.f)) {           // the free step
            f = tt;
            r = fmaf(-alpha, q, r);
            rho_old = rho;
            free_old = fr;
            conj_ok = true;
            continue;
        }
        const float fp = fmaxf(tt, 0.f), d = fp - f; // the projected step
        if (t < KP) xs[t] = d;
        __syncthreads();
        const float hd = pass(std::false_type());
        ++passes;
        float dhd;
        const float dr = dot2(d * r, d * hd, dhd);
        if (!als_cg_positive_finite(dr) || !als_cg_positive_finite(dhd)) break;
        const float theta = dr / dhd;
        if (theta >= 1.f) {
            f = fp;
            r -= hd;
        } else {
            f = fmaxf(fmaf(theta, d, f), 0.f);
            r = fmaf(-theta, hd, r);
        }
        conj_ok = false;
    }
    if (t < k) out[t] = f;
    if (t == 0) ga.passes[row - g.out_row0] = passes;
}

// ------------------------------------------------------------------ long rows, cut into pieces (the piece kernel: als_cg_piece_kernel)
template <int KP, bool LR>
__global__ __launch_bounds__(256) void als_nncg_combine_kernel(AlsNncgLongArgs g) {
    __shared__ float xs[KP], wsum[16];
    const int t = threadIdx.x, lane = t & 63;
    const int uw = __builtin_amdgcn_readfirstlane(t >> 6);
    const int slot = blockIdx.x, k = g.k, stage = g.stage;
    const AlsCgLongRow lr = g.p.rows[slot];
    float *st = g.p.state + (int64_t)slot * 5 * KP;
    AlsNncgRow *info = g.info + slot;
    float *out = g.Fout + (lr.row - g.out_row0) * KP;
    AlsNncgRow in = AlsNncgRow{0.f, 0.f, 0, ALS_NNCG_ROW_STEP, 0, 0};
    if (stage != 0) in = *info;
    __syncthreads();                                     // every thread has read the row's record before thread 0 rewrites it
    auto finish = [&](float f, int passes) {             // the last launch of the sweep
        if (t < k) out[t] = f;
        if (t == 0) g.passes[lr.row - g.out_row0] = passes;
    };
    if (stage == 1 && in.mode != ALS_NNCG_ROW_STEP) return;
    if (stage == 2 && in.mode != ALS_NNCG_ROW_PROJECT) {
        if (t == 0 && in.mode == ALS_NNCG_ROW_SKIP) info->mode = ALS_NNCG_ROW_STEP;
        if (g.last) finish(t < KP ? st[t] : 0.f, in.passes);
        return;
    }
    float f = 0.f, r = 0.f, x = 0.f, fp = 0.f, o = 0.f;
    bool free_old = false;
    if (t < KP) {
        if (stage == 0) {
            f = fmaxf(g.p.Fin[lr.row * KP + t], 0.f);
            x = f;
        } else {
            f = st[t];
            r = st[KP + t];
            x = st[2 * KP + t];
            fp = st[3 * KP + t];
            free_old = st[4 * KP + t] != 0.f;
        }
        xs[t] = x;
    }
    __syncthreads();
    if (t < KP) o = als_long_row_product<KP, LR>(g.p, lr, g.S, xs, k, g.l2, g.l2m, stage == 0, t);
    const int passes = in.passes + 1;
    float rho_old = in.rho_old;
    bool conj_ok = in.conj_ok != 0;
    // f and r stand; the row stops where it is
    auto stop = [&]() {
        if (t == 0) {
            info->mode = ALS_NNCG_ROW_STOPPED;
            info->passes = passes;
        }
        if (g.last) finish(f, passes);
    };
    // the head of the next step from f, r (and p = x, free_old, rho_old, conj_ok of a free step): its free set, rho and p, to the state
    auto prepare = [&](int mode_alive) {
        const bool fr = t < KP && (f > 0.f || r > 0.f);
        const float z = fr ? r : 0.f;
        const float rho = als_wg_sum(wsum + 8, uw, lane, z * z);   // (the second half of wsum: a launch's step sum went through the first)
        const bool alive = als_cg_positive_finite(rho);
        const bool conj = !__syncthreads_or(fr != free_old) && conj_ok;
        const float p = conj ? fmaf(rho / rho_old, x, z) : z;
        if (t < KP) {
            st[t] = f;
            st[KP + t] = r;
            st[2 * KP + t] = p;
            st[4 * KP + t] = free_old ? 1.f : 0.f;
        }
        if (t == 0) *info = AlsNncgRow{rho, rho_old, conj_ok ? 1 : 0, alive ? mode_alive : ALS_NNCG_ROW_STOPPED, passes, 0};
    };
    if (stage == 0) {
        r = o;
        if (t < KP && g.N) r += g.N[lr.row * KP + t];
        x = 0.f;
        prepare(ALS_NNCG_ROW_STEP);
        return;
    }
    if (stage == 1) {                                    // combine A: x = p, o = q
        float pr;
        const float pq = als_wg_sum<true>(wsum, uw, lane, x * o, x * r, &pr);
        if (!als_cg_positive_finite(pq)) return stop();
        const float alpha = pr / pq;
        const float tt = fmaf(alpha, x, f);
        if (!__syncthreads_or(tt < 0.f)) {               // the free step; stage 2 has nothing to do
            free_old = t < KP && (f > 0.f || r > 0.f);
            f = tt;
            r = fmaf(-alpha, o, r);
            rho_old = in.rho;
            conj_ok = true;
            prepare(ALS_NNCG_ROW_SKIP);
            return;
        }
        fp = fmaxf(tt, 0.f);                             // the projected step: d is the next vector
        if (t < KP) {
            st[2 * KP + t] = fp - f;
            st[3 * KP + t] = fp;
        }
        if (t == 0) {
            info->mode = ALS_NNCG_ROW_PROJECT;
            info->passes = passes;
        }
        return;
    }
    float dhd;                                           // combine B: x = d, o = hd
    const float dr = als_wg_sum<true>(wsum, uw, lane, x * r, x * o, &dhd);
    if (!als_cg_positive_finite(dr) || !als_cg_positive_finite(dhd)) return stop();
    const float theta = dr / dhd;
    if (theta >= 1.f) {
        f = fp;
        r -= o;
    } else {
        f = fmaxf(fmaf(theta, x, f), 0.f);
        r = fmaf(-theta, o, r);
    }
    conj_ok = false;
    if (g.last) return finish(f, passes);
    prepare(ALS_NNCG_ROW_STEP);
}

} // namespace cmfk
