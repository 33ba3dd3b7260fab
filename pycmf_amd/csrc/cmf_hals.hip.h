// cmf_hals.hip.h -- HALS (hierarchical alternating least squares): cyclic coordinate descent on the non-negative Frobenius
// objective  1/2 |X - U V^T|^2 + 1/2 |Y - V Z^T|^2 + l1 sum(U, V, Z) + l2 / 2 (|U|^2 + |V|^2 + |Z|^2).
//
// One sweep of a factor F (rows x k) with numerator N (rows x k) and Gram G (k x k), every row f on its own:
//   for j = 0 .. k - 1:   h = G[j][j] + l2;  h == 0: f[j] stays
//                         f[j] <- max(0, f[j] - (sum_l f[l] G[l][j] + l2 f[j] - N[j] + l1) / h)       (l < j: already updated)
// which is sklearn's _update_coordinate_descent without shuffling (HHt + l2 I, XHt - l1, _update_cdnmf_fast with the identity
// permutation).  The recurrence is sequential in j inside a row only, so it is blocked like a triangular solve:
//
// hals_sweep_kernel<KP>: a 128-thread workgroup (two waves) owns HALS_ROWS = 64 rows of F -- wave w the rows 32 w .. 32 w + 31 --
// and keeps them current in LDS (row pitch KP + 2).  It walks the coordinates in blocks of 32:
//   1. the panel G[:, b] (k rows x 32 columns, row-major, 128 B per row) is staged in LDS for both waves;
//   2. each wave forms  D^T = G[o, b]^T F_w[:, o]^T  over the coordinates o OUTSIDE the block on v_mfma_f32_32x32x2_f32, the panel
//      as the A operand (ds_read_b32 of 32 consecutive floats per lane half), its rows of F as the B operand (one ds_read_b64 per
//      two instructions: lane l reads F[l & 31][4 t + 2 h], h = l >> 5, and pitch = 2 mod 64 puts the 32 rows of a lane half on 32 different bank pairs).  Lane l then holds, for row
//      l & 31, the 16 coordinates (r & 3) + 8 (r >> 2) + 4 h; they go through a 32 x 33 LDS tile so that
//   3. lane l < 32 owns row l of the wave with all 32 coordinates f[] and r[j] = N[j] - l1 - D[j] in registers (every index a
//      compile-time constant: two fully unrolled loops) and runs the 32 steps
//         dot = sum_{l in block} f_l G[l][j]  (the current f),   f_j <- max(0, f_j + ((r_j - dot) - l2 f_j) / h)
//      with a true division; column j of the diagonal block is read from the staged panel at wave-uniform addresses.
//      The block's own part of the sum is formed anew in every step instead of carrying r_j' -= delta G[j][j'] along: from a start
//      far from the minimiser most coordinates are clipped while the sums are still 100 x the values that survive, and a residual
//      updated 31 times keeps the roundings of that phase (measured on full steps: up to 2.0 x the tolerance of the tests, this form
//      at most 0.47 x);
//   4. the 32 new coordinates go back into the LDS image of F (the next block's product sees them) and to memory.
// rows k (k - 32) flops go to the fp32 matrix pipe, rows k 32 multiply-adds and rows k divisions stay on the vector units.
// A row's result depends on its own row of F and N and on G only: no atomics, nothing depends on the grid, a repeated sweep is
// bit-identical.  Coordinates >= k and rows >= rows are neither computed nor written: the padding of F stays zero.
#pragma once
#include "cmf_kernels.hip.h"

namespace cmfk {

enum { HALS_ROWS = 64, HALS_LDR = 33 };

struct HalsArgs {
    float *F;            // rows_pad x KP, updated in place
    const float *N;      // rows_pad x KP
    const float *G;      // KP x KP
    int64_t rows;
    int k;
    float l1, l2;
};

template <int KP>
struct HalsCfg {
    static constexpr int LDF = KP + 2;
    static constexpr size_t LDS_BYTES = (size_t)(HALS_ROWS * LDF + KP * 32 + HALS_ROWS * HALS_LDR) * sizeof(float);
};

template <int KP>
__global__ __launch_bounds__(128) void hals_sweep_kernel(HalsArgs a) {
    constexpr int LDF = HalsCfg<KP>::LDF;
    extern __shared__ f32x4 hals_lds[];
    float *Fs = reinterpret_cast<float *>(hals_lds);   // [HALS_ROWS][LDF]
    float *Ps = Fs + HALS_ROWS * LDF;                  // [k rows][32]: G[:, 32 b .. 32 b + 31]
    float *Rs = Ps + KP * 32;                          // [HALS_ROWS][HALS_LDR]: F G[:, b] of the owned rows without the block's own coordinates
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave * 32 + (lane & 31), h = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * HALS_ROWS;
    const int nb = (a.k + 31) >> 5, kc = nb * 32;      // coordinate blocks that hold a valid coordinate; kc <= KP
    const bool owner = h == 0 && row0 + wr < a.rows;

    for (int i = tid; i < HALS_ROWS * (kc / 2); i += 128) {
        const int r = i / (kc / 2), c2 = i - r * (kc / 2);
        *reinterpret_cast<f32x2 *>(Fs + r * LDF + 2 * c2) = *reinterpret_cast<const f32x2 *>(a.F + (row0 + r) * KP + 2 * c2);
    }
    for (int b = 0; b < nb; ++b) {
        __syncthreads();   // F staged (b = 0); the previous panel and tile are no longer read
        for (int i = tid; i < kc * 8; i += 128) {
            const int kk = i >> 3, q = i & 7;
            *reinterpret_cast<f32x4 *>(Ps + kk * 32 + 4 * q) = *reinterpret_cast<const f32x4 *>(a.G + (int64_t)kk * KP + b * 32 + 4 * q);
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        {
            const float *fp = Fs + wr * LDF + 2 * h;
            const float *pp = Ps + (2 * h) * 32 + (lane & 31);
            // instruction pair t: k = 4 t + 2 h and 4 t + 2 h + 1; the block's own coordinates (t = 8 b .. 8 b + 7) are left out
            for (int t = 0; t < 8 * b; ++t) {
                const f32x2 fv = *reinterpret_cast<const f32x2 *>(fp + 4 * t);
                const float g0 = pp[(4 * t) * 32], g1 = pp[(4 * t + 1) * 32];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g0, fv[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, fv[1], acc, 0, 0, 0);
            }
            for (int t = 8 * b + 8; t < kc / 4; ++t) {
                const f32x2 fv = *reinterpret_cast<const f32x2 *>(fp + 4 * t);
                const float g0 = pp[(4 * t) * 32], g1 = pp[(4 * t + 1) * 32];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g0, fv[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, fv[1], acc, 0, 0, 0);
            }
        }
        float *rp = Rs + wr * HALS_LDR;
#pragma unroll
        for (int i = 0; i < 16; ++i) rp[(i & 3) + 8 * (i >> 2) + 4 * h] = acc[i];
        __syncthreads();
        if (owner) {
            float f[32], r[32];
            const float *np = a.N + (row0 + wr) * KP + b * 32;
            float *fs = Fs + wr * LDF + b * 32;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(np + 4 * q);
                r[4 * q] = v[0]; r[4 * q + 1] = v[1]; r[4 * q + 2] = v[2]; r[4 * q + 3] = v[3];
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const f32x2 v = *reinterpret_cast<const f32x2 *>(fs + 2 * q);
                f[2 * q] = v[0]; f[2 * q + 1] = v[1];
            }
#pragma unroll
            for (int j = 0; j < 32; ++j) r[j] = (r[j] - a.l1) - rp[j];
            const float *gd = Ps + b * 32 * 32;             // G[32 b + l][32 b + j] at gd[32 l + j]: the same address in every lane
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                float dot = 0.f;                            // the block's own part of sum_l f[l] G[l][j], from the current f
#pragma unroll
                for (int l = 0; l < 32; ++l) dot = fmaf(f[l], gd[32 * l + j], dot);
                const float hd = gd[33 * j] + a.l2;
                const bool live = (b * 32 + j < a.k) && hd != 0.f;
                const float nw = fmaxf(0.f, f[j] + ((r[j] - dot) - a.l2 * f[j]) / hd);
                f[j] = live ? nw : f[j];
            }
            float *fg = a.F + (row0 + wr) * KP + b * 32;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                f32x2 v;
                v[0] = f[2 * q]; v[1] = f[2 * q + 1];
                *reinterpret_cast<f32x2 *>(fs + 2 * q) = v;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                f32x4 v;
                v[0] = f[4 * q]; v[1] = f[4 * q + 1]; v[2] = f[4 * q + 2]; v[3] = f[4 * q + 3];
                *reinterpret_cast<f32x4 *>(fg + 4 * q) = v;
            }
        }
    }
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx)
#ifdef CMF_HALS_HOST

// one sweep of factor `which` in place; N (frows_pad x k_pad) and G (k_pad x k_pad) on the device, zero beyond the valid extent
static int hals_sweep(cmf_ctx *c, int which, const float *N, const float *G, double l1, double l2) {
    const int64_t rows = c->frows[which];
    if (rows <= 0) return CMF_OK;
    HalsArgs a;
    a.F = c->F[which]; a.N = N; a.G = G; a.rows = rows; a.k = c->k; a.l1 = (float)l1; a.l2 = (float)l2;
    const dim3 grid((unsigned)((rows + HALS_ROWS - 1) / HALS_ROWS));
    Timed tm(c, CMF_K_HALS, 2.0 * (double)rows * c->k * c->k);
#define CMF_HALS_LAUNCH(KP_)                                                                                       \
    do {                                                                                                           \
        CHK(allow_big_lds(c, reinterpret_cast<const void *>(&hals_sweep_kernel<KP_>), (int)HalsCfg<KP_>::LDS_BYTES)); \
        hipLaunchKernelGGL((hals_sweep_kernel<KP_>), grid, dim3(128), HalsCfg<KP_>::LDS_BYTES, c->stream, a);      \
    } while (0)
    switch (c->kp) {
    case 32: CMF_HALS_LAUNCH(32); break;
    case 64: CMF_HALS_LAUNCH(64); break;
    case 128: CMF_HALS_LAUNCH(128); break;
    case 256: CMF_HALS_LAUNCH(256); break;
    default: return fail(CMF_EUNSUPPORTED, "HALS sweeps are built for n_components <= 256 (k_pad = %d)", c->kp);
    }
#undef CMF_HALS_LAUNCH
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// One HALS iteration in MU's sweep order V, U, Z (cmf_solvers.py:248-263), the new V used for U and Z.  Numerators and Grams are
// the products of an MU iteration, run whole into MU's own buffers: X^T U + Y Z | U^T U + Z^T Z into vbuf, V^T V into G2,
// X V and Y^T V into num.
extern "C" int cmf_hals_step(cmf_ctx *c, double l1, double l2, int mask) {
    NEED_PROBLEM(c);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_hals_step: n_components <= 256 only (k_pad = %d)", c->kp);
    if (mask <= 0 || mask > 7) return fail(CMF_EINVAL, "cmf_hals_step: update_mask must name at least one of U, V, Z (got %d)", mask);
    if (c->wm_kind[0] || c->wm_kind[1]) return fail(CMF_EUNSUPPORTED, "cmf_hals_step: per-entry weights are bound to this context and HALS has no weighted objective (cmf_clear_weight first)");
    DeviceGuard dg(c->device);
    if (mask & CMF_UPD_V) {
        CHK(cmf_mu_v_partials(c, c->vbuf));
        CHK(hals_sweep(c, CMF_V, c->vbuf, c->vbuf + c->dp * c->kp, l1, l2));
    }
    if (!(mask & (CMF_UPD_U | CMF_UPD_Z))) return CMF_OK;
    if ((mask & CMF_UPD_U) && !have_data(c, 0)) return fail(CMF_EINVAL, "X must be set before a U update");
    if ((mask & CMF_UPD_Z) && !have_data(c, 1)) return fail(CMF_EINVAL, "Y must be set before a Z update");
    CHK(gram32(c, c->F[CMF_V], c->dp, c->G2));
    if (mask & CMF_UPD_U) {
        CHK(data_times(c, 0, false, c->F[CMF_V], c->num));
        CHK(hals_sweep(c, CMF_U, c->num, c->G2, l1, l2));
    }
    if (mask & CMF_UPD_Z) {
        CHK(data_times(c, 1, true, c->F[CMF_V], c->num));
        CHK(hals_sweep(c, CMF_Z, c->num, c->G2, l1, l2));
    }
    return CMF_OK;
}

// test entry: one sweep of factor `which` with the caller's numerator and Gram
extern "C" int cmf_hals_sweep(cmf_ctx *c, int which, const double *N, const double *G, double l1, double l2) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2 || !N || !G) return fail(CMF_EINVAL, "cmf_hals_sweep: bad factor selector or null input");
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_hals_sweep: n_components <= 256 only (k_pad = %d)", c->kp);
    DeviceGuard dg(c->device);
    const int64_t rows = c->frows[which], rp = c->frows_pad[which];
    const int k = c->k, kp = c->kp;
    std::vector<float> host((size_t)rp * kp + (size_t)kp * kp, 0.f);
    for (int64_t i = 0; i < rows; ++i)
        for (int j = 0; j < k; ++j) host[(size_t)i * kp + j] = (float)N[i * k + j];
    float *hg = host.data() + (size_t)rp * kp;
    for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) hg[(size_t)i * kp + j] = (float)G[(size_t)i * k + j];
    CHK(ensure_scratch(c, c->hals_ws, host.size() * sizeof(float)));
    float *dev = (float *)c->hals_ws.p;
    HIPCHK(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const int rc = hals_sweep(c, which, dev, dev + (size_t)rp * kp, l1, l2);
    HIPCHK(hipStreamSynchronize(c->stream));   // `host` leaves scope
    return rc;
}

#endif // CMF_HALS_HOST
