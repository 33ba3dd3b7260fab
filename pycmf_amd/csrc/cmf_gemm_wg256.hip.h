// cmf_gemm_wg256.hip.h -- the data passes (ROLE 0, BN = 256, fp32 MFMA) on a 256-thread workgroup.
//
// gemm_kernel (cmf_kernels.hip.h) runs eight waves, two per SIMD, each on a 64 x 128 wave tile with 128 accumulator
// registers.  Here ONE wave per SIMD owns a 128 x 128 wave tile (4 x 4 blocks of v_mfma_f32_32x32x2_f32, 256 accumulator
// registers of the 512 a lane has at this occupancy): one 16-byte A fragment and one 16-byte B fragment feed 16 MFMAs
// instead of 8 + 16 bytes feeding 8, so a K-step reads 128 KB of fragments from LDS instead of 192 KB.
//   NN : X stays in LDS in gemm_kernel's k-contiguous padded image (lanes of an MFMA operand index ROWS of X there).
//   TN : X never enters LDS.  Lane (l31, lh) of wave (wm, wn) needs X[k0 + 2 s + lh][row0 + 128 wm + 4 l31 .. + 3] for
//        k-pair s: one 16-byte global load (two coalesced 512-byte runs per wave instruction) whose four values are the A
//        operands of the wave's four M blocks -- block i owns rows 4 r + i, as the N side owns columns 4 c + j.  Sixteen
//        such loads per lane and K-step form a 64-register ring that is refilled one K-step ahead; LDS holds the factor tile
//        only (32 KB per stage), so the fill of a K-step is 32 wave-level ds_write_b128 instead of 64.
//   FREG : the factor leaves LDS as well.  The B fragment of a group is four consecutive floats of ONE row of the row-major
//        factor [k][256] -- row k0 + 2 s + lh (TN), row k0 + 8 q + 4 lh + e (NN) -- at columns n0 + 128 wn + 4 l31 .. + 3: the
//        access pattern of the X ring.  A second 16-slot ring holds it.  The TN form then has no LDS, no barrier and nothing its
//        four waves share; the NN form keeps X's image (72 KB for both stages), its staging and the barrier.  The slots of
//        group s - 1 are refilled inside group s, one load behind one MFMA, and every global load of these forms is a buffer
//        load whose address is scalar arithmetic (below).
// Accumulation order is gemm_kernel's, element by element: TN group s consumes k = 2 s + lh, NN group 4 q + e consumes
// k = 8 q + 4 lh + e, split-K slabs are cut at the same places -- the output is bit-identical to gemm_kernel's.
// The K loop is ONE basic block: every staging load is issued unconditionally from a clamped address (the last steps fetch
// their own tile again and write it to the idle LDS stage), because a conditional refill makes hipcc close each K-step
// with s_waitcnt vmcnt(0), i.e. wait for loads issued a few hundred cycles earlier.
#pragma once
#include "cmf_kernels.hip.h"

namespace cmfk {

template <int MODE, bool FREG>
struct Wg256Cfg {
    static_assert(MODE == MODE_NN || MODE == MODE_TN, "data passes: NN and TN");
    static constexpr int BM = 256, BN = 256, BK = 32, PADK = BK + 4, NT = 256;
    static constexpr int A_ELEMS = (MODE == MODE_NN) ? BM * PADK : 0;
    static constexpr int B_ELEMS = FREG ? 0 : BK * BN;
    static constexpr int STAGE = A_ELEMS + B_ELEMS;
    static constexpr int LD = BK * BN / 4 / NT; // 16-byte pieces of a 256 x 32 tile per thread (8)
    static constexpr size_t LDS_BYTES = 2 * STAGE * sizeof(float); // TN with FREG: none
};

template <int MODE, bool FREG>
__global__ __launch_bounds__(256) void gemm_wg256_kernel(GemmArgs g) {
    using C = Wg256Cfg<MODE, FREG>;
    constexpr bool NN = (MODE == MODE_NN);
    constexpr bool LDS = C::LDS_BYTES != 0; // the K-step stages something through LDS and ends in a barrier
    constexpr int NGRP = C::BK / 2;
    constexpr int XREG_MI = 5, FREG_MI = 10; // FREG: the MFMAs of a group behind which the two rings are refilled
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int t = threadIdx.x;
    const int lane = t & 63, wid = t >> 6;
    const int l31 = lane & 31, lh = lane >> 5;
    const int wrow0 = 128 * (wid >> 1), wcol0 = 128 * (wid & 1);

    const int64_t row0 = (int64_t)blockIdx.x * C::BM;
    const int64_t n0 = (int64_t)blockIdx.y * C::BN;
    const int64_t kbeg = (int64_t)blockIdx.z * g.klen;
    int64_t kend = kbeg + g.klen;
    if (kend > g.Kred) kend = g.Kred;
    const int nkt = (int)((kend - kbeg) / C::BK);
    const int64_t klast = kend - C::BK; // staging loads past the last tile fetch the last tile again

    f32x16 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int64_t wg_linear = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (g.dbg && t == 0) {
        g.dbg[4 * wg_linear + 0] = __builtin_amdgcn_s_memtime();
        g.dbg[4 * wg_linear + 1] = __builtin_amdgcn_s_memrealtime();
    }

    // staging: piece p of thread t is 16-byte chunk t + 256 p of the tile.  Factor tile [k][256]: row (t >> 6) + 4 p, chunk lane.
    // X tile of the NN form [row][k]: row (t >> 3) + 32 p, chunk t & 7.
    f32x4 rb[FREG ? 1 : C::LD], ra[NN ? C::LD : 1];
    f32x4 xr[NN ? 1 : NGRP];   // TN: the X ring, xr[s] = this lane's A operands of k-pair s
    f32x4 br[FREG ? NGRP : 1]; // FREG: the factor ring, br[s] = this lane's B operands of group s
    const float *Bg = g.B + (int64_t)wid * g.ldb + n0 + 4 * lane;
    const float *Ag = NN ? g.A + (row0 + (t >> 3)) * g.lda + 4 * (t & 7) : g.A + (int64_t)lh * g.lda + row0 + wrow0 + 4 * l31;
    // FREG: every global load of the K loop is a buffer load -- a descriptor at the tile's origin (wave-uniform: kernel arguments,
    // blockIdx, the loop counter), the piece's rows as a scalar offset, the lane's part as a 32-bit byte offset (the host keeps the
    // row pitches below 2^21 floats): a load is scalar arithmetic and one instruction.  With flat addresses each load brought a
    // 64-bit vector add into the MFMA stream, and that add, not the load, was what the matrix pipe waited for (profiles/HISTORY.md
    // section 13).  The addresses are in range by construction; the descriptor's bound is left open
    const char *Xu = reinterpret_cast<const char *>(NN ? g.A + row0 * g.lda : g.A + row0), *Fu = reinterpret_cast<const char *>(g.B + n0);
    auto buf_load = [&](const char *origin, int rows_bytes, uint32_t lane_off) {
        const __amdgpu_buffer_rsrc_t d = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(origin), 0, -1, 0x00020000);
        return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(d, lane_off, rows_bytes, 0));
    };
    const uint32_t x_off = (uint32_t)(4 * (NN ? (t >> 3) * (int)g.lda + 4 * (t & 7) : lh * (int)g.lda + wrow0 + 4 * l31));
    const uint32_t f_off = (uint32_t)(4 * ((NN ? 4 * lh : lh) * (int)g.ldb + wcol0 + 4 * l31));
    const int b_lds = wid * C::BN + 4 * lane, a_lds = (t >> 3) * C::PADK + 4 * (t & 7);

    auto gload_b = [&](int64_t k0, int p) { rb[p] = *reinterpret_cast<const f32x4 *>(Bg + (k0 + 4 * p) * g.ldb); };
    auto lstore_b = [&](float *Bs, int p) { *reinterpret_cast<f32x4 *>(Bs + b_lds + 4 * p * C::BN) = rb[p]; };
    auto gload_a = [&](int64_t k0, int p) { ra[p] = *reinterpret_cast<const f32x4 *>(Ag + 32 * p * g.lda + k0); };
    auto lstore_a = [&](float *As, int p) { *reinterpret_cast<f32x4 *>(As + a_lds + 32 * p * C::PADK) = ra[p]; };
    auto gload_x = [&](int64_t k0, int s) { xr[s] = *reinterpret_cast<const f32x4 *>(Ag + (k0 + 2 * s) * g.lda); };
    auto gload_xu = [&](int64_t k0, int s) { xr[s] = buf_load(Xu + k0 * g.lda * 4, 2 * s * (int)g.lda * 4, x_off); };
    auto gload_au = [&](int64_t k0, int p) { ra[p] = buf_load(Xu + k0 * 4, 32 * p * (int)g.lda * 4, x_off); };
    auto gload_f = [&](int64_t k0, int s) {
        br[s] = buf_load(Fu + k0 * g.ldb * 4, (NN ? 8 * (s >> 2) + (s & 3) : 2 * s) * (int)g.ldb * 4, f_off);
    };

    // (the host cuts split-K slabs so that every workgroup has at least one K-step; leaving here keeps the accumulators out of a
    // join with the zero state, which would move all 256 of them through ordinary registers behind the loop)
    if (nkt <= 0) return;
    {
        const int64_t k1 = kbeg + C::BK < klast ? kbeg + C::BK : klast; // tile 1 waits in registers
        if constexpr (!FREG) {
            float *As0 = smem, *Bs0 = smem + C::A_ELEMS;
#pragma unroll
            for (int p = 0; p < C::LD; ++p) {
                gload_b(kbeg, p);
                if constexpr (NN) gload_a(kbeg, p);
            }
#pragma unroll
            for (int p = 0; p < C::LD; ++p) {
                lstore_b(Bs0, p);
                if constexpr (NN) lstore_a(As0, p);
            }
#pragma unroll
            for (int p = 0; p < C::LD; ++p) {
                gload_b(k1, p);
                if constexpr (NN) gload_a(k1, p);
            }
            // the ring LAST, as in the steady state (staging loads of a K-step are older than its ring refills): the waits hipcc
            // counts for the loop are the stricter of entry and back edge
            if constexpr (!NN)
#pragma unroll
                for (int s = 0; s < NGRP; ++s) gload_x(kbeg, s);
        } else if constexpr (NN) {
            // the steady state's order again, pinned (in any other hipcc opens every K-step with vmcnt(0)): the X pieces of tile 1
            // with slot 0 of the ring behind the fifth, then slots 1 .. 14; slot 15 is filled by the first K-step's group 0
#pragma unroll
            for (int p = 0; p < C::LD; ++p) gload_au(kbeg, p);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < C::LD; ++p) lstore_a(smem, p);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < C::LD; ++p) {
                gload_au(k1, p);
                __builtin_amdgcn_sched_barrier(0);
                if (p == FREG_MI / 2 - 1) {
                    gload_f(kbeg, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int s = 1; s < NGRP - 1; ++s) {
                gload_f(kbeg, s);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            // x0, b0, x1, b1, ... x14, b14 as the loop refills them, pinned; slot 15 is filled by the first K-step's group 0
#pragma unroll
            for (int s = 0; s < NGRP - 1; ++s) {
                gload_xu(kbeg, s);
                __builtin_amdgcn_sched_barrier(0);
                gload_f(kbeg, s);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if constexpr (LDS) __syncthreads();
        for (int kt = 0; kt < nkt; ++kt) {
            const float *As = smem + (kt & 1) * C::STAGE, *Bs = As + C::A_ELEMS;
            float *nAs = smem + ((kt + 1) & 1) * C::STAGE, *nBs = nAs + C::A_ELEMS;
            int64_t kn1 = kbeg + (int64_t)(kt + 1) * C::BK, kn2 = kn1 + C::BK;
            kn1 = kn1 < klast ? kn1 : klast;
            kn2 = kn2 < klast ? kn2 : klast;
            // One K-step = 16 MFMA groups (k-pairs) of 16 MFMAs.  The wave is alone on its SIMD, so everything else is issued
            // BETWEEN the MFMAs of a group, one piece behind one MFMA: the LDS writes of tile t+1 and behind them the global loads
            // of tile t+2 into the registers just drained (TN: 8 + 8 pieces, all in group 0; NN: 16 writes in group 0, 16 loads
            // in group 1; NN with FREG: 8 writes, 8 loads), the fragment reads of group s+1 at the head of group s, and (TN without
            // FREG) the X slot of group s refilled with tile t+1 behind the group's last MFMA.  sched_barrier(0) pins that order.
            f32x4 a[NN ? 2 : 1][4], b[2];
            auto ldb_frag = [&](int sidx) {
                const int kk = NN ? 8 * (sidx >> 2) + 4 * lh + (sidx & 3) : 2 * sidx + lh;
                b[sidx & 1] = *reinterpret_cast<const f32x4 *>(Bs + kk * C::BN + wcol0 + 4 * l31);
            };
            auto lda_frag = [&](int q) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    a[q & 1][i] = *reinterpret_cast<const f32x4 *>(As + (wrow0 + 32 * i + l31) * C::PADK + 4 * (2 * q + lh));
            };
            if constexpr (NN) lda_frag(0);
            if constexpr (!FREG) ldb_frag(0);
#pragma unroll
            for (int sidx = 0; sidx < NGRP; ++sidx) {
                const int q = sidx >> 2, e = sidx & 3;
                if (sidx + 1 < NGRP) {
                    if constexpr (!FREG) ldb_frag(sidx + 1);
                    if constexpr (NN)
                        if (e == 0 && q + 1 < NGRP / 4) lda_frag(q + 1);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mi = 0; mi < 16; ++mi) {
                    const int i = mi >> 2, j = mi & 3;
                    const float av = NN ? a[q & 1][i][e] : xr[sidx][i];
                    const float bv = FREG ? br[sidx][j] : b[sidx & 1][j];
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i][j], 0, 0, 0);
                    if constexpr (NN && FREG) {
                        // X alone: 8 writes in group 0, 8 loads in group 1, each behind every other MFMA
                        if (sidx == 0 && (mi & 1)) lstore_a(nAs, mi >> 1);
                        if (sidx == 1 && (mi & 1)) gload_au(kn2, mi >> 1);
                    } else if constexpr (NN) {
                        // 8 + 8 pieces: writes in group 0, loads in group 1
                        const int p = mi >> 1;
                        if (sidx == 0) {
                            if (mi & 1) lstore_b(nBs, p);
                            else lstore_a(nAs, p);
                        } else if (sidx == 1) {
                            if (mi & 1) gload_b(kn2, p);
                            else gload_a(kn2, p);
                        }
                    } else if constexpr (!FREG) {
                        if (sidx == 0 && mi < C::LD) lstore_b(nBs, mi);
                        if (sidx == 0 && mi >= C::LD) gload_b(kn2, mi - C::LD);
                    }
                    if constexpr (FREG) {
                        // the ring: a slot is free behind its group's last MFMA, and one load fits behind one MFMA -- so the slots
                        // of group s - 1 are refilled with tile t+1 inside group s, group 0 fetching THIS tile's slot 15
                        const int rs = (sidx + NGRP - 1) % NGRP;
                        const int64_t kr = sidx == 0 ? kbeg + (int64_t)kt * C::BK : kn1;
                        if (!NN && mi == XREG_MI) gload_xu(kr, rs);
                        if (mi == FREG_MI) gload_f(kr, rs);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (!NN && !FREG) {
                    gload_x(kn1, sidx);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (LDS) __syncthreads();
        }
    }

    if (g.dbg && t == 0) {
        g.dbg[4 * wg_linear + 2] = __builtin_amdgcn_s_memtime();
        g.dbg[4 * wg_linear + 3] = __builtin_amdgcn_s_memrealtime();
    }
    // epilogue: direct store, accumulate into red_out, or this split's slab (X and Y are padded to 256 rows and columns: no guards)
    const bool in_red = g.red_out != nullptr;
    // this lane's origin; every element is then a wave-uniform row offset away
    float *Cl = (in_red ? g.red_out : g.C + (int64_t)blockIdx.z * g.slab_stride) +
                (row0 + wrow0 + (NN ? 4 : 16) * lh) * g.ldc + n0 + wcol0 + 4 * l31;
    const int ldc = (int)g.ldc;
    auto rowoff = [&](int i, int r) -> int {
        const int rr = (r & 3) + 8 * (r >> 2);
        return (NN ? 32 * i + rr : 4 * rr + i) * ldc;
    };
    if (in_red && g.red_acc) { // out += acc: the sixteen old values of a block row are fetched together
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j])); // block row i leaves the accumulator registers here, not before
            f32x4 old[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) old[r] = *reinterpret_cast<const f32x4 *>(Cl + rowoff(i, r));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                f32x4 v = {acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
                v += old[r];
                *reinterpret_cast<f32x4 *>(Cl + rowoff(i, r)) = v;
            }
            __builtin_amdgcn_sched_barrier(0); // one block row at a time: all 256 accumulators moved out at once would spill
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j])); // block row i leaves the accumulator registers here, not before
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f32x4 v = {acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
                *reinterpret_cast<f32x4 *>(Cl + rowoff(i, r)) = v;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

} // namespace cmfk
