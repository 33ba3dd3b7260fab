// cmf_rank.hip.h -- exact ranks of held-out entries under the order of cmf_topk, never forming the product (held-out evaluation).
//
// rank(i, j) = the number of candidates c != j of query i, not in i's exclusion list, that precede j in cmf_topk's order: larger
// raw float32 score first (-0 counts as +0), equal scores by smaller candidate index, a NaN-scored candidate absent.  Every score
// -- a held-out entry's own included -- is the fma chain of topk_scan_kernel: v_mfma_f32_32x32x2_f32 with the candidates as the A
// operand and the queries as the B operand, k = 8 c + j of lane half 0 paired with k = 8 c + 4 + j of half 1, c and j ascending.
// An element of an MFMA result depends on its own row of A and column of B only, so the bits of a score depend neither on the
// tile, nor on the candidate split, nor on what else shares the instruction: rank r < n <=> entry r of cmf_topk's list.
//
// rank_extract_kernel: the held-out entries' own scores.  A wave takes 32 entries, lane l & 31 loads entry t's candidate row as
//   row t of A and its query row as column t of B (global memory, no LDS) and keeps the diagonal of the 32 x 32 result: 32 times
//   the flops an entry needs, 64 held_nnz k in all -- against the 2 nq C k of a scan nothing.  (The issue's other route, a
//   second full scan that picks the marked scores out of the stream, costs a whole scan for the same bits.)
// rank_scan_kernel<KP>: the geometry of topk_scan_kernel, copied: 128 (virtual) queries per 256-thread workgroup, query rows in
//   KP / 2 registers per lane, candidates register-staged through 32 KB XOR-swizzled LDS tiles, lane l holds 16 scores of query
//   l & 31, the candidate stream cut into S shares (blockIdx.y).
//   * thresholds: a virtual query has up to RANK_HB held-out entries; their keys -- topk's 64-bit key: ordered score, inverted
//     candidate index -- lie in LDS position-major (thr[p][query]), the lanes l and l + 32 read the same word (broadcast).
//   * exclusion: per tile, lane l < 32 of a wave walks a cursor through the sorted exclusion list of query l (started at
//     lower_bound(c_begin), monotone afterwards, the next index waits in a register) and sets bits in one word per 32-candidate
//     sub-tile in LDS; candidates at or beyond the share's end are marked the same way.  A lane tests its 16 bits in registers:
//     a marked or NaN-scored candidate gets key 0, below every threshold, and so counts for nothing.
//   * counters: RANK_HB int32 per lane in registers, cnt[p] += key(candidate) > thr[p] -- one 64-bit compare and an add with
//     carry; j never precedes itself.  Thresholds beyond the longest list of the wave's 32 queries are skipped (wave-uniform).
//   * at the end the two lane halves of a query are added and cnt[share][query][p] is written.  No atomics of any kind.
// rank_finish_kernel: sums the shares (integers: any order gives the same bits) and scatters to the entries' places; an entry
//   whose own score is NaN gets -1.
// A row with more than RANK_HB held-out entries becomes several virtual queries with the same query row and exclusion list; the
// table is built on the host side of the call.  Rows without held-out entries are not scanned at all.
//
// No existing kernel is touched.  Reference counterpart: none.
#pragma once
#include "cmf_topk.hip.h"

namespace cmfk {

enum { RANK_HB = 16 };

struct RankArgs {
    const float *Q;          // query rows, pitch kp
    const int64_t *qrows;    // row of Q for query i (nullable: row i)
    const float *B;          // candidate rows, pitch kp, padded with zero rows to a multiple of 256
    int64_t C;               // valid candidates
    int64_t rows_per_split;  // multiple of 256
    const int32_t *vquery;   // virtual query -> query of the call
    const int64_t *vbeg;     // ... -> first of its held-out entries
    const int32_t *vcnt;     // ... -> how many (1 .. RANK_HB)
    int64_t nv;              // virtual queries of this launch
    const int32_t *hidx;     // held-out candidates, entry order
    const float *hscore;     // their scores (rank_extract_kernel)
    const int64_t *xptr;     // exclusion lists of the queries of the call (CSR, sorted; nullable)
    const int32_t *xidx;
    int32_t *cnt;            // [split][virtual query][RANK_HB]
};

__device__ __forceinline__ unsigned long long rank_key(float s, unsigned cand) {
    return ((unsigned long long)topk_ord(s) << 32) | (0xFFFFFFFFu - cand);
}

// 128 entries per 256-thread workgroup, 32 per wave
template <int KP>
__global__ __launch_bounds__(256) void rank_extract_kernel(const float *Q, const int64_t *qrows, const float *B, const int32_t *hq, const int32_t *hidx,
                                                           int64_t nnz, float *hscore) {
    constexpr int NCH = KP / 8;
    const int lane = threadIdx.x & 63, h = lane >> 5, t = lane & 31;
    const int64_t e = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 32 + t;
    const int64_t ee = e < nnz ? e : 0; // entries beyond the end compute on entry 0 and are never written
    const int64_t qi = hq[ee];
    const f32x4 *qsrc = (const f32x4 *)(Q + (qrows ? qrows[qi] : qi) * KP);
    const f32x4 *bsrc = (const f32x4 *)(B + (int64_t)hidx[ee] * KP);
    f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 4
    for (int c = 0; c < NCH; ++c) {
        const f32x4 a = bsrc[2 * c + h], b = qsrc[2 * c + h];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc, 0, 0, 0);
    }
    // register r of the lane: row (r & 3) + 8 (r >> 2) + 4 h, column t.  The diagonal (row t) sits in half (t >> 2) & 1
    const int rr = (t & 3) + 4 * (t >> 3);
    float s = acc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) s = rr == r ? acc[r] : s;
    if (e < nnz && h == ((t >> 2) & 1)) hscore[e] = s;
}

template <int KP>
__global__ __launch_bounds__(256, 2) void rank_scan_kernel(RankArgs g) {
    constexpr int CT = TOPK_TILE_FLOATS / KP;  // candidate rows per LDS tile (32 at KP = 256 ... 256 at KP = 32)
    constexpr int SLOTS = KP / 4;              // float4 slots per row
    constexpr int SW = (SLOTS < 16 ? SLOTS : 16) - 1; // slot ^ (row & SW): rows of one fragment read land on different banks
    constexpr int NCH = KP / 8;                // 8-deep k pieces: one float4 per lane half
    constexpr int NSUB = CT / 32;
    constexpr int KG = KP == 256 ? 4 : 8;      // scores turned into keys and compared at a time
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
    f32x4 *tile = (f32x4 *)topk_lds;                                                     // CT rows x SLOTS float4, swizzled
    unsigned long long *thr = (unsigned long long *)(topk_lds + TOPK_TILE_FLOATS * 4);   // [p][query]
    unsigned *bitmap = (unsigned *)(thr + RANK_HB * TOPK_QB);                            // [sub-tile][query]: bit b = candidate 32 sub + b skipped
    int *nheld = (int *)(bitmap + NSUB * TOPK_QB);                                       // [query]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int qcol = wave * 32 + (lane & 31);                 // query column of this lane inside the workgroup
    const int64_t v = (int64_t)blockIdx.x * TOPK_QB + qcol;   // virtual query of the launch
    const bool qvalid = v < g.nv;
    const int64_t qi = g.vquery[qvalid ? v : 0];              // beyond nv: compute on virtual query 0, never written

    // thresholds of this wave's queries (written and read by the same wave; the barrier below orders them anyway)
    if (h == 0) {
        const int nh = qvalid ? g.vcnt[v] : 0;
        const int64_t hb = qvalid ? g.vbeg[v] : 0;
        nheld[qcol] = nh;
        for (int p = 0; p < RANK_HB; ++p)
            thr[p * TOPK_QB + qcol] = p < nh ? rank_key(g.hscore[hb + p], (unsigned)g.hidx[hb + p]) : ~0ull;
    }
    __syncthreads();
    int nhmax = 0;
    for (int i = 0; i < 32; ++i) nhmax = max(nhmax, nheld[wave * 32 + i]);
    nhmax = __builtin_amdgcn_readfirstlane(nhmax);

    // the query row in registers: piece c = floats 8 c + 4 h .. + 3
    f32x4 qf[NCH];
    {
        const int64_t qrow = g.qrows ? g.qrows[qi] : qi;
        const f32x4 *src = (const f32x4 *)(g.Q + qrow * KP);
#pragma unroll
        for (int c = 0; c < NCH; ++c) qf[c] = src[2 * c + h];
    }

    const int64_t c_begin = (int64_t)blockIdx.y * g.rows_per_split;
    const int64_t c_end = min(c_begin + g.rows_per_split, g.C);
    const int ntiles = c_end > c_begin ? (int)((c_end - c_begin + CT - 1) / CT) : 0;

    // exclusion cursor (lanes 0 .. 31 of every wave): first entry of the list at or after c_begin; xnext = the candidate it names
    int64_t xcur = 0, xhi = 0;
    unsigned xnext = 0xFFFFFFFFu;
    if (h == 0 && qvalid && g.xptr) {
        int64_t lo = g.xptr[qi];
        xhi = g.xptr[qi + 1];
        int64_t hi = xhi;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)g.xidx[mid] < c_begin) lo = mid + 1;
            else hi = mid;
        }
        xcur = lo;
        if (xcur < xhi) xnext = (unsigned)g.xidx[xcur];
    }

    // staging: float4 number i * 256 + tid of the tile (8 per thread); a tile never leaves the 256-row block it starts in
    f32x4 st[8];
    auto fetch = [&](int t) {
        const f32x4 *src = (const f32x4 *)(g.B + (c_begin + (int64_t)t * CT) * KP);
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = src[i * 256 + tid];
    };
    if (ntiles > 0) fetch(0);

    int cnt[RANK_HB];
#pragma unroll
    for (int p = 0; p < RANK_HB; ++p) cnt[p] = 0;

    for (int t = 0; t < ntiles; ++t) {
        __syncthreads(); // tile t - 1 and its bitmap have been read by every wave
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int gidx = i * 256 + tid, row = gidx / SLOTS, slot = gidx % SLOTS;
            tile[row * SLOTS + (slot ^ (row & SW))] = st[i];
        }
        if (h == 0) { // the skipped candidates of this tile: beyond the share's end, or on the query's exclusion list
            const unsigned tb = (unsigned)(c_begin + (int64_t)t * CT), cend = (unsigned)c_end; // candidates < 2^31
            unsigned w[NSUB];
#pragma unroll
            for (int s = 0; s < NSUB; ++s) {
                const unsigned sb = tb + 32 * s;
                w[s] = sb >= cend ? 0xFFFFFFFFu : (cend - sb < 32 ? 0xFFFFFFFFu << (cend - sb) : 0u);
            }
            while (xnext < tb + CT) { // xnext >= tb: the cursor never falls behind the stream
                const unsigned off = xnext - tb;
#pragma unroll
                for (int s = 0; s < NSUB; ++s) w[s] |= (off >> 5) == (unsigned)s ? 1u << (off & 31) : 0u;
                ++xcur;
                xnext = xcur < xhi ? (unsigned)g.xidx[xcur] : 0xFFFFFFFFu;
            }
#pragma unroll
            for (int s = 0; s < NSUB; ++s) bitmap[s * TOPK_QB + qcol] = w[s];
        }
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1);

        for (int sub = 0; sub < NSUB; ++sub) {
            const int row = sub * 32 + (lane & 31);
            const f32x4 *arow = tile + row * SLOTS;
            const int sw = row & SW;
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const f32x4 a = arow[(2 * c + h) ^ sw];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], qf[c][0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], qf[c][1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], qf[c][2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], qf[c][3], acc, 0, 0, 0);
                if ((c & 3) == 3) __builtin_amdgcn_sched_barrier(0); // fragment reads at most four pieces ahead: the query rows need the registers
            }
            // register r of the lane: candidate row (r & 3) + 8 (r >> 2) + 4 h of the 32, query lane & 31
            const unsigned skip = bitmap[sub * TOPK_QB + qcol] >> (4 * h);
            const unsigned cbase = (unsigned)(c_begin + (int64_t)t * CT) + sub * 32 + 4 * h;
#pragma unroll
            for (int grp = 0; grp < 16 / KG; ++grp) { // KG scores at a time: sixteen 64-bit keys beside the query row do not fit the registers at KP = 256
                unsigned long long key[KG];
#pragma unroll
                for (int r8 = 0; r8 < KG; ++r8) {
                    const int r = KG * grp + r8, off = (r & 3) + 8 * (r >> 2);
                    const float s = acc[r];
                    const bool absent = ((skip >> off) & 1u) || s != s;
                    key[r8] = absent ? 0ull : rank_key(s, cbase + off);
                }
#pragma unroll
                for (int p = 0; p < RANK_HB; ++p) {
                    if (p < nhmax) {
                        const unsigned long long kt = thr[p * TOPK_QB + qcol];
#pragma unroll
                        for (int r8 = 0; r8 < KG; ++r8) cnt[p] += key[r8] > kt ? 1 : 0;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < RANK_HB; ++p) cnt[p] += __shfl_xor(cnt[p], 32);
    if (qvalid && h == 0) {
        int32_t *dst = g.cnt + ((int64_t)blockIdx.y * g.nv + v) * RANK_HB;
#pragma unroll
        for (int p = 0; p < RANK_HB; ++p) dst[p] = cnt[p];
    }
}

// one thread per (virtual query, place): the sum over the shares goes to the entry's place; a NaN-scored entry has no rank
__global__ __launch_bounds__(256) void rank_finish_kernel(const int32_t *cnt, int64_t nv, int nsplit, const int64_t *vbeg, const int32_t *vcnt,
                                                          const float *hscore, int32_t *rank) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t v = i / RANK_HB;
    const int p = (int)(i % RANK_HB);
    if (v >= nv || p >= vcnt[v]) return;
    int r = 0;
    for (int s = 0; s < nsplit; ++s) r += cnt[((int64_t)s * nv + v) * RANK_HB + p];
    const int64_t e = vbeg[v] + p;
    const float sc = hscore[e];
    rank[e] = sc != sc ? -1 : r;
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx)
#ifdef CMF_RANK_HOST

// tile + thresholds + bitmap words of the tile + list lengths: 53 KB at most, so two workgroups share a CU
static size_t rank_scan_lds(int kp) { return (size_t)TOPK_TILE_FLOATS * 4 + (size_t)RANK_HB * TOPK_QB * 8 + (size_t)(TOPK_TILE_FLOATS / kp / 32) * TOPK_QB * 4 + TOPK_QB * 4; }

struct RankPlan {
    int64_t nsplit = 1, rows_per_split = 256; // candidate shares (multiples of 256 rows)
    int64_t nv_bound = 0;                     // no call has more virtual queries than this
    int64_t chunk = 0;                        // virtual queries per scan launch
    size_t scratch = 0;                       // device bytes the call takes
};

// Scratch of one call, sized from nq, the two list lengths and the split S (nv = nq + held_nnz / RANK_HB bounds the virtual queries):
//   chunk * RANK_HB * 4 * S   counters of the shares        nv * 16   virtual-query table (query, first entry, count)
//   held_nnz * 16             entry -> query, candidate, score, rank
//   nq * 8                    query rows (cmf_rank with `rows`)          (nq + 1) * 8 + 4 * excl_nnz   exclusion lists
//   rup(nq, 128) * k_pad * 4  the uploaded query block of cmf_rank_queries
// chunk = nv unless the counters of all virtual queries would pass 256 MB (then a multiple of 128 that stays below it).  The
// shares are topk's: as many as fill the chip twice over (two workgroups per CU), or the option "topk_split".
static void rank_plan(const cmf_ctx *c, int64_t nq, int64_t C, int64_t held_nnz, bool have_rows, bool own_queries, int64_t excl_nnz, RankPlan &pl) {
    const int64_t blocks = (C + 255) / 256;
    pl.nv_bound = std::max<int64_t>(1, nq + held_nnz / RANK_HB);
    const int64_t nvb = (pl.nv_bound + TOPK_QB - 1) / TOPK_QB;
    const int64_t want = 2 * (int64_t)c->num_cu;
    int64_t S = c->opt_topk_split > 0 ? c->opt_topk_split : (want + nvb - 1) / nvb;
    S = std::max<int64_t>(1, std::min<int64_t>(S, std::min<int64_t>(blocks, TOPK_MERGE_MAX)));
    pl.rows_per_split = (blocks + S - 1) / S * 256;
    pl.nsplit = (blocks * 256 + pl.rows_per_split - 1) / pl.rows_per_split;
    const int64_t per_query = pl.nsplit * RANK_HB * 4;
    pl.chunk = std::min<int64_t>(pl.nv_bound, std::max<int64_t>(TOPK_QB, ((int64_t)256 << 20) / per_query / TOPK_QB * TOPK_QB));
    pl.scratch = (size_t)pl.chunk * per_query + (size_t)pl.nv_bound * 16 + (size_t)held_nnz * 16 + (have_rows ? (size_t)nq * 8 : 0) +
                 (excl_nnz >= 0 ? (size_t)(nq + 1) * 8 + (size_t)excl_nnz * 4 : 0) + (own_queries ? (size_t)rup(nq, TOPK_QB) * c->kp * 4 : 0);
}

static int rank_check_list(const char *what, int64_t nq, int64_t C, const int64_t *xp, const int32_t *xi) {
    if (xp[0] != 0) return fail(CMF_EINVAL, "rank: %s_indptr[0] must be 0", what);
    for (int64_t i = 0; i < nq; ++i) {
        if (xp[i + 1] < xp[i]) return fail(CMF_EINVAL, "rank: %s_indptr decreases at query %lld", what, (long long)i);
        if (xp[i + 1] > xp[i] && !xi) return fail(CMF_EINVAL, "rank: %s_indices is null but query %lld has entries", what, (long long)i);
        for (int64_t e = xp[i]; e < xp[i + 1]; ++e) {
            if (xi[e] < 0 || xi[e] >= C) return fail(CMF_EINVAL, "rank: %s index %d of query %lld is outside [0, %lld)", what, xi[e], (long long)i, (long long)C);
            if (e > xp[i] && xi[e] <= xi[e - 1]) return fail(CMF_EINVAL, "rank: the %s list of query %lld is not sorted (strictly ascending)", what, (long long)i);
        }
    }
    return CMF_OK;
}

static int rank_check_common(cmf_ctx *c, int cand, int64_t nq, const int64_t *hp, const int32_t *hi, const int64_t *xp, const int32_t *xi,
                             const int32_t *rank, const int32_t *eligible) {
    if (cand < 0 || cand > 2) return fail(CMF_EINVAL, "rank: bad candidate factor id %d", cand);
    if (nq < 0) return fail(CMF_EINVAL, "rank: negative query count");
    if (!rank || !eligible) return fail(CMF_EINVAL, "rank: rank and eligible must not be null");
    if (!hp) return fail(CMF_EINVAL, "rank: held_indptr must not be null");
    const int64_t C = c->frows[cand];
    if (C >= 0x7FFFFFFF) return fail(CMF_EUNSUPPORTED, "rank: candidate indices are int32");
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "rank: k_pad = %d (n_components above 256) is not supported", c->kp);
    if ((xp == nullptr) != (xi == nullptr)) return fail(CMF_EINVAL, "rank: excl_indptr and excl_indices go together (both or neither)");
    CHK(rank_check_list("held", nq, C, hp, hi));
    if (nq >= 0x7FFFFFFF) return fail(CMF_EUNSUPPORTED, "rank: query indices are int32");
    if (xp) CHK(rank_check_list("excl", nq, C, xp, xi));
    return CMF_OK;
}

template <typename T>
static int rank_upload(cmf_ctx *c, TopkBufs &bufs, T **dev, const T *host, size_t count) {
    CHK(bufs.get((void **)dev, count * sizeof(T)));
    if (count) HIPCHK(hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return CMF_OK;
}

// Q: query rows on the device (pitch k_pad); rows: host indices into Q for the nq queries, or null (query i = row i)
static int rank_run(cmf_ctx *c, const float *Q, const int64_t *rows, int64_t nq, int cand, const int64_t *hp, const int32_t *hi,
                    const int64_t *xp, const int32_t *xi, int32_t *rank, float *score, int32_t *eligible, TopkBufs &bufs, bool own_queries) {
    const int64_t C = c->frows[cand];
    for (int64_t i = 0; i < nq; ++i) eligible[i] = (int32_t)(C - (xp ? xp[i + 1] - xp[i] : 0));
    const int64_t nnz = hp[nq];
    if (nq == 0 || nnz == 0) return CMF_OK;
    RankPlan pl;
    rank_plan(c, nq, C, nnz, rows != nullptr, own_queries, xp ? xp[nq] : -1, pl);

    // the launch table: a row with h held-out entries is ceil(h / RANK_HB) virtual queries
    std::vector<int32_t> vquery, vcnt, hq((size_t)nnz);
    std::vector<int64_t> vbeg;
    for (int64_t i = 0; i < nq; ++i) {
        for (int64_t e = hp[i]; e < hp[i + 1]; ++e) hq[(size_t)e] = (int32_t)i;
        for (int64_t e = hp[i]; e < hp[i + 1]; e += RANK_HB) {
            vquery.push_back((int32_t)i);
            vbeg.push_back(e);
            vcnt.push_back((int32_t)std::min<int64_t>(RANK_HB, hp[i + 1] - e));
        }
    }
    const int64_t nv = (int64_t)vquery.size();

    int32_t *dvq = nullptr, *dvc = nullptr, *dhq = nullptr, *dhi = nullptr, *dxi = nullptr, *drank = nullptr, *dcnt = nullptr;
    int64_t *dvb = nullptr, *drows = nullptr, *dxp = nullptr;
    float *dscore = nullptr;
    CHK(rank_upload(c, bufs, &dvq, vquery.data(), (size_t)nv));
    CHK(rank_upload(c, bufs, &dvc, vcnt.data(), (size_t)nv));
    CHK(rank_upload(c, bufs, &dvb, vbeg.data(), (size_t)nv));
    CHK(rank_upload(c, bufs, &dhq, hq.data(), (size_t)nnz));
    CHK(rank_upload(c, bufs, &dhi, hi, (size_t)nnz));
    if (rows) CHK(rank_upload(c, bufs, &drows, rows, (size_t)nq));
    if (xp) {
        CHK(rank_upload(c, bufs, &dxp, xp, (size_t)nq + 1));
        CHK(rank_upload(c, bufs, &dxi, xi, (size_t)xp[nq]));
    }
    CHK(bufs.get((void **)&dscore, (size_t)nnz * 4));
    CHK(bufs.get((void **)&drank, (size_t)nnz * 4));
    const int64_t chunk = std::min(pl.chunk, nv);
    const size_t lds = rank_scan_lds(c->kp);
    {
        const void *scan = nullptr;
        switch (c->kp) {
        case 32: scan = (const void *)rank_scan_kernel<32>; break;
        case 64: scan = (const void *)rank_scan_kernel<64>; break;
        case 128: scan = (const void *)rank_scan_kernel<128>; break;
        default: scan = (const void *)rank_scan_kernel<256>; break;
        }
        CHK(allow_big_lds(c, scan, (int)lds));
    }
    CHK(bufs.get((void **)&dcnt, (size_t)chunk * pl.nsplit * RANK_HB * 4));

    for (int64_t v0 = 0; v0 < nv; v0 += chunk) {
        const int64_t nc = std::min(chunk, nv - v0);
        RankArgs a;
        a.Q = Q;
        a.qrows = drows;
        a.B = c->F[cand];
        a.C = C;
        a.rows_per_split = pl.rows_per_split;
        a.vquery = dvq + v0;
        a.vbeg = dvb + v0;
        a.vcnt = dvc + v0;
        a.nv = nc;
        a.hidx = dhi;
        a.hscore = dscore;
        a.xptr = dxp;
        a.xidx = dxi;
        a.cnt = dcnt;
        Timed tm(c, CMF_K_TOPK, 2.0 * (double)nc * (double)C * c->k);
        const dim3 egrid((unsigned)((nnz + 127) / 128)), grid((unsigned)((nc + TOPK_QB - 1) / TOPK_QB), (unsigned)pl.nsplit);
        const dim3 fgrid((unsigned)((nc * RANK_HB + 255) / 256));
        switch (c->kp) {
        case 32:
            if (v0 == 0) hipLaunchKernelGGL(rank_extract_kernel<32>, egrid, dim3(256), 0, c->stream, Q, (const int64_t *)drows, a.B, (const int32_t *)dhq, (const int32_t *)dhi, nnz, dscore);
            hipLaunchKernelGGL(rank_scan_kernel<32>, grid, dim3(256), lds, c->stream, a);
            break;
        case 64:
            if (v0 == 0) hipLaunchKernelGGL(rank_extract_kernel<64>, egrid, dim3(256), 0, c->stream, Q, (const int64_t *)drows, a.B, (const int32_t *)dhq, (const int32_t *)dhi, nnz, dscore);
            hipLaunchKernelGGL(rank_scan_kernel<64>, grid, dim3(256), lds, c->stream, a);
            break;
        case 128:
            if (v0 == 0) hipLaunchKernelGGL(rank_extract_kernel<128>, egrid, dim3(256), 0, c->stream, Q, (const int64_t *)drows, a.B, (const int32_t *)dhq, (const int32_t *)dhi, nnz, dscore);
            hipLaunchKernelGGL(rank_scan_kernel<128>, grid, dim3(256), lds, c->stream, a);
            break;
        default:
            if (v0 == 0) hipLaunchKernelGGL(rank_extract_kernel<256>, egrid, dim3(256), 0, c->stream, Q, (const int64_t *)drows, a.B, (const int32_t *)dhq, (const int32_t *)dhi, nnz, dscore);
            hipLaunchKernelGGL(rank_scan_kernel<256>, grid, dim3(256), lds, c->stream, a);
            break;
        }
        hipLaunchKernelGGL(rank_finish_kernel, fgrid, dim3(256), 0, c->stream, (const int32_t *)dcnt, nc, (int)pl.nsplit, (const int64_t *)a.vbeg, a.vcnt,
                           (const float *)dscore, drank);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(rank, drank, (size_t)nnz * 4, hipMemcpyDeviceToHost, c->stream));
    if (score) HIPCHK(hipMemcpyAsync(score, dscore, (size_t)nnz * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_rank(cmf_ctx *c, int query, int cand, const int64_t *rows, int64_t nq, const int64_t *held_indptr, const int32_t *held_indices,
                        const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *rank, float *score, int32_t *eligible) {
    NEED_PROBLEM(c);
    if (query < 0 || query > 2 || cand < 0 || cand > 2) return fail(CMF_EINVAL, "rank: bad factor id (query %d, candidates %d)", query, cand);
    if (!((query == CMF_U && cand == CMF_V) || (query == CMF_V && cand == CMF_U) || (query == CMF_V && cand == CMF_Z) || (query == CMF_Z && cand == CMF_V)))
        return fail(CMF_EINVAL, "rank: the model defines no product of %s and %s (X ~ f(U V^T): (U, V) / (V, U); Y ~ f(V Z^T): (V, Z) / (Z, V))",
                    topk_fname[query], topk_fname[cand]);
    if (!rows) nq = c->frows[query];
    CHK(rank_check_common(c, cand, nq, held_indptr, held_indices, excl_indptr, excl_indices, rank, eligible));
    if (rows)
        for (int64_t i = 0; i < nq; ++i)
            if (rows[i] < 0 || rows[i] >= c->frows[query])
                return fail(CMF_EINVAL, "rank: rows[%lld] = %lld is outside [0, %lld) of factor %s", (long long)i, (long long)rows[i], (long long)c->frows[query], topk_fname[query]);
    DeviceGuard dg(c->device);
    TopkBufs bufs(c);
    return rank_run(c, c->F[query], rows, nq, cand, held_indptr, held_indices, excl_indptr, excl_indices, rank, score, eligible, bufs, false);
}

extern "C" int cmf_rank_queries(cmf_ctx *c, const double *Q, int64_t rs, int64_t cs, int64_t nq, int cand, const int64_t *held_indptr, const int32_t *held_indices,
                                const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *rank, float *score, int32_t *eligible) {
    NEED_PROBLEM(c);
    if (!Q && nq > 0) return fail(CMF_EINVAL, "rank: null query matrix");
    CHK(rank_check_common(c, cand, nq, held_indptr, held_indices, excl_indptr, excl_indices, rank, eligible));
    if (nq == 0) return CMF_OK;
    DeviceGuard dg(c->device);
    TopkBufs bufs(c);
    float *dq = nullptr;
    const size_t qbytes = (size_t)rup(nq, TOPK_QB) * c->kp * sizeof(float);
    CHK(bufs.get((void **)&dq, qbytes));
    HIPCHK(hipMemsetAsync(dq, 0, qbytes, c->stream));
    CHK(upload_strided<double>(c, dq, c->kp, nq, c->k, Q, rs, cs));
    return rank_run(c, dq, nullptr, nq, cand, held_indptr, held_indices, excl_indptr, excl_indices, rank, score, eligible, bufs, true);
}

extern "C" int cmf_rank_layout(cmf_ctx *c, int64_t nq, int cand, int64_t held_nnz, int64_t excl_nnz, int own_queries, int64_t *out4) {
    NEED_PROBLEM(c);
    if (cand < 0 || cand > 2 || !out4 || nq < 1 || held_nnz < 0) return fail(CMF_EINVAL, "rank layout: bad argument");
    RankPlan pl;
    rank_plan(c, nq, c->frows[cand], held_nnz, false, own_queries != 0, excl_nnz, pl);
    out4[0] = RANK_HB;
    out4[1] = pl.nsplit;
    out4[2] = pl.chunk;
    out4[3] = (int64_t)pl.scratch;
    return CMF_OK;
}
#endif // CMF_RANK_HOST
