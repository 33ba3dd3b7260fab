// cmf_topk.hip.h -- top-n of a link-transformed factor product f(Q B^T), never materialised (prediction from fitted factors).
//
// topk_scan_kernel: one 256-thread workgroup (4 waves, one per SIMD) owns TOPK_QB = 128 queries -- wave w the 32 queries
// 32 w .. 32 w + 31, their float32 rows resident in KP / 2 registers per lane -- and one share of the candidates, which it
// streams through LDS in tiles of 8192 / KP rows (32 KB; register-staged, so the loads of tile t + 1 travel under the MFMAs of
// tile t).  Scores come from v_mfma_f32_32x32x2_f32 with the CANDIDATES as the A operand (accumulator rows = registers) and the
// QUERIES as the B operand (accumulator columns = lanes): lane l of a wave holds 16 scores of ONE query, query l & 31 -- the
// lanes l and l + 32 share it -- and filters them in registers against that query's threshold, the worst entry of its list.
//   * the list of a query is a binary min-heap of n 64-bit keys in LDS (position-major: heap[p][query]); a key packs the
//     score and the candidate so that ONE unsigned compare is the order relation of the result: larger raw float32 score
//     first (-0 counts as +0), equal scores: smaller candidate index first.  Unfilled places hold a sentinel below every
//     real key.  Only a score that passes the float compare with the threshold builds its key; only a key above the heap's
//     root is looked up in the query's exclusion list (binary search, global memory) and then replaces the root.
//   * a list is touched by one wave only, by its two half-waves one after the other (structured control flow of one wave: LDS
//     operations of a wave complete in order), so there is no lock and no atomic.
//   * every score is one fma chain over k in an order fixed by this file alone (float4 pieces: k = 8 c + j of lane half 0 with
//     k = 8 c + 4 + j of half 1, c and j ascending): it depends neither on the tile, nor on the candidate split, nor on the
//     other queries of the call.  The top n of a set under a total order is unique, so the result is too.
//   * a NaN score never passes the filter: such a candidate is treated as absent.
// topk_merge_kernel: one workgroup per query sorts the n S keys of the S candidate shares (bitonic, LDS) and writes the first n
// as (index, f(score)); sentinels come out as (-1, -inf).  It also runs for S = 1 (a heap is not sorted).
//
// No existing kernel is touched.  Reference counterpart: none on the device -- the reference's only consumer of the factors is
// the host argsort of pycmf/analysis.py:3-16.
#pragma once
#include "cmf_kernels.hip.h"

namespace cmfk {

enum { TOPK_QB = 128, TOPK_TILE_FLOATS = 8192, TOPK_MERGE_MAX = 8192 };

// worst possible key: score -inf, candidate 0x7fffffff (no real candidate has that index)
#define CMF_TOPK_SENTINEL 0x007FFFFF80000000ull

struct TopkArgs {
    const float *Q;          // query rows, pitch kp
    const int64_t *qrows;    // row of Q for query i (nullable: row i)
    int64_t nq;              // queries of this launch
    const float *B;          // candidate rows, pitch kp, padded with zero rows to a multiple of 256
    int64_t C;               // valid candidates
    int64_t rows_per_split;  // multiple of 256
    int n;
    const int64_t *xptr;     // exclusion lists of the queries of this launch (CSR, sorted; nullable)
    const int32_t *xidx;
    unsigned long long *part; // [split][query][n]
};

__device__ __forceinline__ unsigned topk_ord(float s) {
    if (s == 0.0f) s = 0.0f; // -0 ranks as +0
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float topk_unord(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// key (> root) replaces the root of the min-heap whose column starts at `heap` and sinks to its place
__device__ __forceinline__ void topk_heap_replace(unsigned long long *heap, int n, unsigned long long key) {
    int i = 0;
    for (;;) {
        const int l = 2 * i + 1;
        if (l >= n) break;
        const unsigned long long kl = heap[l * TOPK_QB];
        const unsigned long long kr = l + 1 < n ? heap[(l + 1) * TOPK_QB] : ~0ull;
        const bool left = kl <= kr;
        const unsigned long long kc = left ? kl : kr;
        if (kc >= key) break;
        heap[i * TOPK_QB] = kc;
        i = left ? l : l + 1;
    }
    heap[i * TOPK_QB] = key;
}

__device__ __forceinline__ bool topk_excluded(const int32_t *xi, int64_t lo, int64_t hi, int32_t cand) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int32_t v = xi[mid];
        if (v == cand) return true;
        if (v < cand) lo = mid + 1;
        else hi = mid;
    }
    return false;
}

template <int KP>
__global__ __launch_bounds__(256, 2) void topk_scan_kernel(TopkArgs g) {
    constexpr int CT = TOPK_TILE_FLOATS / KP;  // candidate rows per LDS tile (32 at KP = 256 ... 256 at KP = 32)
    constexpr int SLOTS = KP / 4;              // float4 slots per row
    constexpr int SW = (SLOTS < 16 ? SLOTS : 16) - 1; // slot ^ (row & SW): rows of one fragment read land on different banks
    constexpr int NCH = KP / 8;                // 8-deep k pieces: one float4 per lane half
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
    f32x4 *tile = (f32x4 *)topk_lds;                                             // CT rows x SLOTS float4, swizzled
    unsigned long long *heaps = (unsigned long long *)(topk_lds + TOPK_TILE_FLOATS * 4); // [n][TOPK_QB]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int qcol = wave * 32 + (lane & 31);                 // query column of this lane inside the workgroup
    const int64_t q = (int64_t)blockIdx.x * TOPK_QB + qcol;   // query of the launch
    const bool qvalid = q < g.nq;
    const int n = g.n;

    for (int i = tid; i < n * TOPK_QB; i += 256) heaps[i] = CMF_TOPK_SENTINEL;
    __syncthreads();

    // the query row in registers: piece c = floats 8 c + 4 h .. + 3 (queries beyond nq compute on query 0's row and are never written)
    f32x4 qf[NCH];
    {
        const int64_t qq = qvalid ? q : 0;
        const int64_t qrow = g.qrows ? g.qrows[qq] : qq;
        const f32x4 *src = (const f32x4 *)(g.Q + qrow * KP);
#pragma unroll
        for (int c = 0; c < NCH; ++c) qf[c] = src[2 * c + h];
    }
    int64_t xlo = 0, xhi = 0;
    if (qvalid && g.xptr) { xlo = g.xptr[q]; xhi = g.xptr[q + 1]; }

    const int64_t c_begin = (int64_t)blockIdx.y * g.rows_per_split;
    const int64_t c_end = min(c_begin + g.rows_per_split, g.C);
    const int ntiles = c_end > c_begin ? (int)((c_end - c_begin + CT - 1) / CT) : 0;

    // staging: float4 number i * 256 + tid of the tile (8 per thread); a tile never leaves the 256-row block it starts in
    f32x4 st[8];
    auto fetch = [&](int t) {
        const f32x4 *src = (const f32x4 *)(g.B + (c_begin + (int64_t)t * CT) * KP);
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = src[i * 256 + tid];
    };
    if (ntiles > 0) fetch(0);

    unsigned long long *myheap = heaps + qcol;
    float thr = -INFINITY; // score of the root as last seen: never above the root's, so the filter never drops a winner

    for (int t = 0; t < ntiles; ++t) {
        __syncthreads(); // tile t - 1 has been read by every wave
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int gidx = i * 256 + tid, row = gidx / SLOTS, slot = gidx % SLOTS;
            tile[row * SLOTS + (slot ^ (row & SW))] = st[i];
        }
        __syncthreads();
        if (t + 1 < ntiles) fetch(t + 1);

        for (int sub = 0; sub < CT / 32; ++sub) {
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
            bool pass = false;
#pragma unroll
            for (int r = 0; r < 16; ++r) pass |= acc[r] >= thr;
            pass = pass && qvalid;
            if (__any(pass)) {
                const unsigned cbase = (unsigned)(c_begin + (int64_t)t * CT) + sub * 32 + 4 * h, cend = (unsigned)c_end; // candidates < 2^31
                for (int hh = 0; hh < 2; ++hh) {
                    if (h == hh && pass) {
                        unsigned long long root = myheap[0];
                        unsigned todo = 0; // the registers whose score reaches the threshold (one copy of the list code, not sixteen)
#pragma unroll
                        for (int r = 0; r < 16; ++r) todo |= (acc[r] >= thr ? 1u : 0u) << r;
                        while (todo) {
                            const int rr = __builtin_ctz(todo);
                            todo &= todo - 1;
                            float s = acc[0];
#pragma unroll
                            for (int r = 1; r < 16; ++r) s = rr == r ? acc[r] : s;
                            const unsigned cand = cbase + (rr & 3) + 8 * (rr >> 2);
                            if (cand < cend) {
                                const unsigned long long key = ((unsigned long long)topk_ord(s) << 32) | (0xFFFFFFFFu - cand);
                                if (key > root && !topk_excluded(g.xidx, xlo, xhi, (int32_t)cand)) {
                                    topk_heap_replace(myheap, n, key);
                                    root = myheap[0];
                                }
                            }
                        }
                        thr = topk_unord((unsigned)(root >> 32));
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (qvalid && h == 0) {
        unsigned long long *dst = g.part + ((int64_t)blockIdx.y * g.nq + q) * n;
        for (int p = 0; p < n; ++p) dst[p] = myheap[p * TOPK_QB];
    }
}

// one workgroup per query: the n * nsplit keys of its shares, sorted (descending) in LDS; the first n leave as (index, f(score))
__global__ __launch_bounds__(256) void topk_merge_kernel(const unsigned long long *part, int64_t nq, int n, int nsplit, int P, int link,
                                                         int32_t *idx, float *val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
    unsigned long long *key = (unsigned long long *)topk_lds;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x, total = n * nsplit;
    for (int e = tid; e < P; e += nt) key[e] = e < total ? part[((int64_t)(e / n) * nq + q) * n + e % n] : 0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = tid; e < P; e += nt) {
                const int o = e ^ j;
                if (o > e) {
                    const unsigned long long a = key[e], b = key[o];
                    const bool desc = (e & k) == 0;
                    if (desc ? a < b : a > b) { key[e] = b; key[o] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < n; e += nt) {
        const unsigned long long kk = key[e];
        const bool real = kk > CMF_TOPK_SENTINEL;
        const float s = topk_unord((unsigned)(kk >> 32));
        idx[q * n + e] = real ? (int32_t)(0xFFFFFFFFu - (unsigned)kk) : -1;
        val[q * n + e] = real ? (link ? sigmoidf_(s) : s) : -INFINITY;
    }
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_ctx)
#ifdef CMF_TOPK_HOST

struct TopkPlan {
    int64_t nsplit = 1, rows_per_split = 256; // candidate shares (multiples of 256 rows)
    int64_t chunk = 0;                        // queries per launch pair
    int P = 1, merge_threads = 64;            // bitonic length / workgroup of the merge
    size_t scan_lds = 0;
    size_t scratch = 0;                       // device bytes the call takes (all buffers of one chunk)
};

// Scratch of one call, all of it sized from nq, n and the split S:
//   chunk * n * 8 * S   partial lists        chunk * n * 8   (index, value) images of the result
//   chunk * 8           query rows (cmf_topk with `rows`)     (chunk + 1) * 8 + 4 * nnz   exclusion lists of the chunk
//   rup(nq, 128) * k_pad * 4   the uploaded query block of cmf_topk_queries
// chunk = nq unless the partial lists of all queries would pass 256 MB (then a multiple of 128 queries that stays below it).
static void topk_plan(const cmf_ctx *c, int64_t nq, int64_t C, int n, bool have_rows, bool own_queries, int64_t excl_nnz, TopkPlan &pl) {
    const int64_t blocks = (C + 255) / 256, nqb = (nq + TOPK_QB - 1) / TOPK_QB;
    pl.scan_lds = (size_t)TOPK_TILE_FLOATS * 4 + (size_t)n * TOPK_QB * 8;
    // as many shares as fill the chip once: two workgroups per CU while their LDS fits twice (n <= 48), else one.  Not more: every
    // share fills a list of its own, n (1 + ln(C / (S n))) insertions per query, so the list work grows with S
    const int64_t want = (2 * pl.scan_lds <= 160 * 1024 ? 2 : 1) * (int64_t)c->num_cu;
    int64_t S = c->opt_topk_split > 0 ? c->opt_topk_split : (want + nqb - 1) / std::max<int64_t>(nqb, 1);
    S = std::max<int64_t>(1, std::min<int64_t>(S, std::min<int64_t>(blocks, TOPK_MERGE_MAX / n)));
    pl.rows_per_split = (blocks + S - 1) / S * 256;
    pl.nsplit = (blocks * 256 + pl.rows_per_split - 1) / pl.rows_per_split;
    const int64_t per_query = pl.nsplit * n * 8;
    pl.chunk = std::min<int64_t>(nq, std::max<int64_t>(TOPK_QB, ((int64_t)256 << 20) / per_query / TOPK_QB * TOPK_QB));
    pl.P = 1;
    while (pl.P < pl.nsplit * n) pl.P <<= 1;
    pl.merge_threads = pl.P <= 512 ? 64 : 256;
    pl.scratch = (size_t)pl.chunk * n * 8 * (pl.nsplit + 1) + (have_rows ? (size_t)pl.chunk * 8 : 0) +
                 (excl_nnz >= 0 ? (size_t)(pl.chunk + 1) * 8 + (size_t)excl_nnz * 4 : 0) +
                 (own_queries ? (size_t)rup(nq, TOPK_QB) * c->kp * 4 : 0);
}

static int topk_check_common(cmf_ctx *c, int cand, int link, int64_t nq, int n, const int64_t *xp, const int32_t *xi, const int32_t *idx, const float *val) {
    if (cand < 0 || cand > 2) return fail(CMF_EINVAL, "top-n: bad candidate factor id %d", cand);
    if (link != CMF_LINK_LINEAR && link != CMF_LINK_LOGIT) return fail(CMF_EINVAL, "top-n: link must be CMF_LINK_LINEAR or CMF_LINK_LOGIT");
    if (nq < 0) return fail(CMF_EINVAL, "top-n: negative query count");
    if (!idx || !val) return fail(CMF_EINVAL, "top-n: idx and val must not be null");
    const int64_t C = c->frows[cand];
    if (n < 1) return fail(CMF_EINVAL, "top-n: n must be at least 1 (got %d)", n);
    if (n > CMF_TOPK_MAX_N) return fail(CMF_EINVAL, "top-n: n = %d exceeds CMF_TOPK_MAX_N = %d", n, CMF_TOPK_MAX_N);
    if (n > C) return fail(CMF_EINVAL, "top-n: n = %d exceeds the %lld candidates", n, (long long)C);
    if (C >= 0x7FFFFFFF) return fail(CMF_EUNSUPPORTED, "top-n: candidate indices are int32");
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "top-n: k_pad = %d (n_components above 256) is not supported", c->kp);
    if ((xp == nullptr) != (xi == nullptr)) return fail(CMF_EINVAL, "top-n: excl_indptr and excl_indices go together (both or neither)");
    if (xp) {
        if (xp[0] != 0) return fail(CMF_EINVAL, "top-n: excl_indptr[0] must be 0");
        for (int64_t i = 0; i < nq; ++i) {
            if (xp[i + 1] < xp[i]) return fail(CMF_EINVAL, "top-n: excl_indptr decreases at query %lld", (long long)i);
            for (int64_t e = xp[i]; e < xp[i + 1]; ++e) {
                if (xi[e] < 0 || xi[e] >= C) return fail(CMF_EINVAL, "top-n: excluded index %d of query %lld is outside [0, %lld)", xi[e], (long long)i, (long long)C);
                if (e > xp[i] && xi[e] <= xi[e - 1]) return fail(CMF_EINVAL, "top-n: the exclusion list of query %lld is not sorted (strictly ascending)", (long long)i);
            }
        }
    }
    return CMF_OK;
}

struct TopkBufs { // scratch of one call: context allocator, released when the call returns
    cmf_ctx *c;
    std::vector<void *> p;
    explicit TopkBufs(cmf_ctx *c_) : c(c_) {}
    int get(void **out, size_t bytes) {
        CHK(dev_alloc(c, out, bytes, false));
        p.push_back(*out);
        return CMF_OK;
    }
    ~TopkBufs() {
        if (!p.empty()) (void)hipStreamSynchronize(c->stream);
        for (void *q : p) dev_free(c, q);
    }
};

// Q: query rows on the device (pitch k_pad); rows: host indices into Q for the nq queries, or null (query i = row i)
static int topk_run(cmf_ctx *c, const float *Q, const int64_t *rows, int64_t nq, int cand, int link, int n, const int64_t *xp, const int32_t *xi,
                    int32_t *idx, float *val, TopkBufs &bufs, bool own_queries) {
    if (nq == 0) return CMF_OK;
    const int64_t C = c->frows[cand];
    TopkPlan pl;
    topk_plan(c, nq, C, n, rows != nullptr, own_queries, xp ? xp[nq] : -1, pl);
    static_assert((size_t)TOPK_TILE_FLOATS * 4 + (size_t)CMF_TOPK_MAX_N * TOPK_QB * 8 <= 160 * 1024, "tile + lists of the largest n must fit the 160 KB of LDS of a gfx950 CU");
    const void *scan = nullptr;
    switch (c->kp) {
    case 32: scan = (const void *)topk_scan_kernel<32>; break;
    case 64: scan = (const void *)topk_scan_kernel<64>; break;
    case 128: scan = (const void *)topk_scan_kernel<128>; break;
    default: scan = (const void *)topk_scan_kernel<256>; break;
    }
    if (pl.scan_lds > 48 * 1024) CHK(allow_big_lds(c, scan, (int)pl.scan_lds));
    if ((size_t)pl.P * 8 > 48 * 1024) CHK(allow_big_lds(c, (const void *)topk_merge_kernel, pl.P * 8));

    unsigned long long *part = nullptr;
    int32_t *didx = nullptr, *dxi = nullptr;
    float *dval = nullptr;
    int64_t *drows = nullptr, *dxp = nullptr;
    CHK(bufs.get((void **)&part, (size_t)pl.chunk * n * 8 * pl.nsplit));
    CHK(bufs.get((void **)&didx, (size_t)pl.chunk * n * 4));
    CHK(bufs.get((void **)&dval, (size_t)pl.chunk * n * 4));
    if (rows) CHK(bufs.get((void **)&drows, (size_t)pl.chunk * 8));
    std::vector<int64_t> xp_local;
    if (xp) { // room for the longest chunk's lists
        int64_t nnz_max = 1;
        for (int64_t q0 = 0; q0 < nq; q0 += pl.chunk) nnz_max = std::max(nnz_max, xp[std::min(nq, q0 + pl.chunk)] - xp[q0]);
        CHK(bufs.get((void **)&dxp, (size_t)(pl.chunk + 1) * 8));
        CHK(bufs.get((void **)&dxi, (size_t)nnz_max * 4));
    }
    for (int64_t q0 = 0; q0 < nq; q0 += pl.chunk) {
        const int64_t nc = std::min(pl.chunk, nq - q0);
        if (rows) HIPCHK(hipMemcpyAsync(drows, rows + q0, (size_t)nc * 8, hipMemcpyHostToDevice, c->stream));
        if (xp) { // the lists of this chunk only, offsets from 0
            const int64_t e0 = xp[q0], nnz = xp[q0 + nc] - e0;
            xp_local.resize(nc + 1);
            for (int64_t i = 0; i <= nc; ++i) xp_local[i] = xp[q0 + i] - e0;
            HIPCHK(hipMemcpyAsync(dxp, xp_local.data(), (size_t)(nc + 1) * 8, hipMemcpyHostToDevice, c->stream));
            if (nnz) HIPCHK(hipMemcpyAsync(dxi, xi + e0, (size_t)nnz * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream)); // xp_local is reused by the next chunk
        }
        TopkArgs a;
        a.Q = Q;
        a.qrows = rows ? drows : nullptr;
        if (!rows && q0) a.Q = Q + q0 * c->kp;
        a.nq = nc;
        a.B = c->F[cand];
        a.C = C;
        a.rows_per_split = pl.rows_per_split;
        a.n = n;
        a.xptr = dxp;
        a.xidx = dxi;
        a.part = part;
        {
            Timed tm(c, CMF_K_TOPK, 2.0 * (double)nc * (double)C * c->k);
            const dim3 grid((unsigned)((nc + TOPK_QB - 1) / TOPK_QB), (unsigned)pl.nsplit);
            switch (c->kp) {
            case 32: hipLaunchKernelGGL(topk_scan_kernel<32>, grid, dim3(256), pl.scan_lds, c->stream, a); break;
            case 64: hipLaunchKernelGGL(topk_scan_kernel<64>, grid, dim3(256), pl.scan_lds, c->stream, a); break;
            case 128: hipLaunchKernelGGL(topk_scan_kernel<128>, grid, dim3(256), pl.scan_lds, c->stream, a); break;
            default: hipLaunchKernelGGL(topk_scan_kernel<256>, grid, dim3(256), pl.scan_lds, c->stream, a); break;
            }
            hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)nc), dim3(pl.merge_threads), (size_t)pl.P * 8, c->stream,
                               (const unsigned long long *)part, nc, n, (int)pl.nsplit, pl.P, link, didx, dval);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(idx + q0 * n, didx, (size_t)nc * n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(val + q0 * n, dval, (size_t)nc * n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return CMF_OK;
}

static const char *const topk_fname[3] = {"U", "V", "Z"};

extern "C" int cmf_topk(cmf_ctx *c, int query, int cand, int link, const int64_t *rows, int64_t nq, int n,
                        const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *idx, float *val) {
    NEED_PROBLEM(c);
    if (query < 0 || query > 2 || cand < 0 || cand > 2) return fail(CMF_EINVAL, "top-n: bad factor id (query %d, candidates %d)", query, cand);
    if (!((query == CMF_U && cand == CMF_V) || (query == CMF_V && cand == CMF_U) || (query == CMF_V && cand == CMF_Z) || (query == CMF_Z && cand == CMF_V)))
        return fail(CMF_EINVAL, "top-n: the model defines no product of %s and %s (X ~ f(U V^T): (U, V) / (V, U); Y ~ f(V Z^T): (V, Z) / (Z, V))",
                    topk_fname[query], topk_fname[cand]);
    if (!rows) nq = c->frows[query];
    CHK(topk_check_common(c, cand, link, nq, n, excl_indptr, excl_indices, idx, val));
    if (rows)
        for (int64_t i = 0; i < nq; ++i)
            if (rows[i] < 0 || rows[i] >= c->frows[query])
                return fail(CMF_EINVAL, "top-n: rows[%lld] = %lld is outside [0, %lld) of factor %s", (long long)i, (long long)rows[i], (long long)c->frows[query], topk_fname[query]);
    DeviceGuard dg(c->device);
    TopkBufs bufs(c);
    return topk_run(c, c->F[query], rows, nq, cand, link, n, excl_indptr, excl_indices, idx, val, bufs, false);
}

extern "C" int cmf_topk_queries(cmf_ctx *c, const double *Q, int64_t rs, int64_t cs, int64_t nq, int cand, int link, int n,
                                const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *idx, float *val) {
    NEED_PROBLEM(c);
    if (!Q && nq > 0) return fail(CMF_EINVAL, "top-n: null query matrix");
    CHK(topk_check_common(c, cand, link, nq, n, excl_indptr, excl_indices, idx, val));
    if (nq == 0) return CMF_OK;
    DeviceGuard dg(c->device);
    TopkBufs bufs(c);
    float *dq = nullptr;
    const size_t qbytes = (size_t)rup(nq, TOPK_QB) * c->kp * sizeof(float);
    CHK(bufs.get((void **)&dq, qbytes));
    HIPCHK(hipMemsetAsync(dq, 0, qbytes, c->stream));
    CHK(upload_strided<double>(c, dq, c->kp, nq, c->k, Q, rs, cs));
    return topk_run(c, dq, nullptr, nq, cand, link, n, excl_indptr, excl_indices, idx, val, bufs, true);
}

extern "C" int cmf_topk_layout(cmf_ctx *c, int64_t nq, int cand, int n, int64_t excl_nnz, int own_queries, int64_t *out4) {
    NEED_PROBLEM(c);
    if (cand < 0 || cand > 2 || !out4 || nq < 1 || n < 1 || n > CMF_TOPK_MAX_N || n > c->frows[cand]) return fail(CMF_EINVAL, "top-n layout: bad argument");
    TopkPlan pl;
    topk_plan(c, nq, c->frows[cand], n, false, own_queries != 0, excl_nnz, pl);
    out4[0] = TOPK_QB;
    out4[1] = pl.nsplit;
    out4[2] = pl.chunk;
    out4[3] = (int64_t)pl.scratch;
    return CMF_OK;
}
#endif // CMF_TOPK_HOST
