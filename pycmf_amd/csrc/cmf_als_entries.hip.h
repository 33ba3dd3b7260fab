// cmf_als_entries.hip.h -- the entry passes of the ALS solver: what every kernel that walks the stored entries of one row PIECE of a
// CSR image shares (the bias sweep, cmf_als_bias.hip.h; the logistic loss, cmf_als_logit.hip.h; the Huber and logistic reweighting
// passes and the Huber loss, cmf_als_reweight.hip.h).  One 256-thread workgroup per piece of at most L consecutive stored entries of
// one row; GL = k_pad / 4 lanes hold one factor row, a float4 per lane (the lane layout of wmu_res_csr_kernel); the 256 / GL lane
// groups deal the piece's entries among themselves round-robin.  No group ever walks a whole long row.
//   als_entry_walk<GL, NF>(args, body)  the walk: the row a in registers, NF gathered rows in flight per lane group.  Per round, in
//                          this order: the NF entry numbers e = base + grp + j NG and their clamped twins q = min(e, len - 1); the
//                          NF gathers of B[idx]; body.load(j, q, column) for the body's own scalar loads, which so stay in flight
//                          with the gathers; the NF scores s = a . b in float32 in the fixed order of group_sum; body.use(j, s, e,
//                          real).  e and q count from the piece's first entry: body.begin(beg), once per piece, is where a body
//                          moves its pointers there (a position in the image per load instead is a 64-bit add per load, and the
//                          Huber pass measured 1.8 % slower with it).  Every group runs the same number of rounds: an entry past
//                          the piece's end reads the piece's last entry again and is not `real` (the body neither stores nor adds
//                          it), so the lanes of a wave stay together through group_sum.  Group grp meets the entries e = grp (mod
//                          NG) in ascending e whatever NF is: NF changes how many loads are in flight and no sum.
//   als_group_reduce<GL, N>  N doubles per lane group through red[N][NG] in LDS; thread 0 adds the groups in group order
//   als_piece_sum_kernel   the pieces' doubles in piece order, one thread: the cross-workgroup sum of a loss, a kernel boundary
// No atomics, no grid-wide barrier, vector stores only: a repeated call from the same state is bit-identical.
#pragma once
#include "cmf_kernels.hip.h"

namespace cmfk {

struct AlsEntryPiece {
    int64_t beg;   // first stored entry
    int32_t len;   // 1 .. L
    int32_t row;   // of the image
};

// what the walk reads; the argument record of every entry kernel extends it
struct AlsEntryArgs {
    const AlsEntryPiece *pieces;
    const int32_t *idx;
    const float *A, *B;      // the factor of the image's rows, the gathered factor; pitch kp
    int kp;
};

template <int GL, int NF, class Body>
__device__ __forceinline__ void als_entry_walk(const AlsEntryArgs &g, Body &body) {
#pragma clang fp contract(off)
    constexpr int NG = 256 / GL;
    const AlsEntryPiece pc = g.pieces[blockIdx.x];
    const int gl = threadIdx.x % GL, grp = threadIdx.x / GL;
    const f32x4 a = *reinterpret_cast<const f32x4 *>(g.A + (int64_t)pc.row * g.kp + 4 * gl);
    const int32_t *idx = g.idx + pc.beg;
    body.begin(pc.beg);
    for (int base = 0; base < pc.len; base += NF * NG) {
        int e[NF], q[NF];
        int32_t col[NF];
        f32x4 b[NF];
        float s[NF];
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            e[j] = base + grp + j * NG;
            q[j] = min(e[j], pc.len - 1);
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            col[j] = idx[q[j]];
            b[j] = *reinterpret_cast<const f32x4 *>(g.B + (int64_t)col[j] * g.kp + 4 * gl);
        }
#pragma unroll
        for (int j = 0; j < NF; ++j) body.load(j, q[j], col[j]);
#pragma unroll
        for (int j = 0; j < NF; ++j) s[j] = group_sum<GL>(a[0] * b[j][0] + a[1] * b[j][1] + a[2] * b[j][2] + a[3] * b[j][3]);
#pragma unroll
        for (int j = 0; j < NF; ++j) body.use(j, s[j], e[j], e[j] < pc.len);
    }
}

// v[n] of every lane group (its first lane holds it) summed over the groups in group order into out[n], by thread 0
template <int GL, int N>
__device__ __forceinline__ void als_group_reduce(const double (&v)[N], double *out) {
    constexpr int NG = 256 / GL;
    __shared__ double red[N][NG];
    const int gl = threadIdx.x % GL, grp = threadIdx.x / GL;
    if (gl == 0)
        for (int n = 0; n < N; ++n) red[n][grp] = v[n];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int n = 0; n < N; ++n) {
            double x = red[n][0];
            for (int q = 1; q < NG; ++q) x += red[n][q];
            out[n] = x;
        }
}

__global__ void als_piece_sum_kernel(const double *part, int64_t n, double *out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double v = 0.0;
    for (int64_t p = 0; p < n; ++p) v += part[p];
    *out = v;
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als.hip.h)
#ifdef CMF_ALS_HOST
enum { ALS_ENTRY_PIECE = 2048 };   // the piece of the reweighting passes and of the losses (the bias sweep has an option: als_bias_piece)

// The piece list of one image from its row lengths (the pattern lives on the device only): rows cut into pieces of at most L stored
// entries, in an allocation of its own.  what: the caller's name in the message.  first_dev: non-null for first[row] .. first[row + 1],
// the pieces of every row, beside the list.  Synchronises: the host vectors may go.
static int als_image_pieces(cmf_ctx *c, const WCsrDev &M, int64_t L, const char *what, cmfk::AlsEntryPiece **pieces_dev, int64_t *npieces,
                            int64_t **first_dev) {
    std::vector<int64_t> ip((size_t)M.rows + 1, 0);
    HIPCHK(hipMemcpyAsync(ip.data(), M.indptr, ip.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<cmfk::AlsEntryPiece> pieces;
    const std::vector<int64_t> first = als_cut_rows(&ip, 1, M.rows, L, [&](int64_t r, int, int64_t beg, int32_t len) {
        pieces.push_back(cmfk::AlsEntryPiece{beg, len, (int32_t)r});
    });
    if ((int64_t)pieces.size() > INT32_MAX)
        return fail(CMF_EUNSUPPORTED, "%s: more than 2^31 - 1 pieces%s", what, first_dev ? " (als_bias_piece too small)" : "");
    CHK(dev_alloc(c, (void **)pieces_dev, std::max<size_t>(16, pieces.size() * sizeof(cmfk::AlsEntryPiece)), false));
    if (!pieces.empty()) HIPCHK(hipMemcpyAsync(*pieces_dev, pieces.data(), pieces.size() * sizeof(cmfk::AlsEntryPiece), hipMemcpyHostToDevice, c->stream));
    if (first_dev) {
        CHK(dev_alloc(c, (void **)first_dev, first.size() * sizeof(int64_t), false));
        HIPCHK(hipMemcpyAsync(*first_dev, first.data(), first.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    *npieces = (int64_t)pieces.size();
    return CMF_OK;
}

// The pieces of ALS_ENTRY_PIECE entries of image t of relation `which`, built at the first pass or loss over a bound pattern and
// kept with the reweighting state (AlsReweight; als_reweight_free drops them with the weights): the reweighting passes and both
// losses walk the same lists.
static int als_entry_pieces(cmf_ctx *c, int which, int t, const char *what) {
    AlsReweight &h = c->als_reweight[which];
    if (h.pieces[t]) return CMF_OK;
    return als_image_pieces(c, c->wm_sp[which][t], ALS_ENTRY_PIECE, what, &h.pieces[t], &h.npieces[t], nullptr);
}

// the factor of the rows (fa) and the gathered factor (fb) of image t (0 the pattern, 1 its transpose) of relation `which`
static void als_image_factors(int which, int t, int *fa, int *fb) {
    const int rows = which == 0 ? CMF_U : CMF_V, cols = which == 0 ? CMF_V : CMF_Z;
    *fa = t == 0 ? rows : cols;
    *fb = t == 0 ? cols : rows;
}

// what the walk reads of image t of relation `which` at the current factors, over the piece list `pieces`
static void als_entry_args(const cmf_ctx *c, int which, int t, const cmfk::AlsEntryPiece *pieces, cmfk::AlsEntryArgs &a) {
    int fa, fb;
    als_image_factors(which, t, &fa, &fb);
    a.pieces = pieces;
    a.idx = c->wm_sp[which][t].idx;
    a.A = c->F[fa];
    a.B = c->F[fb];
    a.kp = c->kp;
}

// The tail of a loss over np > 0 pieces of an image of nnz entries: launch(part) starts the kernel that writes one double per piece
// into part[np]; the pieces are added in piece order behind it and the sum comes back into *out.
template <class Launch>
static int als_pieces_loss(cmf_ctx *c, int64_t np, int64_t nnz, Launch launch, double *out) {
    CHK(ensure_scratch(c, c->als_bias_part, (size_t)(np + 1) * sizeof(double)));
    double *part = (double *)c->als_bias_part.p, *sum = part + np;
    {
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)nnz * (double)c->kp);
        launch(part);
        hipLaunchKernelGGL(cmfk::als_piece_sum_kernel, dim3(1), dim3(64), 0, c->stream, (const double *)part, np, sum);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, sum, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

// the effective weights and products of an image into the caller's buffers (the *_weights test entries); either may be null
static int als_weights_out(cmf_ctx *c, const WCsrDev &M, float *w_eff, float *p_eff) {
    if (M.nnz && w_eff) HIPCHK(hipMemcpyAsync(w_eff, M.hw, (size_t)M.nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (M.nnz && p_eff) HIPCHK(hipMemcpyAsync(p_eff, M.hp, (size_t)M.nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

#endif // CMF_ALS_HOST
