// cmf_als_bias.hip.h -- ALS for explicit ratings: a fixed offset mu and row / column biases on a relation whose weights are bound as
// CSR.  Its term of the objective is
//   1/2 sum_{O} w_ij (t_ij - mu - r_i - c_j - a_i . b_j)^2  +  lb/2 (|r|^2 + |c|^2),        lb >= 0, mu fixed
// One iteration is block coordinate descent: the factor sweeps of cmf_als.hip.h on the ADJUSTED targets bt = t - mu - r_i - c_j
// (the row kernels run unchanged: they read bp = w bt where they read pv = w t), then per biased relation r and c, each the exact
// minimiser of its block:   r_i = sum_{j in O_i} w (t - mu - c_j - a_i . b_j) / (sum_{j in O_i} w + lb),   0 for a row without
// stored entries or with a zero denominator.  What this file adds:
//   als_bias_piece_kernel<GL>   one 256-thread workgroup per PIECE (at most L consecutive stored entries of one row of a CSR image;
//                          option "als_bias_piece"), the walk of cmf_als_entries.hip.h with two gathers in flight per group.  Per
//                          entry the term w (t - mu - other[idx] - a . b) in float32; every group sums its terms and its weights in
//                          float64; the groups are added in group order and the workgroup writes one (num, wsum) pair of doubles.
//                          At most 512 bytes of static LDS
//   als_bias_combine_kernel  per row: its pieces added in piece order, bias = (float)(num / (wsum + lb)), or 0
//   als_bias_targets_kernel  bt = ((t - mu) - rowbias[row]) - colbias[idx] and bp = w bt of one image, each operation rounded once in
//                          float32; one wave per piece (on the transposed image the roles of r and c are swapped by the caller)
//   predict_pairs_kernel<GL>  out = f(((offset + rowbias[row]) + colbias[col]) + a_row . b_col) for arbitrary pairs, one lane group per
//                          pair, f linear or sigmoid; the k-sum in the fixed order of group_sum
// Every cross-workgroup sum is a kernel boundary; no atomics, no grid-wide barrier, vector stores only: a repeated call from the
// same state is bit-identical, and a row's bias depends on the row and on L alone.
#pragma once
#include "cmf_als_entries.hip.h"

namespace cmfk {

struct AlsBiasArgs : AlsEntryArgs {
    const float *tv, *wv;
    const float *other;      // the bias of the image's columns
    float mu;
    double *part;            // [pieces][2]: num, wsum
};

enum { ALS_BIAS_FLIGHT = 2 };   // gathered rows in flight per lane group

// the term w (t - mu - other[idx] - a . b) in float32; sum[0] its sum, sum[1] the weights', in float64 per lane group
struct AlsBiasBody {
    const AlsBiasArgs &g;
    const float *tv, *wv;    // of the piece
    float t[ALS_BIAS_FLIGHT], w[ALS_BIAS_FLIGHT], o[ALS_BIAS_FLIGHT];
    double sum[2] = {0.0, 0.0};
    __device__ __forceinline__ void begin(int64_t beg) { tv = g.tv + beg, wv = g.wv + beg; }
    __device__ __forceinline__ void load(int j, int q, int32_t col) {
        t[j] = tv[q];
        w[j] = wv[q];
        o[j] = g.other[col];
    }
    __device__ __forceinline__ void use(int j, float d, int, bool real) {
#pragma clang fp contract(off)
        const float x = w[j] * (((t[j] - g.mu) - o[j]) - d);
        if (real) {
            sum[0] += (double)x;
            sum[1] += (double)w[j];
        }
    }
};

template <int GL>
__global__ __launch_bounds__(256) void als_bias_piece_kernel(AlsBiasArgs g) {
    AlsBiasBody body{g};
    als_entry_walk<GL, ALS_BIAS_FLIGHT>(g, body);
    als_group_reduce<GL>(body.sum, g.part + 2 * (int64_t)blockIdx.x);
}

// first[row] .. first[row + 1]: the pieces of the row
__global__ __launch_bounds__(256) void als_bias_combine_kernel(const double *part, const int64_t *first, int64_t rows, double lb, float *bias) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int64_t p0 = first[row], p1 = first[row + 1];
    double n = 0.0, w = 0.0;
    for (int64_t p = p0; p < p1; ++p) {
        n += part[2 * p];
        w += part[2 * p + 1];
    }
    const double den = w + lb;
    bias[row] = (p1 > p0 && den > 0.0) ? (float)(n / den) : 0.f;
}

__global__ __launch_bounds__(256) void als_bias_targets_kernel(const AlsEntryPiece *pieces, int64_t npieces, const int32_t *idx, const float *tv, const float *wv,
                                                               const float *rowbias, const float *colbias, float mu, float *bt, float *bp) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (p >= npieces) return;
    const AlsEntryPiece pc = pieces[p];
    const float rb = rowbias[pc.row];
    for (int e = threadIdx.x & 63; e < pc.len; e += 64) {
        const int64_t q = pc.beg + e;
        const float v = ((tv[q] - mu) - rb) - colbias[idx[q]];
        bt[q] = v;
        bp[q] = wv[q] * v;
    }
}

// link: CMF_LINK_LINEAR | CMF_LINK_LOGIT (f = sigmoid).  rowbias / colbias may be null (no such term)
template <int GL>
__global__ __launch_bounds__(256) void predict_pairs_kernel(const int64_t *rows, const int64_t *cols, int64_t n, const float *A, const float *B, int kp,
                                                            const float *rowbias, const float *colbias, float offset, int link, float *out) {
#pragma clang fp contract(off)
    constexpr int NG = 256 / GL;
    const int gl = threadIdx.x % GL, grp = threadIdx.x / GL;
    const int64_t p = (int64_t)blockIdx.x * NG + grp, pq = min(p, n - 1);   // a group past the end repeats the last pair and stores nothing
    const int64_t i = rows[pq], j = cols[pq];
    const f32x4 a = *reinterpret_cast<const f32x4 *>(A + i * kp + 4 * gl);
    const f32x4 b = *reinterpret_cast<const f32x4 *>(B + j * kp + 4 * gl);
    float d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    d = group_sum<GL>(d);
    float s = offset;
    if (rowbias) s = s + rowbias[i];
    if (colbias) s = s + colbias[j];
    s = s + d;
    if (link) s = sigmoidf_(s);
    if (gl == 0 && p < n) out[p] = s;
}

} // namespace cmfk

// ------------------------------------------------------------------ host side (included by cmf_api.hip behind cmf_als_entries.hip.h;
// the bias sweep itself, which under a Huber loss runs the reweighting pass first, stands behind that pass: als_bias_sweep,
// cmf_als_steps.hip.h)
#ifdef CMF_ALS_HOST

enum { ALS_BIAS_PIECE_DEFAULT = 2048 };
// entries per piece ("als_bias_piece": > 0 rounded up to 16; 0 the default; < 0 every row is one piece)
static int64_t als_bias_piece_len(const cmf_ctx *c) {
    if (c->opt_als_bias_piece < 0) return INT32_MAX;
    return c->opt_als_bias_piece > 0 ? rup(c->opt_als_bias_piece, 16) : (int64_t)ALS_BIAS_PIECE_DEFAULT;
}

static bool als_bias_any(const cmf_ctx *c) { return c->als_bias[0].on || c->als_bias[1].on; }

// the piece lists of both images of a relation, from the row lengths (the pattern lives on the device only)
static int als_bias_plan(cmf_ctx *c, int which) {
    AlsBias &b = c->als_bias[which];
    const int64_t L = als_bias_piece_len(c);
    for (int t = 0; t < 2; ++t) {
        dev_free(c, b.pieces[t]); dev_free(c, b.first[t]);
        b.pieces[t] = nullptr; b.first[t] = nullptr;
        CHK(als_image_pieces(c, c->wm_sp[which][t], L, "cmf_set_biases", &b.pieces[t], &b.npieces[t], &b.first[t]));
    }
    b.L = L;
    return CMF_OK;
}
static int als_bias_replan(cmf_ctx *c, int which) {   // the option may have changed since the lists were built
    return c->als_bias[which].L == als_bias_piece_len(c) ? CMF_OK : als_bias_plan(c, which);
}

// bt and bp of both images from the current biases
static int als_bias_refresh(cmf_ctx *c, int which) {
    AlsBias &b = c->als_bias[which];
    if (!b.on || !b.dirty) return CMF_OK;
    CHK(als_bias_replan(c, which));
    for (int t = 0; t < 2; ++t) {
        WCsrDev &M = c->wm_sp[which][t];
        if (b.npieces[t] == 0) continue;
        Timed tm(c, CMF_K_ELEMWISE);
        hipLaunchKernelGGL(cmfk::als_bias_targets_kernel, dim3((unsigned)((b.npieces[t] + 3) / 4)), dim3(256), 0, c->stream,
                           (const cmfk::AlsEntryPiece *)b.pieces[t], b.npieces[t], (const int32_t *)M.idx, (const float *)M.tv, (const float *)M.wv,
                           (const float *)(t == 0 ? b.r : b.c), (const float *)(t == 0 ? b.c : b.r), (float)b.mu, M.bt, M.bp);
        HIPCHK(hipGetLastError());
    }
    b.dirty = false;
    return CMF_OK;
}

// t of relation `which` in the stored order of the transpose: the counting sort of cmf_set_weighted_csr again, from the images on
// the device
static int als_transposed_targets(cmf_ctx *c, int which, std::vector<float> &tt) {
    const WCsrDev &M0 = c->wm_sp[which][0], &M1 = c->wm_sp[which][1];
    const int64_t nnz = M0.nnz;
    std::vector<int64_t> ip((size_t)M0.rows + 1), ipt((size_t)M1.rows + 1);
    std::vector<int32_t> ix((size_t)nnz);
    std::vector<float> t((size_t)nnz);
    tt.assign((size_t)nnz, 0.f);
    HIPCHK(hipMemcpyAsync(ip.data(), M0.indptr, ip.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(ipt.data(), M1.indptr, ipt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (nnz) {
        HIPCHK(hipMemcpyAsync(ix.data(), M0.idx, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(t.data(), M0.tv, (size_t)nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<int64_t> pos(ipt.begin(), ipt.end() - 1);
    for (int64_t i = 0; i < M0.rows; ++i)
        for (int64_t q = ip[(size_t)i]; q < ip[(size_t)i + 1]; ++q) tt[(size_t)pos[(size_t)ix[(size_t)q]]++] = t[(size_t)q];
    return CMF_OK;
}

static int als_bias_which_ok(const char *what, int which) {
    if (which != 0 && which != 1) return fail(CMF_EINVAL, "%s: which must be 0 (X) or 1 (Y)", what);
    return CMF_OK;
}

extern "C" int cmf_set_biases(cmf_ctx *c, int which, int enable, double mu, double lb) {
    NEED_PROBLEM(c);
    CHK(als_bias_which_ok("cmf_set_biases", which));
    const char *nm = which == 0 ? "X" : "Y";
    DeviceGuard dg(c->device);
    if (!enable) {
        HIPCHK(hipStreamSynchronize(c->stream));
        als_bias_free(c, which);
        return CMF_OK;
    }
    if (c->wm_kind[which] != WM_CSR) return fail(CMF_EINVAL, "cmf_set_biases: %s has no CSR weights bound (cmf_set_weighted_csr first)", nm);
    if (!std::isfinite(mu) || !std::isfinite((float)mu) || !(lb >= 0.0) || !std::isfinite(lb))
        return fail(CMF_EINVAL, "cmf_set_biases: mu must be finite (in float32) and lb finite and >= 0, got mu = %g, lb = %g", mu, lb);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_set_biases: n_components <= 256 only (k_pad = %d)", c->kp);
    if (c->wm_bg[which] > 0.0)
        return fail(CMF_EUNSUPPORTED, "cmf_set_biases: %s has a background weight bound; biases and a background weight are not built together: "
                                      "clear it with cmf_set_background_weight(ctx, %d, 0)", nm, which);
    HIPCHK(hipStreamSynchronize(c->stream));
    als_bias_free(c, which);
    AlsBias &b = c->als_bias[which];
    WCsrDev &M0 = c->wm_sp[which][0], &M1 = c->wm_sp[which][1];
    const int64_t nnz = M0.nnz;
    {
        std::vector<float> tt;
        CHK(als_transposed_targets(c, which, tt));
        int rc = dev_alloc(c, (void **)&M1.tv, std::max<size_t>(16, (size_t)nnz * sizeof(float)), false);
        if (rc == CMF_OK && nnz) {
            hipError_t he = hipMemcpyAsync(M1.tv, tt.data(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice, c->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
            if (he != hipSuccess) rc = fail(CMF_EHIP, "cmf_set_biases: %s", hipGetErrorString(he));
        }
        if (rc != CMF_OK) {
            als_bias_free(c, which);
            return rc;
        }
    }
    int rc = dev_alloc(c, (void **)&b.r, std::max<size_t>(16, (size_t)M0.rows * sizeof(float)));
    if (rc == CMF_OK) rc = dev_alloc(c, (void **)&b.c, std::max<size_t>(16, (size_t)M0.cols * sizeof(float)));
    for (int t = 0; t < 2 && rc == CMF_OK; ++t) {
        rc = dev_alloc(c, (void **)&c->wm_sp[which][t].bt, std::max<size_t>(16, (size_t)nnz * sizeof(float)));
        if (rc == CMF_OK) rc = dev_alloc(c, (void **)&c->wm_sp[which][t].bp, std::max<size_t>(16, (size_t)nnz * sizeof(float)));
    }
    b.mu = mu; b.lb = lb;
    if (rc == CMF_OK) rc = als_bias_plan(c, which);
    if (rc != CMF_OK) {
        (void)hipStreamSynchronize(c->stream);
        als_bias_free(c, which);
        return rc;
    }
    b.on = true;
    b.dirty = true;
    return als_bias_refresh(c, which);   // bt / bp are never stale when an entry point returns: every step reads them
}

extern "C" int cmf_get_biases(cmf_ctx *c, int which, double *mu, double *lb, int *enabled) {
    NEED_PROBLEM(c);
    CHK(als_bias_which_ok("cmf_get_biases", which));
    const AlsBias &b = c->als_bias[which];
    if (mu) *mu = b.on ? b.mu : 0.0;
    if (lb) *lb = b.on ? b.lb : 0.0;
    if (enabled) *enabled = b.on ? 1 : 0;
    return CMF_OK;
}

static int als_bias_vector(cmf_ctx *c, const char *what, int which, int axis, float **vec, int64_t *n) {
    CHK(als_bias_which_ok(what, which));
    if (axis != 0 && axis != 1) return fail(CMF_EINVAL, "%s: axis must be 0 (rows) or 1 (columns)", what);
    AlsBias &b = c->als_bias[which];
    if (!b.on) return fail(CMF_EINVAL, "%s: %s has no biases bound (cmf_set_biases first)", what, which == 0 ? "X" : "Y");
    *vec = axis == 0 ? b.r : b.c;
    *n = c->wm_sp[which][axis].rows;
    return CMF_OK;
}

extern "C" int cmf_set_bias_f64(cmf_ctx *c, int which, int axis, const double *v) {
    NEED_PROBLEM(c);
    float *dst; int64_t n;
    CHK(als_bias_vector(c, "cmf_set_bias_f64", which, axis, &dst, &n));
    if (!v && n > 0) return fail(CMF_EINVAL, "cmf_set_bias_f64: null pointer");
    std::vector<float> h((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        h[(size_t)i] = (float)v[i];
        if (!std::isfinite(h[(size_t)i])) return fail(CMF_EINVAL, "cmf_set_bias_f64: entry %lld is not finite in float32", (long long)i);
    }
    DeviceGuard dg(c->device);
    if (n) HIPCHK(hipMemcpyAsync(dst, h.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->als_bias[which].dirty = true;
    return als_bias_refresh(c, which);
}

extern "C" int cmf_get_bias_f64(cmf_ctx *c, int which, int axis, double *v) {
    NEED_PROBLEM(c);
    float *src; int64_t n;
    CHK(als_bias_vector(c, "cmf_get_bias_f64", which, axis, &src, &n));
    if (!v && n > 0) return fail(CMF_EINVAL, "cmf_get_bias_f64: null pointer");
    std::vector<float> h((size_t)n);
    DeviceGuard dg(c->device);
    if (n) HIPCHK(hipMemcpyAsync(h.data(), src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; ++i) v[i] = (double)h[(size_t)i];
    return CMF_OK;
}

// test entry: the adjusted targets bt and bp = w bt of one image (0 the pattern, 1 its transpose); nnz: the entries the
// caller's buffers hold, which must be the stored entries of the pattern
extern "C" int cmf_als_bias_targets(cmf_ctx *c, int which, int image, int64_t nnz, float *host_bt, float *host_bp) {
    NEED_PROBLEM(c);
    float *vec; int64_t n;
    CHK(als_bias_vector(c, "cmf_als_bias_targets", which, image, &vec, &n));
    const WCsrDev &M = c->wm_sp[which][image];
    if (nnz != M.nnz)
        return fail(CMF_EINVAL, "cmf_als_bias_targets: the caller's buffers hold %lld entries, the pattern stores %lld", (long long)nnz, (long long)M.nnz);
    DeviceGuard dg(c->device);
    CHK(als_bias_refresh(c, which));
    if (M.nnz && host_bt) HIPCHK(hipMemcpyAsync(host_bt, M.bt, (size_t)M.nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (M.nnz && host_bp) HIPCHK(hipMemcpyAsync(host_bp, M.bp, (size_t)M.nnz * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_predict_pairs(cmf_ctx *c, int which, int link, int64_t n, const int64_t *rows, const int64_t *cols, float *out) {
    NEED_PROBLEM(c);
    CHK(als_bias_which_ok("cmf_predict_pairs", which));
    if (link != CMF_LINK_LINEAR && link != CMF_LINK_LOGIT) return fail(CMF_EINVAL, "cmf_predict_pairs: link must be CMF_LINK_LINEAR or CMF_LINK_LOGIT");
    if (n < 0) return fail(CMF_EINVAL, "cmf_predict_pairs: negative pair count");
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_predict_pairs: n_components <= 256 only (k_pad = %d)", c->kp);
    if (n == 0) return CMF_OK;
    if (!rows || !cols || !out) return fail(CMF_EINVAL, "cmf_predict_pairs: null pointer");
    const int fa = which == 0 ? CMF_U : CMF_V, fb = which == 0 ? CMF_V : CMF_Z;
    for (int64_t q = 0; q < n; ++q)
        if (rows[q] < 0 || rows[q] >= c->frows[fa] || cols[q] < 0 || cols[q] >= c->frows[fb])
            return fail(CMF_EINVAL, "cmf_predict_pairs: pair %lld = (%lld, %lld) lies outside the %lld x %lld relation", (long long)q, (long long)rows[q],
                        (long long)cols[q], (long long)c->frows[fa], (long long)c->frows[fb]);
    DeviceGuard dg(c->device);
    const size_t ibytes = (size_t)n * sizeof(int64_t);
    CHK(ensure_scratch(c, c->als_bias_ws, 2 * ibytes + (size_t)n * sizeof(float)));
    int64_t *dr = (int64_t *)c->als_bias_ws.p, *dc = dr + n;
    float *dout = (float *)(dc + n);
    HIPCHK(hipMemcpyAsync(dr, rows, ibytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dc, cols, ibytes, hipMemcpyHostToDevice, c->stream));
    const AlsBias &b = c->als_bias[which];
    const float *rb = b.on ? b.r : nullptr, *cb = b.on ? b.c : nullptr;
    const float off = b.on ? (float)b.mu : 0.f;
    {
        Timed tm(c, CMF_K_KLMU, 2.0 * (double)n * (double)c->kp);
        const int gl = c->kp / 4, ng = 256 / gl;
        const dim3 grid((unsigned)((n + ng - 1) / ng)), block(256);
        const float *A = c->F[fa], *B = c->F[fb];
        ALS_LAUNCH_GL(c, predict_pairs_kernel, grid, block, 0, c->stream, dr, dc, n, A, B, c->kp, rb, cb, off, link, dout);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

#endif // CMF_ALS_HOST
