// cmf_als_steps.hip.h -- the host side of the ALS sweeps behind everything it calls (cmf_als.hip.h: the routes and the kernels; the
// sweep descriptor, the ladders and the piece plan; cmf_als_entries / _bias / _bg / _logit / _reweight.hip.h): the chunk loop of the
// formed systems, the planners of the matrix-free and the dual rows, the bias sweep, als_route, als_step -- the one place that
// sweeps -- and the entry points.
#pragma once
#ifdef CMF_ALS_HOST

// ------------------------------------------------------------------ per-row l2 (cmf_set_l2_rows)
// The regulariser l2 / 2 sum_F sum_i m_F[i] |f_i|^2: row i of a sweep of F solves its system under lambda_i = l2 m_F[i].  The device
// holds m_F as float32 and every row kernel forms lambda_i as ONE float32 product (float)l2 * mult[row] (cmfk::als_row_l2); with
// nothing bound the pointer is null and lambda_i = l2.  What the host reads of the multipliers:
//   als_l2_mult    the device image of factor f, or null
//   als_l2_floor   the smallest lambda of the sweep: the l2 the exact solve derives its threshold from (l2 min(m_F) / 16)
//   als_l2_shared  the one l2 of a shared route (a factor without an observed relation: ONE matrix for all rows), which takes equal
//                  multipliers and refuses others
static const float *als_l2_mult(const cmf_ctx *c, int f) { return c->als_l2rows[f].dev; }
static double als_l2_floor(const cmf_ctx *c, int f, double l2) { return c->als_l2rows[f].dev ? l2 * (double)c->als_l2rows[f].min : l2; }
static int als_l2_shared(const cmf_ctx *c, const char *what, int f, double *l2) {
    const AlsL2Rows &m = c->als_l2rows[f];
    if (!m.dev) return CMF_OK;
    if (!m.equal)
        return fail(CMF_EUNSUPPORTED, "%s: %s has per-row l2 multipliers that differ (cmf_set_l2_rows) but no observed relation: its sweep has one "
                                      "matrix for all rows and cannot give them different penalties", what, f == CMF_U ? "U" : (f == CMF_V ? "V" : "Z"));
    *l2 *= (double)m.head;
    return CMF_OK;
}

extern "C" int cmf_set_l2_rows(cmf_ctx *c, int which, const double *mult) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "cmf_set_l2_rows: bad factor selector %d", which);
    const int64_t n = c->frows[which], np = c->frows_pad[which];
    std::vector<float> img((size_t)np, 1.0f);
    if (mult)
        for (int64_t i = 0; i < n; ++i) {
            if (!std::isfinite(mult[i]) || !(mult[i] > 0.0) || !std::isfinite((float)mult[i]) || !((float)mult[i] > 0.f))
                return fail(CMF_EINVAL, "cmf_set_l2_rows: multiplier %lld is %g; every multiplier must be finite and positive (in float32 too)", (long long)i, mult[i]);
            img[(size_t)i] = (float)mult[i];
        }
    DeviceGuard dg(c->device);
    AlsL2Rows &m = c->als_l2rows[which];
    if (!mult) {
        if (m.dev) {
            HIPCHK(hipStreamSynchronize(c->stream));
            dev_free(c, m.dev);
        }
        m = AlsL2Rows();
        return CMF_OK;
    }
    if (!m.dev) CHK(dev_alloc(c, (void **)&m.dev, (size_t)np * sizeof(float), false));
    HIPCHK(hipMemcpyAsync(m.dev, img.data(), (size_t)np * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vector may go
    m.host.assign(mult, mult + n);
    m.min = m.head = n > 0 ? img[0] : 1.0f;
    m.equal = true;
    for (int64_t i = 1; i < n; ++i) {
        m.min = std::min(m.min, img[(size_t)i]);
        m.equal = m.equal && img[(size_t)i] == m.head;
    }
    return CMF_OK;
}

extern "C" int cmf_get_l2_rows(cmf_ctx *c, int which, double *mult, int *set) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "cmf_get_l2_rows: bad factor selector %d", which);
    const AlsL2Rows &m = c->als_l2rows[which];
    if (set) *set = m.dev ? 1 : 0;
    if (mult)
        for (int64_t i = 0; i < c->frows[which]; ++i) mult[i] = m.dev ? m.host[(size_t)i] : 1.0;
    return CMF_OK;
}

// lg: the sweep reads a logistic relation (a.F, a.logit0 / logit1 are set): the instance with the reweighting, and its dot products
static int als_launch_normal(cmf_ctx *c, const cmfk::AlsArgs &a, int64_t npieces, int64_t nnz, bool lg) {
    if (npieces <= 0) return CMF_OK;
    Timed tm(c, CMF_K_ROWHESS, 2.0 * (double)nnz * c->k * c->k + (lg ? 2.0 * (double)nnz * c->k : 0.0));
    const dim3 grid((unsigned)npieces), block(512);
    if (lg) {
        ALS_LAUNCH_KP(c, als_normal_kernel, "ALS normal equations are", hipLaunchKernelGGL(kern, grid, block, 0, c->stream, a), true);
    } else {
        ALS_LAUNCH_KP(c, als_normal_kernel, "ALS normal equations are", hipLaunchKernelGGL(kern, grid, block, 0, c->stream, a), false);
    }
    return CMF_OK;
}

static int als_nnls_launch(cmf_ctx *c, const float *H, const float *g, float *F, const int64_t *first, int64_t nrows, int sweeps) {
    if (nrows <= 0) return CMF_OK;
    cmfk::NnlsArgs a;
    a.H = H; a.g = g; a.F = F; a.first = first; a.nrows = nrows; a.k = c->k; a.sweeps = sweeps;
    Timed tm(c, CMF_K_HALS, 2.0 * (double)nrows * c->k * c->k * sweeps);
    const dim3 grid((unsigned)((nrows + cmfk::NNLS_WAVES - 1) / cmfk::NNLS_WAVES)), block(64 * cmfk::NNLS_WAVES);
    ALS_LAUNCH_KP(c, als_nnls_kernel, "the non-negative row solve is", hipLaunchKernelGGL(kern, grid, block, 0, c->stream, a));
    return CMF_OK;
}

// The observed sides of the sweep as the row kernels read them (weights: the excess under a background; targets: the adjusted ones
// under biases): one binder for the formed route, one for the routes that walk a row's entries themselves.  A side the sweep does
// not have is left as the caller zeroed it.
static void als_bind_sides(const AlsSweep &sw, cmfk::AlsSide &s0, cmfk::AlsSide &s1) {
    for (int s = 0; s < sw.nobs; ++s) {
        const WCsrDev &M = *sw.obs[s].M;
        (s == 0 ? s0 : s1) = cmfk::AlsSide{M.idx, als_side_targets(M), als_side_weights(M), sw.obs[s].B};
    }
}
static void als_bind_sides(const AlsSweep &sw, cmfk::AlsCgSide &s0, cmfk::AlsCgSide &s1) {
    for (int s = 0; s < sw.nobs; ++s) {
        const WCsrDev &M = *sw.obs[s].M;
        (s == 0 ? s0 : s1) = cmfk::AlsCgSide{M.indptr, M.idx, als_side_targets(M), als_side_weights(M), sw.obs[s].B};
    }
}

// The finished systems of slots [slot0, slot0 + nr) of a plan as als_chunks hands them on: H [nr][k_pad][k_pad] (c->als_h), g
// [nr][k_pad] (in c->als_g, where the plan puts it), and the piece index of those slots (no pieces: a row without information), null
// where S gives every row a system.  row0: the row of slot0 in a plan of a range.
struct AlsChunk { int64_t slot0, row0, nr; float *H; const float *g; const int64_t *no_info; };

// THE chunk loop: the only caller of als_normal_kernel / als_finish_kernel.  The slots of the plan in per-row form, chunk by chunk:
// als_normal_kernel over the chunk's pieces, als_finish_kernel, then use(chunk).  A chunk holds at most `cap` slots and (but for a
// single slot) as many pieces.  A plan that is not on the device yet is sent there.
// lrows (a plan of listed rows): the device list of the rows of the slots, which the per-row l2 is looked up by.
template <class Use>
static int als_chunks(cmf_ctx *c, const AlsSweep &sw, double l2, AlsPlan &pl, int64_t cap, Use use, const int64_t *lrows = nullptr) {
    using namespace cmfk;
    const int kp = c->kp;
    const int64_t kk = (int64_t)kp * kp, nslots = (int64_t)pl.first.size() - 1;
    const bool lg = als_logit_sweep(c, sw);   // a sweep that reads a fused logistic relation: the LG = true instance of als_normal_kernel
    int64_t max_rows = 0, max_pieces = 0;
    std::vector<int64_t> cuts{0};
    for (int64_t r = 0; r < nslots;) {
        int64_t e = r;
        while (e < nslots && e - r < cap && (e == r || pl.first[(size_t)e + 1] - pl.first[(size_t)r] <= cap)) ++e;
        max_rows = std::max(max_rows, e - r);
        max_pieces = std::max(max_pieces, pl.first[(size_t)e] - pl.first[(size_t)r]);
        cuts.push_back(e);
        r = e;
    }
    CHK(ensure_scratch(c, c->als_h, (size_t)std::max<int64_t>(1, max_rows) * kk * sizeof(float)));
    CHK(ensure_scratch(c, c->als_part, (size_t)std::max<int64_t>(1, max_pieces) * (kk + kp) * sizeof(float)));
    CHK(ensure_scratch(c, c->als_g, (size_t)(pl.listed ? std::max<int64_t>(1, max_rows) : c->frows_pad[sw.f]) * kp * sizeof(float)));
    if (!pl.dfirst) CHK(als_plan_upload(c, pl));

    AlsArgs a;
    memset(&a, 0, sizeof a);
    als_bind_sides(sw, a.s0, a.s1);
    float *Hc = (float *)c->als_h.p, *Hp = (float *)c->als_part.p;
    const float *l2m = als_l2_mult(c, sw.f);   // the finish kernel finds a slot's multiplier by its row: row0 + slot, or lrows[slot]
    a.Hp = Hp;
    a.gp = Hp + std::max<int64_t>(1, max_pieces) * kk;
    if (lg) {
        a.F = c->F[sw.f];
        for (int s = 0, o = 0; s < sw.nrel; ++s)
            if (sw.observed[s]) (o++ == 0 ? a.logit0 : a.logit1) = als_logit_fused(c, sw.rel[s].which) ? 1 : 0;
    }
    for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
        const int64_t c0 = cuts[ci], c1 = cuts[ci + 1], nr = c1 - c0, row0 = pl.row0 + c0;
        const int64_t pbase = pl.first[(size_t)c0], np = pl.first[(size_t)c1] - pbase;
        float *grad = (float *)c->als_g.p + (pl.listed ? 0 : row0 * kp);
        a.pieces = pl.dpieces + pbase;
        int64_t nnz = 0;
        for (int64_t p = pbase; p < pbase + np; ++p) nnz += pl.pieces[(size_t)p].len;
        CHK(als_launch_normal(c, a, np, nnz, lg));
        {
            Timed tm(c, CMF_K_ELEMWISE);
            if (l2m)
                hipLaunchKernelGGL(als_finish_kernel<true>, dim3((unsigned)nr), dim3(256), 0, c->stream, (const float *)Hp, (const float *)a.gp, pl.dfirst + c0, pbase,
                                   pl.S, pl.N ? pl.N + row0 * kp : nullptr, (float)l2, c->k, kp, Hc, grad, pl.listed ? l2m : l2m + row0,
                                   pl.listed ? lrows + c0 : nullptr);
            else
                hipLaunchKernelGGL(als_finish_kernel<false>, dim3((unsigned)nr), dim3(256), 0, c->stream, (const float *)Hp, (const float *)a.gp, pl.dfirst + c0, pbase,
                                   pl.S, pl.N ? pl.N + row0 * kp : nullptr, (float)l2, c->k, kp, Hc, grad, (const float *)nullptr, (const int64_t *)nullptr);
            HIPCHK(hipGetLastError());
        }
        CHK(use(AlsChunk{c0, row0, nr, Hc, grad, pl.S ? nullptr : pl.dfirst + c0}));
    }
    return CMF_OK;
}

// Rows [r_begin, r_end) of the sweep through the chunk loop: the shared terms (the full relation: its Gram into every row's matrix,
// its product into the right-hand sides; a background: c0 times the Gram), then the plan of the range.
template <class Use>
static int als_chunks_range(cmf_ctx *c, const AlsSweep &sw, double l2, int64_t r_begin, int64_t r_end, int64_t cap, Use use) {
    AlsPlan pl;
    CHK(als_shared_terms(c, sw, &pl.S, &pl.N));
    CHK(als_plan(c, sw, r_begin, r_end, pl));
    return als_chunks(c, sw, l2, pl, cap, use);   // (a range: no list)
}

// What safe_solve_rows (cmf_newton.hip.h) reads and writes of the Newton step's state: put back when the scope ends.
struct AlsNewtonStateGuard {
    cmf_ctx *const c;
    const bool psd;
    const int64_t rank1, eig;
    std::vector<int> bad;
    explicit AlsNewtonStateGuard(cmf_ctx *ctx) : c(ctx), psd(ctx->hess_psd), rank1(ctx->rank1_rows), eig(ctx->eig_clamp_rows) { bad.swap(c->bad_host); }
    ~AlsNewtonStateGuard() { c->hess_psd = psd; c->rank1_rows = rank1; c->eig_clamp_rows = eig; c->bad_host.swap(bad); }
};

// THE exact solve of nr systems of order n (pitch np) with lambda_min >= l2: the plain route of the per-row Newton sweeps, the
// matrices declared positive semi-definite.  Its threshold l2 / 16 lies well below l2: the test of that route (a Cholesky of
// H_i - pert I whose pivots must exceed 4e-6 max H_jj) passes unless cond(H_i) is above ~2e5, where a float32 factorisation has
// nothing left to give.  The exact rows, the dual systems and the formed rows of a dual sweep all come here.
// Under per-row multipliers the caller passes the smallest lambda of the sweep (als_l2_floor): lambda_min >= that for every row.
static int als_solve_rows(cmf_ctx *c, float *H, const float *g, float *out, int64_t nr, int n, int np, double l2) {
    AlsNewtonStateGuard keep(c);
    c->hess_psd = true;
    return safe_solve_rows(c, H, g, out, nr, n, np, l2 / 16.0);
}

// rows exact: the solves of every chunk into c->als_sol
static int als_rows_solve(cmf_ctx *c, const AlsSweep &sw, double l2) {
    CHK(ensure_scratch(c, c->als_sol, (size_t)c->frows_pad[sw.f] * c->kp * sizeof(float)));
    return als_chunks_range(c, sw, l2, 0, c->frows[sw.f], hessian_chunk_rows(c, c->frows_pad[sw.f]), [&](const AlsChunk &ch) -> int {
        return als_solve_rows(c, ch.H, ch.g, (float *)c->als_sol.p + ch.row0 * c->kp, ch.nr, c->k, c->kp, als_l2_floor(c, sw.f, l2));
    });
}

// rows NNLS: `sweeps` coordinate-descent sweeps of every chunk's rows of F, in place (the gathered factors are the other ones: the
// chunks to come do not read the rows written here)
static int als_rows_nnls(cmf_ctx *c, const AlsSweep &sw, double l2, int sweeps) {
    return als_chunks_range(c, sw, l2, 0, c->frows[sw.f], hessian_chunk_rows(c, c->frows_pad[sw.f]), [&](const AlsChunk &ch) -> int {
        return als_nnls_launch(c, ch.H, ch.g, c->F[sw.f] + ch.row0 * c->kp, ch.no_info, ch.nr, sweeps);
    });
}

// cmf_als_normal: the finished systems of rows [r_begin, r_end), one chunk, back to the host
static int als_rows_to_host(cmf_ctx *c, const AlsSweep &sw, double l2, int64_t r_begin, int64_t r_end, float *host_H, float *host_g) {
    return als_chunks_range(c, sw, l2, r_begin, r_end, INT64_MAX, [&](const AlsChunk &ch) -> int {
        if (host_H) HIPCHK(hipMemcpyAsync(host_H, ch.H, (size_t)ch.nr * c->kp * c->kp * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (host_g) HIPCHK(hipMemcpyAsync(host_g, ch.g, (size_t)ch.nr * c->kp * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return CMF_OK;
    });
}

static int als_apply(cmf_ctx *c, int f, const float *sol, bool nn) {
    return launch_ew(c, cmfk::als_apply_kernel, c->frows[f] * c->kp, c->F[f], sol, c->frows[f], c->k, c->kp, nn ? 1 : 0);
}

// shared exact: F <- clamp(N (G + l2 I)^-1), the inverse formed once in float64
static int als_sweep_shared(cmf_ctx *c, const char *what, const AlsSweep &sw, double l2, bool nn) {
    CHK(als_l2_shared(c, what, sw.f, &l2));
    CHK(ensure_shared64(c));
    for (int s = 0; s < sw.nrel; ++s) {
        const AlsRel &r = sw.rel[s];
        CHK(gram64(c, c->F[r.fb], c->frows_pad[r.fb], (double *)(s == 0 ? c->g64a.p : c->g64b.p), nullptr));
        CHK(data_times(c, r.which, r.data_trans, c->F[r.fb], c->num, s > 0));
    }
    CHK(launch_hess64(c, (const double *)c->g64a.p, 1.0, sw.nrel > 1 ? (const double *)c->g64b.p : nullptr, 1.0, l2));
    const int rc = shared_inverse64(c, (const double *)c->h64.p, c->k, 0.5 * l2, true);
    if (rc == CMF_EUNSUPPORTED) return fail(CMF_EHIP, "%s: the float64 inverse of G + l2 I failed (non-finite factors?)", what);
    CHK(rc);
    CHK(gemm(c, MODE_NN, c->num, c->kp, c->Hinv, c->kp, c->den, c->frows_pad[sw.f], c->kp, c->kp));
    return als_apply(c, sw.f, c->den, nn);
}

// shared HALS: N and G as cmf_hals_step forms them, `sweeps` passes of hals_sweep
static int als_nnls_sweep_shared(cmf_ctx *c, const char *what, int f, double l2, int sweeps) {
    CHK(als_l2_shared(c, what, f, &l2));
    const float *N = c->num, *G = c->G2;
    if (f == CMF_V) {
        CHK(cmf_mu_v_partials(c, c->vbuf));
        N = c->vbuf;
        G = c->vbuf + c->dp * c->kp;
    } else {
        CHK(gram32(c, c->F[CMF_V], c->dp, c->G2));
        CHK(data_times(c, f == CMF_U ? 0 : 1, f == CMF_Z, c->F[CMF_V], c->num));
    }
    for (int s = 0; s < sweeps; ++s) CHK(hals_sweep(c, f, N, G, 0.0, l2));
    return CMF_OK;
}

enum { ALS_CG_LDS_TOTAL = 156 * 1024, ALS_CG_CLASSES = 4 };   // (156 KB: the largest dynamic LDS any kernel here asks for)
// bytes of dynamic LDS the gathered rows of one row may take ("als_cg_lds": 0 every row streams; at most what is left of 156 KB).
// The default leaves room for four workgroups per CU: measured on C5's pattern at k_pad = 256, rows of 100 entries resident at one
// workgroup per CU take twice the time of the same rows gathered again in every pass at eight.
static int64_t als_cg_lds_bytes(const cmf_ctx *c) {
    const int64_t fixed = 4 * (int64_t)cmfk::als_cg_fixed_floats(c->kp);
    return c->opt_als_cg_lds < 0 ? ALS_CG_LDS_TOTAL / 4 - fixed : std::min<int64_t>(c->opt_als_cg_lds, ALS_CG_LDS_TOTAL - fixed);
}

static int als_cg_launch(cmf_ctx *c, const cmfk::AlsCgArgs &a, int64_t nrows) {
    if (nrows <= 0) return CMF_OK;
    const size_t lds = 4 * (size_t)cmfk::als_cg_fixed_floats(c->kp) + (size_t)a.cap * cmfk::als_cg_entry_bytes(c->kp);
    const dim3 grid((unsigned)nrows), block(256);
    if (a.l2m) {   // per-row l2: the LR = true instance
        ALS_LAUNCH_KP(c, als_cg_kernel, "the conjugate-gradient row solve is",
                      CHK(allow_big_lds(c, (const void *)kern, ALS_CG_LDS_TOTAL)); hipLaunchKernelGGL(kern, grid, block, lds, c->stream, a), true);
    } else {
        ALS_LAUNCH_KP(c, als_cg_kernel, "the conjugate-gradient row solve is",
                      CHK(allow_big_lds(c, (const void *)kern, ALS_CG_LDS_TOTAL)); hipLaunchKernelGGL(kern, grid, block, lds, c->stream, a), false);
    }
    return CMF_OK;
}

enum { ALS_CG_PIECE_DEFAULT = 2048 };   // the fastest of 2048, 4096, 16384 and 65536 on the V sweep of C5 Zipf at k = 256
// entries per piece of a long row of the CG route ("als_cg_piece": > 0 rounded up to 16; 0 the default; < 0 no row is ever cut)
static int64_t als_cg_piece_len(const cmf_ctx *c) {
    if (c->opt_als_cg_piece < 0) return INT64_MAX;
    return c->opt_als_cg_piece > 0 ? rup(c->opt_als_cg_piece, 16) : (int64_t)ALS_CG_PIECE_DEFAULT;
}

// What als_cg_piece_kernel reads of the long rows of a sweep, signed or non-negative, and their scratch (als_cg_long):
// state [vecs][k_pad] per row | partials [k_pad] per piece | row_bytes per row of the route's own words, which start at *own.
static int als_cg_piece_args(cmf_ctx *c, const cmfk::AlsCgArgs &a, const cmfk::AlsCgLongRow *dlongs, const cmfk::AlsCgPiece *dpieces, size_t nl,
                             size_t npieces, int vecs, size_t row_bytes, cmfk::AlsCgPieceArgs &p, float **own) {
    const size_t sfloats = ((size_t)vecs * nl + npieces) * (size_t)c->kp;
    CHK(ensure_scratch(c, c->als_cg_long, sfloats * sizeof(float) + nl * row_bytes));
    memset(&p, 0, sizeof p);
    p.s0 = a.s0; p.s1 = a.s1;
    p.pieces = dpieces; p.rows = dlongs;
    p.Fin = a.Fin;
    p.state = (float *)c->als_cg_long.p;
    p.state_vecs = vecs;
    p.partial = p.state + (size_t)vecs * nl * (size_t)c->kp;
    *own = p.state + sfloats;
    return CMF_OK;
}

// one pass over the pieces: the first one (every row, x = the factor row, clamped for the non-negative rows), or a later one of the
// rows whose word in p.takes holds `takes_value`
static int als_cg_piece_pass(cmf_ctx *c, cmfk::AlsCgPieceArgs &p, int64_t npieces, bool first, bool clamp, int takes_value) {
    p.first = first ? 1 : 0;
    p.clamp = clamp ? 1 : 0;
    p.takes_value = takes_value;
    ALS_LAUNCH_KP(c, als_cg_piece_kernel, "the conjugate-gradient row solve is",
                  hipLaunchKernelGGL(kern, dim3((unsigned)npieces), dim3(256), 0, c->stream, p));
    return CMF_OK;
}

// the long rows of a sweep: 2 (steps + 1) launches, pieces then combine, once for r = g - H f and once per step
static int als_cg_long_rows(cmf_ctx *c, cmfk::AlsCgLongArgs &a, int64_t nlong, int64_t npieces, int steps) {
    if (nlong <= 0) return CMF_OK;
    const dim3 cgrid((unsigned)nlong), block(256);
    for (int s = 0; s <= steps; ++s) {
        a.phase = s == 0 ? 0 : (s == steps ? 2 : 1);
        CHK(als_cg_piece_pass(c, a.p, npieces, s == 0, false, 1));   // (later passes: the rows still alive)
        if (a.l2m) {
            ALS_LAUNCH_KP(c, als_cg_combine_kernel, "the conjugate-gradient row solve is", hipLaunchKernelGGL(kern, cgrid, block, 0, c->stream, a), true);
        } else {
            ALS_LAUNCH_KP(c, als_cg_combine_kernel, "the conjugate-gradient row solve is", hipLaunchKernelGGL(kern, cgrid, block, 0, c->stream, a), false);
        }
    }
    return CMF_OK;
}

// The launches of the non-negative rows (cmf_als_nncg.hip.h) behind the plan of als_cg_rows: one launch per capacity class, then the
// long rows -- 2 launches for r = g - H f and 4 per step (piece, combine A, piece, combine B).  The passes every row ran stay on the
// device; they come back (4 bytes a row) only for cmf_als_nncg_passes, or with kernel timing on, behind the timed stretch, to charge
// 4 len k flops per pass (+ 2 k^2 with a full side): a sweep without either waits for nothing.
static int als_nncg_count(cmf_ctx *c) {
    if (c->als_nncg_counted) return CMF_OK;
    const size_t n = c->als_nncg_lens.size();
    std::vector<int32_t> passes(n, 0);
    if (n) {
        HIPCHK(hipMemcpyAsync(passes.data(), c->als_nncg_passes.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    int64_t total = 0, entry_passes = 0;
    for (size_t r = 0; r < n; ++r) {
        total += passes[r];
        entry_passes += (int64_t)c->als_nncg_lens[r] * passes[r];
    }
    c->als_nncg_last[2] = total;
    c->als_nncg_last[3] = entry_passes;
    c->als_nncg_counted = true;
    return CMF_OK;
}

static int als_nncg_launches(cmf_ctx *c, const cmfk::AlsCgArgs &a, const std::vector<int64_t> &lens, const std::vector<int64_t> *list,
                             const int64_t *caps, const int64_t *drows, const cmfk::AlsCgLongRow *dlongs, const cmfk::AlsCgPiece *dpieces,
                             const std::vector<cmfk::AlsCgLongRow> &longs, int64_t npieces, int64_t nrows) {
    using namespace cmfk;
    const int kp = c->kp, steps = a.steps;
    const size_t nl = longs.size();
    CHK(ensure_scratch(c, c->als_nncg_passes, (size_t)nrows * sizeof(int32_t)));
    HIPCHK(hipMemsetAsync(c->als_nncg_passes.p, 0, (size_t)nrows * sizeof(int32_t), c->stream));
    AlsNncgArgs na;
    na.a = a;
    na.passes = (int32_t *)c->als_nncg_passes.p;
    AlsNncgLongArgs pa;
    memset(&pa, 0, sizeof pa);
    if (nl) {   // the state of a long row is 5 vectors, its own words a record; a later pass takes the rows whose record's mode asks for it
        float *own;
        CHK(als_cg_piece_args(c, a, dlongs, dpieces, nl, (size_t)npieces, 5, sizeof(AlsNncgRow), pa.p, &own));
        pa.info = (AlsNncgRow *)own;
        pa.p.takes = &pa.info->mode;
        pa.p.takes_stride = (int)(sizeof(AlsNncgRow) / sizeof(int32_t));
        pa.S = a.S; pa.N = a.N; pa.Fout = a.Fout; pa.out_row0 = a.out_row0;
        pa.passes = na.passes;
        pa.l2 = a.l2; pa.l2m = a.l2m; pa.k = a.k;
    }
    c->als_nncg_lens.assign(lens.begin(), lens.end());   // (each at most 2^31 - 1: the planner's check)
    c->als_nncg_counted = false;
    bool timed = false;
    {
        Timed tm(c, CMF_K_ROWHESS, 0.0);
        timed = tm.on;
        int64_t done = 0;
        for (int q = 0; q <= ALS_CG_CLASSES; ++q) {
            const int64_t n = (int64_t)list[q].size();
            na.a.rows = drows + done;
            na.a.cap = (int)caps[q];
            done += n;
            if (n <= 0) continue;
            const size_t lds = 4 * (size_t)als_cg_fixed_floats(kp) + (size_t)na.a.cap * als_cg_entry_bytes(kp);
            const dim3 grid((unsigned)n), block(256);
            if (a.l2m) {   // per-row l2: the LR = true instance
                ALS_LAUNCH_KP(c, als_nncg_kernel, "the non-negative conjugate-gradient row solve is",
                              CHK(allow_big_lds(c, (const void *)kern, ALS_CG_LDS_TOTAL)); hipLaunchKernelGGL(kern, grid, block, lds, c->stream, na), true);
            } else {
                ALS_LAUNCH_KP(c, als_nncg_kernel, "the non-negative conjugate-gradient row solve is",
                              CHK(allow_big_lds(c, (const void *)kern, ALS_CG_LDS_TOTAL)); hipLaunchKernelGGL(kern, grid, block, lds, c->stream, na), false);
            }
        }
        if (nl) {
            const dim3 cgrid((unsigned)nl), block(256);
            for (int s = 0; s <= 2 * steps; ++s) {
                pa.stage = s == 0 ? 0 : 2 - (s & 1);
                pa.last = s == 2 * steps ? 1 : 0;
                CHK(als_cg_piece_pass(c, pa.p, npieces, s == 0, true, pa.stage == 1 ? ALS_NNCG_ROW_STEP : ALS_NNCG_ROW_PROJECT));
                if (a.l2m) {
                    ALS_LAUNCH_KP(c, als_nncg_combine_kernel, "the non-negative conjugate-gradient row solve is", hipLaunchKernelGGL(kern, cgrid, block, 0, c->stream, pa), true);
                } else {
                    ALS_LAUNCH_KP(c, als_nncg_combine_kernel, "the non-negative conjugate-gradient row solve is", hipLaunchKernelGGL(kern, cgrid, block, 0, c->stream, pa), false);
                }
            }
        }
    }
    if (timed) {   // (the scope has recorded its events: the read-back is not in the timed stretch)
        CHK(als_nncg_count(c));
        c->pending.back().flops = 4.0 * (double)c->als_nncg_last[3] * c->k + (a.S ? 2.0 * (double)c->als_nncg_last[2] * c->k * c->k : 0.0);
    }
    return CMF_OK;
}

// rows CG: rows [r_begin, r_end) of the sweep (which has an observed relation) by `steps` CG steps from the rows of c->F[f];
// row r goes to Fout + (r - out_row0) * k_pad (in place: Fout = c->F[f], out_row0 = 0 -- the gathered factors are the other ones).
// The rows are sorted into capacity classes by their stored entries: capacity / 8, / 4, / 2 and the whole capacity keep the
// gathered rows in LDS (shorter rows: more workgroups per CU), longer rows stream; one launch per class.  A row with more than
// als_cg_piece_len entries goes to none of them: it is cut into pieces (cmf_als_cg.hip.h), all such rows of the sweep together.
// nn: the non-negative rows of cmf_als_nncg.hip.h instead (the same classes, the same pieces; the passes every row ran come back to
// the host, which charges the passes actually run).
static int als_cg_rows(cmf_ctx *c, const char *what, const AlsSweep &sw, double l2, int64_t r_begin, int64_t r_end, int steps, float *Fout, int64_t out_row0,
                       bool nn = false) {
    using namespace cmfk;
    const int kp = c->kp;
    const int64_t nrows = r_end - r_begin;
    AlsCgArgs a;
    memset(&a, 0, sizeof a);
    CHK(als_shared_terms(c, sw, &a.S, &a.N));
    std::vector<int64_t> ip[2];
    CHK(als_fetch_indptr(c, sw, r_begin, r_end, ip));
    const std::vector<int64_t> lens = als_row_lens(ip, sw.nobs, nrows);
    als_bind_sides(sw, a.s0, a.s1);
    const int64_t cap_max = als_cg_lds_bytes(c) / als_cg_entry_bytes(kp);
    int64_t caps[ALS_CG_CLASSES + 1];
    for (int q = 0; q < ALS_CG_CLASSES; ++q) caps[q] = cap_max >> (ALS_CG_CLASSES - 1 - q);
    caps[ALS_CG_CLASSES] = 0;                                   // the streamed class
    const int64_t L = als_cg_piece_len(c);
    std::vector<int64_t> list[ALS_CG_CLASSES + 1];
    std::vector<AlsCgLongRow> longs;
    std::vector<AlsCgPiece> pieces;
    int64_t nnz = 0;
    for (int64_t r = 0; r < nrows; ++r) {
        const int64_t len = lens[(size_t)r];
        if (len > INT32_MAX) return fail(CMF_EUNSUPPORTED, "%s: a row with more than 2^31 - 1 stored entries", what);
        nnz += len;
        if (len > L) {
            const int64_t np = (len + L - 1) / L;
            if ((int64_t)pieces.size() + np > INT32_MAX) return fail(CMF_EUNSUPPORTED, "%s: more than 2^31 - 1 pieces of long rows (als_cg_piece too small)", what);
            const int32_t slot = (int32_t)longs.size();
            longs.push_back(AlsCgLongRow{r_begin + r, (int32_t)pieces.size(), (int32_t)np});
            for (int64_t q = 0; q < len; q += L) pieces.push_back(AlsCgPiece{slot, (int32_t)q, (int32_t)std::min(L, len - q), 0});
            continue;
        }
        int q = 0;
        while (q < ALS_CG_CLASSES && len > caps[q]) ++q;
        list[q].push_back(r_begin + r);
    }
    int64_t *last = nn ? c->als_nncg_last : c->als_cg_last;
    last[0] = (int64_t)longs.size();
    last[1] = (int64_t)pieces.size();
    std::vector<int64_t> all;
    all.reserve((size_t)nrows);
    for (int q = 0; q <= ALS_CG_CLASSES; ++q) all.insert(all.end(), list[q].begin(), list[q].end());
    // descriptors, once per sweep: the rows of the class launches | the long rows | their pieces
    const size_t rbytes = std::max<size_t>(16, all.size() * sizeof(int64_t)), lbytes = longs.size() * sizeof(AlsCgLongRow);
    CHK(ensure_scratch(c, c->als_desc, rbytes + lbytes + pieces.size() * sizeof(AlsCgPiece)));
    int64_t *drows = (int64_t *)c->als_desc.p;
    AlsCgLongRow *dlongs = (AlsCgLongRow *)((char *)c->als_desc.p + rbytes);
    AlsCgPiece *dpieces = (AlsCgPiece *)((char *)dlongs + lbytes);
    if (!all.empty()) HIPCHK(hipMemcpyAsync(drows, all.data(), all.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (!longs.empty()) {
        HIPCHK(hipMemcpyAsync(dlongs, longs.data(), lbytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dpieces, pieces.data(), pieces.size() * sizeof(AlsCgPiece), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream)); // the host vectors may go
    a.Fin = c->F[sw.f];
    a.Fout = Fout;
    a.out_row0 = out_row0;
    a.l2 = (float)l2;
    a.l2m = als_l2_mult(c, sw.f);
    a.k = c->k;
    a.steps = steps;
    if (nn) return als_nncg_launches(c, a, lens, list, caps, drows, dlongs, dpieces, longs, (int64_t)pieces.size(), nrows);
    AlsCgLongArgs pa;
    memset(&pa, 0, sizeof pa);
    if (!longs.empty()) {   // the state of a long row is 3 vectors, its own words r.r (all rows) | alive flags (all rows)
        const size_t nl = longs.size();
        CHK(als_cg_piece_args(c, a, dlongs, dpieces, nl, pieces.size(), 3, 2 * sizeof(float), pa.p, &pa.rr));
        pa.alive = (int32_t *)(pa.rr + nl);
        pa.p.takes = pa.alive;
        pa.p.takes_stride = 1;
        pa.S = a.S; pa.N = a.N; pa.Fout = Fout; pa.out_row0 = out_row0;
        pa.l2 = a.l2; pa.l2m = a.l2m; pa.k = a.k;
    }
    Timed tm(c, CMF_K_ROWHESS, (4.0 * (double)nnz * c->k + (a.S ? 2.0 * (double)nrows * c->k * c->k : 0.0)) * (steps + 1));
    int64_t done = 0;
    for (int q = 0; q <= ALS_CG_CLASSES; ++q) {
        a.rows = drows + done;
        a.cap = (int)caps[q];
        CHK(als_cg_launch(c, a, (int64_t)list[q].size()));
        done += (int64_t)list[q].size();
    }
    return als_cg_long_rows(c, pa, (int64_t)longs.size(), (int64_t)pieces.size(), steps);
}

// ------------------------------------------------------------------ rows dual (kernels: cmf_als_dual.hip.h)
enum { ALS_DUAL_CLASSES = 3, ALS_DUAL_MAX = 128 };
static int als_dual_np(int64_t n) { return n <= 32 ? 32 : (n <= 64 ? 64 : 128); }
// what becomes of a row of `len` stored entries (the slots of cmf_als_dual_last): 0 | 1 | 2 dual in class 32 | 64 | 128, 3 formed, 4 zeros
enum { ALS_DUAL_FORMED = ALS_DUAL_CLASSES, ALS_DUAL_ZERO, ALS_DUAL_KINDS };
static int als_dual_kind(int64_t len, int dual_max, int kp) {
    if (len == 0) return ALS_DUAL_ZERO;
    if (len > dual_max || als_dual_np(len) >= kp) return ALS_DUAL_FORMED;
    return als_dual_np(len) == 32 ? 0 : (als_dual_np(len) == 64 ? 1 : 2);
}

// why the sweep is not eligible for the dual route (null: it is): every relation it reads must be observed without a background
// weight (als_shared_terms then gives S = N = null) and none may be logistic -- als_route's conditions, in words
static const char *als_dual_why_not(const cmf_ctx *c, const AlsSweep &sw) {
    if (!als_observed(sw)) return "no observed relation: one shared matrix, no per-row systems";
    if (als_shared_present(c, sw)) return "a shared term (a full relation or a background weight): the Woodbury form with a shared matrix is not built";
    if (als_logit_sweep(c, sw)) return "a logistic relation: reweighted dual rows are not built";
    return nullptr;
}

template <int KP, bool LR>
static int als_dual_launch_class_lr(cmf_ctx *c, const cmfk::AlsDualArgs &a, int np) {
    using namespace cmfk;
    const dim3 block(256);
    if constexpr (KP > 32) {
        if (np == 32) hipLaunchKernelGGL((als_dual_gram_kernel<KP, 32, LR>), dim3((unsigned)((a.nrows + 3) / 4)), block, 0, c->stream, a);
    }
    if constexpr (KP > 64) {
        if (np == 64) hipLaunchKernelGGL((als_dual_gram_kernel<KP, 64, LR>), dim3((unsigned)a.nrows), block, 0, c->stream, a);
    }
    if constexpr (KP > 128) {
        if (np == 128) hipLaunchKernelGGL((als_dual_gram_kernel<KP, 128, LR>), dim3((unsigned)a.nrows), block, 0, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    return CMF_OK;
}
// (per-row l2 bound: the LR = true instances)
template <int KP>
static int als_dual_launch_class(cmf_ctx *c, const cmfk::AlsDualArgs &a, int np) {
    return a.l2m ? als_dual_launch_class_lr<KP, true>(c, a, np) : als_dual_launch_class_lr<KP, false>(c, a, np);
}

// Rows [r_begin, r_end) of an ELIGIBLE sweep (als_dual_why_not is null, k_pad > 32) under dual_max >= 1: the dual rows class by class
// (Gram, solve, back-product, in chunks of rows whose K scratch stays within the byte budget hessian_chunk_rows gives the exact
// route), zeros for the rows without a stored entry, and the rest through the chunk loop as a plan of listed rows, solved and
// scattered: a formed row keeps the bits cmf_als_step gives it.  Row r goes to Fout + (r - out_row0) k_pad.
// none_dual (a whole sweep): when no row of the plan goes dual nothing is launched, no list and no piece is built, and *none_dual is
// set -- the caller runs the exact sweep as it stands (the same bits: a row without an entry solves l2 f = 0).
static int als_dual_rows(cmf_ctx *c, const AlsSweep &sw, double l2, int64_t r_begin, int64_t r_end, int dual_max, bool nn, float *Fout, int64_t out_row0,
                         bool *none_dual = nullptr) {
    using namespace cmfk;
    const int kp = c->kp;
    const int64_t nrows = r_end - r_begin;
    std::vector<int64_t> ip[2];
    CHK(als_fetch_indptr(c, sw, r_begin, r_end, ip));
    const std::vector<int64_t> lens = als_row_lens(ip, sw.nobs, nrows);
    int64_t *cnt = c->als_dual_last;
    for (int q = 0; q < ALS_DUAL_KINDS; ++q) cnt[q] = 0;
    for (int64_t r = 0; r < nrows; ++r) ++cnt[als_dual_kind(lens[(size_t)r], dual_max, kp)];
    if (none_dual) {
        *none_dual = cnt[0] + cnt[1] + cnt[2] == 0;
        if (*none_dual) return CMF_OK;
    }
    std::vector<int64_t> list[ALS_DUAL_KINDS];   // rows of the range (from r_begin)
    for (int q = 0; q < ALS_DUAL_KINDS; ++q) list[q].reserve((size_t)cnt[q]);
    for (int64_t r = 0; r < nrows; ++r) list[als_dual_kind(lens[(size_t)r], dual_max, kp)].push_back(r);
    // the plan of the formed rows; with it, once per sweep, the row lists: the three classes | the formed rows | the zero rows
    AlsPlan pl;
    pl.listed = true;
    pl.first = als_cut_rows(ip, sw.nobs, nrows, als_piece_len(c), [&](int64_t r, int s, int64_t beg, int32_t len) {
        pl.pieces.push_back(AlsPiece{beg, len, s, r_begin + r});
    }, &list[ALS_DUAL_FORMED]);
    pl.rows.reserve((size_t)nrows);
    for (int q = 0; q < ALS_DUAL_KINDS; ++q)
        for (const int64_t r : list[q]) pl.rows.push_back(r_begin + r);
    CHK(als_plan_upload(c, pl));

    const int64_t cap_exact = hessian_chunk_rows(c, c->frows_pad[sw.f]);
    const int64_t budget = cap_exact * kp * kp;          // floats of K scratch a chunk may take: the exact route's
    AlsDualArgs a;
    memset(&a, 0, sizeof a);
    als_bind_sides(sw, a.s0, a.s1);
    a.Fout = Fout;
    a.out_row0 = out_row0;
    a.l2 = (float)l2;
    a.l2m = als_l2_mult(c, sw.f);
    a.k = c->k;
    a.nn = nn ? 1 : 0;
    int64_t done = 0;
    for (int q = 0; q < ALS_DUAL_CLASSES; ++q) {
        const int np = 32 << q;
        const int64_t n = cnt[q], per = (int64_t)np * np;
        const int64_t cap = std::max<int64_t>(4, budget / per / 4 * 4);
        for (int64_t r0 = 0; r0 < n; r0 += cap) {
            const int64_t nr = std::min(cap, n - r0);
            CHK(ensure_scratch(c, c->als_dual_ws, (size_t)nr * (per + 2 * np) * sizeof(float)));
            a.rows = pl.drows + done + r0;
            a.nrows = nr;
            a.K = (float *)c->als_dual_ws.p;
            a.y = a.K + nr * per;
            float *z = a.y + nr * np;
            a.z = z;
            {
                Timed tm(c, CMF_K_ROWHESS, 2.0 * (double)nr * np * np * c->k);
                switch (kp) {
                case 64: CHK(als_dual_launch_class<64>(c, a, np)); break;
                case 128: CHK(als_dual_launch_class<128>(c, a, np)); break;
                case 256: CHK(als_dual_launch_class<256>(c, a, np)); break;
                default: return fail(CMF_EUNSUPPORTED, "the dual ALS rows are built for k_pad 64, 128 and 256 (k_pad = %d)", kp);
                }
            }
            CHK(als_solve_rows(c, a.K, a.y, z, nr, np, np, als_l2_floor(c, sw.f, l2)));
            {
                Timed tm(c, CMF_K_ELEMWISE);
                const dim3 grid((unsigned)((nr + 3) / 4)), block(256);
                switch (kp) {
                case 64: hipLaunchKernelGGL((als_dual_back_kernel<64>), grid, block, 0, c->stream, a, np); break;
                case 128: hipLaunchKernelGGL((als_dual_back_kernel<128>), grid, block, 0, c->stream, a, np); break;
                default: hipLaunchKernelGGL((als_dual_back_kernel<256>), grid, block, 0, c->stream, a, np); break;
                }
                HIPCHK(hipGetLastError());
            }
        }
        done += n;
    }
    const int64_t *dformed = pl.drows + done, *dzeros = dformed + cnt[ALS_DUAL_FORMED];
    if (cnt[ALS_DUAL_ZERO])
        CHK(launch_ew(c, als_dual_scatter_kernel, cnt[ALS_DUAL_ZERO] * kp, Fout, out_row0, dzeros, (const float *)nullptr, cnt[ALS_DUAL_ZERO], c->k, kp, 0));
    if (!cnt[ALS_DUAL_FORMED]) return CMF_OK;
    CHK(ensure_scratch(c, c->als_sol, (size_t)std::min(cnt[ALS_DUAL_FORMED], cap_exact) * kp * sizeof(float)));   // (a chunk's rows)
    return als_chunks(c, sw, l2, pl, cap_exact, [&](const AlsChunk &ch) -> int {
        float *sol = (float *)c->als_sol.p;
        CHK(als_solve_rows(c, ch.H, ch.g, sol, ch.nr, c->k, kp, als_l2_floor(c, sw.f, l2)));
        return launch_ew(c, als_dual_scatter_kernel, ch.nr * kp, Fout, out_row0, dformed + ch.slot0, (const float *)sol, ch.nr, c->k, kp, nn ? 1 : 0);
    }, dformed);
}

// ------------------------------------------------------------------ the dispatcher
// What an entry point asks of a step beyond l2 and the masks; 0 / false: it has no such argument.
//   nn_sweeps > 0    the factors in nn_mask are swept by coordinate descent (0: their solved rows are projected)
//   cg_steps > 0     a signed factor with an observed relation runs that many CG steps per row instead of the exact solves
//   nn_cg_steps > 0  a non-negative factor with an observed relation runs that many projected CG steps per row
//   dual_max > 0     an exact row sweep without a shared term or a logistic relation solves its rows of 1 .. dual_max entries in dual form
//   biases           biases are bound: the adjusted targets are refreshed before the sweeps and the bias blocks swept after them
// A relation under a Huber loss (cmf_als_reweight.hip.h) is no option of a step: every sweep that reads one runs the reweighting pass
// first and its route, whichever it is, reads the effective weights and products for the sweep's duration (AlsReweightGuard).  So does
// a logistic relation under cmf_set_logit_pass, which the routes then take for a Frobenius one.
struct AlsStepOpts { int nn_sweeps = 0, cg_steps = 0, nn_cg_steps = 0, dual_max = 0; bool biases = false; };

enum AlsRoute { ALS_SHARED_EXACT, ALS_SHARED_HALS, ALS_ROWS_EXACT, ALS_ROWS_NNLS, ALS_ROWS_CG, ALS_ROWS_NNCG, ALS_ROWS_DUAL };
// The route of one sweep: the table of cmf_als.hip.h, in its order of precedence.  The facts of the sweep: it has an observed
// relation; its rows share a term S (als_shared_present); it reads a logistic relation; k_pad; the factor is non-negative.
static AlsRoute als_route(bool observed, bool shared, bool logit, int kp, bool nn, const AlsStepOpts &o) {
    if (observed && nn && o.nn_cg_steps) return ALS_ROWS_NNCG;
    if (nn && o.nn_sweeps) return observed ? ALS_ROWS_NNLS : ALS_SHARED_HALS;
    if (!observed) return ALS_SHARED_EXACT;
    if (!nn && o.cg_steps) return ALS_ROWS_CG;
    return o.dual_max > 0 && !shared && !logit && kp > 32 ? ALS_ROWS_DUAL : ALS_ROWS_EXACT;   // (k_pad = 32: no class is below it)
}

// One bias sweep of relation `which` along `axis` (0 rows, 1 columns) into out (device, rows of that image): als_bias_piece_kernel
// over the piece lists of cmf_als_bias.hip.h.  Under a Huber loss the block is reweighted like a factor's rows: the pass refreshes the
// image of that axis at the current factors and biases, and the kernel reads w omega where it reads w.
static int als_bias_sweep(cmf_ctx *c, int which, int axis, float *out) {
    AlsBias &b = c->als_bias[which];
    CHK(als_bias_replan(c, which));
    const bool huber = als_huber_rel(c, which);
    if (huber) CHK(als_huber_refresh(c, which, axis));
    const WCsrDev &M = c->wm_sp[which][axis];
    const int64_t np = b.npieces[axis];
    CHK(ensure_scratch(c, c->als_bias_part, std::max<size_t>(16, (size_t)np * 2 * sizeof(double))));
    cmfk::AlsBiasArgs a{};
    als_entry_args(c, which, axis, b.pieces[axis], a);
    a.tv = M.tv; a.wv = huber ? M.hw : M.wv;
    a.other = axis == 0 ? b.c : b.r;
    a.mu = (float)b.mu;
    a.part = (double *)c->als_bias_part.p;
    Timed tm(c, CMF_K_KLMU, 2.0 * (double)M.nnz * (double)c->kp);
    if (np > 0) {
        const dim3 grid((unsigned)np), block(256);
        ALS_LAUNCH_GL(c, als_bias_piece_kernel, grid, block, 0, c->stream, a);
    }
    if (M.rows > 0)
        hipLaunchKernelGGL(cmfk::als_bias_combine_kernel, dim3((unsigned)((M.rows + 255) / 256)), dim3(256), 0, c->stream, (const double *)a.part,
                           (const int64_t *)b.first[axis], M.rows, b.lb, out);
    HIPCHK(hipGetLastError());
    return CMF_OK;
}

// The only place that sweeps: V, U, Z (cmf_solvers.py:248-263), each by its route; under biases the bias blocks after them.
static int als_step(cmf_ctx *c, const char *what, double l2, int nn_mask, int mask, const AlsStepOpts &o) {
    DeviceGuard dg(c->device);
    if (o.biases)
        for (int w = 0; w < 2; ++w) CHK(als_bias_refresh(c, w));   // (written when the biases last changed: nothing to do)
    const int bits[3] = {CMF_UPD_V, CMF_UPD_U, CMF_UPD_Z}, fs[3] = {CMF_V, CMF_U, CMF_Z};
    const int nnb[3] = {CMF_NN_V, CMF_NN_U, CMF_NN_Z};
    for (int s = 0; s < 3; ++s) {
        const int f = fs[s];
        if (!(mask & bits[s]) || c->frows[f] <= 0) continue;
        const bool nn = (nn_mask & nnb[s]) != 0;
        const AlsSweep sw = als_sweep(c, f);
        AlsReweightGuard reweighted(c);   // the Huber and passed-logistic sides of this sweep: refreshed from the current factors, bound until it is over
        CHK(reweighted.bind(sw));
        switch (als_route(als_observed(sw), als_shared_present(c, sw), als_logit_sweep(c, sw), c->kp, nn, o)) {
        case ALS_SHARED_EXACT: CHK(als_sweep_shared(c, what, sw, l2, nn)); break;
        case ALS_SHARED_HALS: CHK(als_nnls_sweep_shared(c, what, f, l2, o.nn_sweeps)); break;
        case ALS_ROWS_NNLS: CHK(als_rows_nnls(c, sw, l2, o.nn_sweeps)); break;
        case ALS_ROWS_CG: CHK(als_cg_rows(c, what, sw, l2, 0, c->frows[f], o.cg_steps, c->F[f], 0)); break;
        case ALS_ROWS_NNCG: CHK(als_cg_rows(c, what, sw, l2, 0, c->frows[f], o.nn_cg_steps, c->F[f], 0, true)); break;
        case ALS_ROWS_DUAL: {
            bool none = false;
            CHK(als_dual_rows(c, sw, l2, 0, c->frows[f], o.dual_max, nn, c->F[f], 0, &none));
            if (!none) break;
        }   // no row of the plan goes dual and nothing was launched: the exact sweep as it stands
            [[fallthrough]];
        case ALS_ROWS_EXACT:
            CHK(als_rows_solve(c, sw, l2));
            CHK(als_apply(c, f, (const float *)c->als_sol.p, nn));
            break;
        }
    }
    if (!o.biases) return CMF_OK;
    // r_x follows U, c_x and r_y follow V, c_y follows Z; r first, then c from the new r
    const int bit[2][2] = {{CMF_UPD_U, CMF_UPD_V}, {CMF_UPD_V, CMF_UPD_Z}};
    for (int w = 0; w < 2; ++w) {
        AlsBias &b = c->als_bias[w];
        if (!b.on) continue;
        for (int axis = 0; axis < 2; ++axis) {
            if (!(mask & bit[w][axis])) continue;
            CHK(als_bias_sweep(c, w, axis, axis == 0 ? b.r : b.c));
            b.dirty = true;
        }
        CHK(als_bias_refresh(c, w));   // the adjusted targets of the next step, and of cmf_als_residual_sq
    }
    return CMF_OK;
}

// ------------------------------------------------------------------ the step entry points: NEED_PROBLEM, the entry point's own checks
// under its own name, an AlsStepOpts, als_step.  None calls another.
static int als_check(cmf_ctx *c, const char *what, double l2, int mask) {
    if (!(l2 > 0.0) || !std::isfinite(l2)) return fail(CMF_EINVAL, "%s: l2 must be positive (a row with fewer than k observations is singular otherwise), got %g", what, l2);
    if (mask <= 0 || mask > 7) return fail(CMF_EINVAL, "%s: update_mask must name at least one of U, V, Z (got %d)", what, mask);
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "%s: n_components <= 256 only (k_pad = %d)", what, c->kp);
    CHK(als_logit_check(c, what, mask));
    CHK(als_huber_check(c, what, mask));
    if (mask & (CMF_UPD_U | CMF_UPD_V)) CHK(als_relation_ok(c, what, 0));
    if (mask & (CMF_UPD_Z | CMF_UPD_V)) CHK(als_relation_ok(c, what, 1));
    return CMF_OK;
}

// the range of a sweep or step count: lo .. 1024
static int als_count_ok(const char *what, const char *name, int n, int lo = 1) {
    if (n < lo || n > 1024) return fail(CMF_EINVAL, "%s: %s must be %d .. 1024, got %d", what, name, lo, n);
    return CMF_OK;
}

static int als_dual_max_ok(const char *what, int dual_max) {
    if (dual_max < 0 || dual_max > ALS_DUAL_MAX) return fail(CMF_EINVAL, "%s: dual_max must be 0 .. %d, got %d", what, (int)ALS_DUAL_MAX, dual_max);
    return CMF_OK;
}

// What the non-negative CG rows cannot sweep: a fused logistic relation (no reweighting pass) and a relation with biases bound
static int als_nncg_sweep_ok(cmf_ctx *c, const char *what, const AlsSweep &sw) {
    for (int s = 0; s < sw.nrel; ++s) {
        const int w = sw.rel[s].which;
        const char *nm = w == 0 ? "X" : "Y";
        if (als_logit_fused(c, w))
            return fail(CMF_EUNSUPPORTED, "%s: %s has a logistic loss; the non-negative conjugate-gradient rows have no reweighting pass: use cmf_als_nnls_step", what, nm);
        if (c->als_bias[w].on)
            return fail(CMF_EUNSUPPORTED, "%s: %s has biases bound; the non-negative conjugate-gradient rows under biases are not built: use cmf_als_bias_step", what, nm);
    }
    return CMF_OK;
}
// ... for every sweep of the step that nn_cg_steps > 0 puts on those rows (none: the step runs the routes that are left)
static int als_nncg_step_ok(cmf_ctx *c, const char *what, int nn_mask, int mask) {
    const int bits[3] = {CMF_UPD_U, CMF_UPD_V, CMF_UPD_Z}, nnb[3] = {CMF_NN_U, CMF_NN_V, CMF_NN_Z}, fs[3] = {CMF_U, CMF_V, CMF_Z};
    for (int s = 0; s < 3; ++s) {
        if (!(mask & bits[s]) || !(nn_mask & nnb[s]) || c->frows[fs[s]] <= 0) continue;
        const AlsSweep sw = als_sweep(c, fs[s]);
        if (als_observed(sw)) CHK(als_nncg_sweep_ok(c, what, sw));
    }
    return CMF_OK;
}

// the bias blocks are not built under a logit link
static int als_bias_logit_ok(cmf_ctx *c, const char *what, int mask) {
    if (als_logit_swept(c, mask))
        return fail(CMF_EUNSUPPORTED, "%s: a swept relation has a logistic loss (cmf_set_relation_loss); biases under a logit link are not built: "
                                      "use cmf_als_step or cmf_als_nnls_step", what);
    return CMF_OK;
}

extern "C" int cmf_als_step(cmf_ctx *c, double l2, int nn_mask, int mask) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_step", l2, mask));
    return als_step(c, "cmf_als_step", l2, nn_mask, mask, AlsStepOpts());
}

extern "C" int cmf_als_nnls_step(cmf_ctx *c, double l2, int nn_mask, int mask, int sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_nnls_step", l2, mask));
    CHK(als_count_ok("cmf_als_nnls_step", "sweeps", sweeps));
    AlsStepOpts o;
    o.nn_sweeps = sweeps;
    return als_step(c, "cmf_als_nnls_step", l2, nn_mask, mask, o);
}

extern "C" int cmf_als_cg_step(cmf_ctx *c, double l2, int nn_mask, int mask, int cg_steps, int nn_sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_cg_step", l2, mask));
    CHK(als_count_ok("cmf_als_cg_step", "cg_steps", cg_steps));
    CHK(als_count_ok("cmf_als_cg_step", "nn_sweeps", nn_sweeps, 0));
    CHK(als_logit_check(c, "cmf_als_cg_step", mask, true));
    AlsStepOpts o;
    o.nn_sweeps = nn_sweeps;
    o.cg_steps = cg_steps;
    return als_step(c, "cmf_als_cg_step", l2, nn_mask, mask, o);
}

// (no factor on the non-negative CG rows: nn_cg_steps selects nothing, and the step is cmf_als_cg_step's, cmf_als_nnls_step's or
// cmf_als_step's with the arguments that are left)
extern "C" int cmf_als_nncg_step(cmf_ctx *c, double l2, int nn_mask, int mask, int cg_steps, int nn_cg_steps, int nn_sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_nncg_step", l2, mask));
    CHK(als_count_ok("cmf_als_nncg_step", "cg_steps", cg_steps, 0));
    CHK(als_count_ok("cmf_als_nncg_step", "nn_cg_steps", nn_cg_steps));
    CHK(als_count_ok("cmf_als_nncg_step", "nn_sweeps", nn_sweeps, 0));
    CHK(als_nncg_step_ok(c, "cmf_als_nncg_step", nn_mask, mask));
    if (cg_steps) CHK(als_logit_check(c, "cmf_als_nncg_step", mask, true));
    AlsStepOpts o;
    o.nn_sweeps = nn_sweeps;
    o.cg_steps = cg_steps;
    o.nn_cg_steps = nn_cg_steps;
    return als_step(c, "cmf_als_nncg_step", l2, nn_mask, mask, o);
}

// (no biases bound: cmf_als_cg_step's step, or with cg_steps = 0 cmf_als_nnls_step's / cmf_als_step's)
extern "C" int cmf_als_bias_step(cmf_ctx *c, double l2, int nn_mask, int mask, int cg_steps, int nn_sweeps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_bias_step", l2, mask));
    CHK(als_count_ok("cmf_als_bias_step", "cg_steps", cg_steps, 0));
    CHK(als_count_ok("cmf_als_bias_step", "nn_sweeps", nn_sweeps, 0));
    CHK(als_bias_logit_ok(c, "cmf_als_bias_step", mask));
    AlsStepOpts o;
    o.nn_sweeps = nn_sweeps;
    o.cg_steps = cg_steps;
    o.biases = als_bias_any(c);
    return als_step(c, "cmf_als_bias_step", l2, nn_mask, mask, o);
}

// (there is no cg_steps: CG would take every sweep the dual route could)
extern "C" int cmf_als_dual_step(cmf_ctx *c, double l2, int nn_mask, int mask, int dual_max, int nn_sweeps, int nn_cg_steps) {
    NEED_PROBLEM(c);
    CHK(als_check(c, "cmf_als_dual_step", l2, mask));
    CHK(als_dual_max_ok("cmf_als_dual_step", dual_max));
    CHK(als_count_ok("cmf_als_dual_step", "nn_sweeps", nn_sweeps, 0));
    CHK(als_count_ok("cmf_als_dual_step", "nn_cg_steps", nn_cg_steps, 0));
    if (nn_cg_steps && als_bias_any(c))
        return fail(CMF_EUNSUPPORTED, "cmf_als_dual_step: nn_cg_steps with biases bound is not built (cmf_als_nncg_step): pass nn_cg_steps = 0");
    if (nn_cg_steps) CHK(als_nncg_step_ok(c, "cmf_als_dual_step", nn_mask, mask));
    if (als_bias_any(c)) CHK(als_bias_logit_ok(c, "cmf_als_dual_step", mask));
    AlsStepOpts o;
    o.nn_sweeps = nn_sweeps;
    o.nn_cg_steps = nn_cg_steps;
    o.dual_max = dual_max;
    o.biases = als_bias_any(c);
    return als_step(c, "cmf_als_dual_step", l2, nn_mask, mask, o);
}

// ------------------------------------------------------------------ test entries
// the bias block a step would write along `axis` of relation `which`, the biases left alone
extern "C" int cmf_als_bias_rows(cmf_ctx *c, int which, int axis, float *host_out) {
    NEED_PROBLEM(c);
    float *vec; int64_t n;
    CHK(als_bias_vector(c, "cmf_als_bias_rows", which, axis, &vec, &n));
    CHK(als_huber_rel_ok(c, "cmf_als_bias_rows", which));   // (a Huber relation: the states every step refuses)
    if (!host_out && n > 0) return fail(CMF_EINVAL, "cmf_als_bias_rows: null output");
    DeviceGuard dg(c->device);
    CHK(ensure_scratch(c, c->als_bias_ws, std::max<size_t>(16, (size_t)n * sizeof(float))));
    CHK(als_bias_sweep(c, which, axis, (float *)c->als_bias_ws.p));
    if (n) HIPCHK(hipMemcpyAsync(host_out, c->als_bias_ws.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

// The row test entries: the rows a route would write for rows [row0, row0 + nrows) of sweep `which`, the factors left alone.
// check(sw): the route's own refusals, of its arguments (sw == null: before the range check) and of the sweep (after it); run(sw,
// out): the rows into out, where row r goes to out + (r - row0) k_pad.
template <class Check, class Run>
static int als_rows_entry(cmf_ctx *c, const char *what, int which, int64_t row0, int64_t nrows, double l2, float *host_f, Check check, Run run) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "%s: bad factor selector", what);
    CHK(als_check(c, what, l2, 1 << which));
    CHK(check(nullptr));
    if (row0 < 0 || nrows < 0 || row0 + nrows > c->frows[which]) return fail(CMF_EINVAL, "%s: rows out of range", what);
    const AlsSweep sw = als_sweep(c, which);
    CHK(check(&sw));
    if (nrows == 0) return CMF_OK;
    if (!host_f) return fail(CMF_EINVAL, "%s: null output", what);
    DeviceGuard dg(c->device);
    const size_t bytes = (size_t)nrows * c->kp * sizeof(float);
    CHK(ensure_scratch(c, c->als_cg_ws, bytes));
    HIPCHK(hipMemsetAsync(c->als_cg_ws.p, 0, bytes, c->stream));
    AlsReweightGuard reweighted(c);
    CHK(reweighted.bind(sw));
    CHK(run(sw, (float *)c->als_cg_ws.p));
    HIPCHK(hipMemcpyAsync(host_f, c->als_cg_ws.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}
static int als_rows_observed(const char *what, const AlsSweep &sw) {
    if (!als_observed(sw)) return fail(CMF_EINVAL, "%s: this sweep has no observed relation: one shared matrix, no per-row systems", what);
    return CMF_OK;
}

extern "C" int cmf_als_cg_rows(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, int cg_steps, float *host_f) {
    const char *what = "cmf_als_cg_rows";
    return als_rows_entry(c, what, which, row0, nrows, l2, host_f, [&](const AlsSweep *sw) -> int {
        if (sw) return als_rows_observed(what, *sw);
        CHK(als_count_ok(what, "cg_steps", cg_steps));
        return als_logit_check(c, what, 1 << which, true);
    }, [&](const AlsSweep &sw, float *out) { return als_cg_rows(c, what, sw, l2, row0, row0 + nrows, cg_steps, out, row0); });
}

extern "C" int cmf_als_nncg_rows(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, int nn_cg_steps, float *host_f) {
    const char *what = "cmf_als_nncg_rows";
    return als_rows_entry(c, what, which, row0, nrows, l2, host_f, [&](const AlsSweep *sw) -> int {
        if (!sw) return als_count_ok(what, "nn_cg_steps", nn_cg_steps);
        CHK(als_rows_observed(what, *sw));
        return als_nncg_sweep_ok(c, what, *sw);
    }, [&](const AlsSweep &sw, float *out) { return als_cg_rows(c, what, sw, l2, row0, row0 + nrows, nn_cg_steps, out, row0, true); });
}

// (an eligible sweep; k_pad = 32: every row with an entry is a formed one)
extern "C" int cmf_als_dual_rows(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, int dual_max, float *host_f) {
    const char *what = "cmf_als_dual_rows";
    return als_rows_entry(c, what, which, row0, nrows, l2, host_f, [&](const AlsSweep *sw) -> int {
        if (!sw) return als_dual_max_ok(what, dual_max);
        if (const char *why = als_dual_why_not(c, *sw)) return fail(CMF_EINVAL, "%s: this sweep is not eligible: %s", what, why);
        return CMF_OK;
    }, [&](const AlsSweep &sw, float *out) -> int {
        for (int s = 0; s < sw.nrel; ++s) CHK(als_bias_refresh(c, sw.rel[s].which));   // (written when the biases last changed: nothing to do)
        return als_dual_rows(c, sw, l2, row0, row0 + nrows, dual_max, false, out, row0);
    });
}

// the long rows and the pieces of the last CG sweep (or cmf_als_cg_rows call)
extern "C" int cmf_als_cg_last(cmf_ctx *c, int64_t *out2) {
    if (!c || !out2) return fail(CMF_EINVAL, "cmf_als_cg_last: null context or output");
    out2[0] = c->als_cg_last[0];
    out2[1] = c->als_cg_last[1];
    return CMF_OK;
}

// the long rows and the pieces of the last non-negative CG sweep (or cmf_als_nncg_rows call); the passes its rows ran and the
// stored entries those passes read
extern "C" int cmf_als_nncg_last(cmf_ctx *c, int64_t *out2) {
    if (!c || !out2) return fail(CMF_EINVAL, "cmf_als_nncg_last: null context or output");
    out2[0] = c->als_nncg_last[0];
    out2[1] = c->als_nncg_last[1];
    return CMF_OK;
}
extern "C" int cmf_als_nncg_passes(cmf_ctx *c, int64_t *out2) {
    if (!c || !out2) return fail(CMF_EINVAL, "cmf_als_nncg_passes: null context or output");
    DeviceGuard dg(c->device);
    CHK(als_nncg_count(c));
    out2[0] = c->als_nncg_last[2];
    out2[1] = c->als_nncg_last[3];
    return CMF_OK;
}

// rows in class 32, 64 and 128, rows left to the formed route and rows written as zeros in the last dual sweep (or cmf_als_dual_rows call)
extern "C" int cmf_als_dual_last(cmf_ctx *c, int64_t *out5) {
    if (!c || !out5) return fail(CMF_EINVAL, "cmf_als_dual_last: null context or output");
    for (int q = 0; q < 5; ++q) out5[q] = c->als_dual_last[q];
    return CMF_OK;
}

// test entry: the kernel on the caller's systems (cmf_als_normal's layout), f in / out
extern "C" int cmf_als_nnls_rows(cmf_ctx *c, int64_t nrows, const float *host_H, const float *host_g, float *host_f, int sweeps) {
    NEED_PROBLEM(c);
    if (!host_H || !host_g || !host_f || nrows < 0) return fail(CMF_EINVAL, "cmf_als_nnls_rows: null pointer or negative row count");
    CHK(als_count_ok("cmf_als_nnls_rows", "sweeps", sweeps));
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_als_nnls_rows: n_components <= 256 only (k_pad = %d)", c->kp);
    if (nrows == 0) return CMF_OK;
    DeviceGuard dg(c->device);
    const int64_t kp = c->kp, nh = nrows * kp * kp, nv = nrows * kp;
    CHK(ensure_scratch(c, c->als_nnls_ws, (size_t)(nh + 2 * nv) * sizeof(float)));
    float *H = (float *)c->als_nnls_ws.p, *g = H + nh, *f = g + nv;
    HIPCHK(hipMemcpyAsync(H, host_H, (size_t)nh * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g, host_g, (size_t)nv * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(f, host_f, (size_t)nv * sizeof(float), hipMemcpyHostToDevice, c->stream));
    CHK(als_nnls_launch(c, H, g, f, nullptr, nrows, sweeps));
    HIPCHK(hipMemcpyAsync(host_f, f, (size_t)nv * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return CMF_OK;
}

extern "C" int cmf_als_normal(cmf_ctx *c, int which, int64_t row0, int64_t nrows, double l2, float *host_H, float *host_g) {
    NEED_PROBLEM(c);
    if (which < 0 || which > 2) return fail(CMF_EINVAL, "cmf_als_normal: bad factor selector");
    CHK(als_check(c, "cmf_als_normal", l2, 1 << which));
    if (row0 < 0 || nrows < 0 || row0 + nrows > c->frows[which]) return fail(CMF_EINVAL, "cmf_als_normal: rows out of range");
    const AlsSweep sw = als_sweep(c, which);
    if (!als_observed(sw)) return fail(CMF_EINVAL, "cmf_als_normal: this sweep has no observed relation: one shared matrix, no per-row systems");
    if (nrows == 0) return CMF_OK;
    DeviceGuard dg(c->device);
    AlsReweightGuard reweighted(c);
    CHK(reweighted.bind(sw));
    return als_rows_to_host(c, sw, l2, row0, row0 + nrows, host_H, host_g);
}

extern "C" int cmf_als_layout(cmf_ctx *c, int64_t *out4) {
    NEED_PROBLEM(c);
    if (!out4) return fail(CMF_EINVAL, "cmf_als_layout: null output");
    if (c->kp > 256) return fail(CMF_EUNSUPPORTED, "cmf_als_layout: n_components <= 256 only (k_pad = %d)", c->kp);
    DeviceGuard dg(c->device);
    out4[0] = als_piece_len(c);
    const int fs[3] = {CMF_U, CMF_V, CMF_Z};
    for (int s = 0; s < 3; ++s) {
        const AlsSweep sw = als_sweep(c, fs[s]);
        AlsPlan pl;
        if (als_observed(sw)) CHK(als_plan(c, sw, 0, c->frows[fs[s]], pl));
        out4[1 + s] = (int64_t)pl.pieces.size();
    }
    return CMF_OK;
}

#endif // CMF_ALS_HOST
