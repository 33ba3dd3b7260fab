/*
 * cmfhip.h -- C ABI of libcmfhip.so: the MI355X (gfx950) factor-update engine
 * for collective matrix factorisation  X ~ f(U V^T),  Y ~ f(V Z^T).
 *
 * The reference (smn-ailab/PyCMF) has no FFI on this path: its seam is the
 * Python solver object built at pycmf/cmf.py:437-451 and driven through
 * `fit_iterative_update` (pycmf/cmf.py:454 -> pycmf/cmf_solvers.py:132-195),
 * whose body is `update_step` (:172).  The closest thing to a native ABI is the
 * (dead) Cython module pycmf/cmf_newton_solver.pyx (`_newton_update_left`
 * :240-292, `_newton_update_V` :295-362).  The entry points below are what a
 * binding for that seam needs; each cites the reference code it replaces.
 *
 * Conventions
 *   - every function returns 0 on success or a CMF_E* code; the message is
 *     available from cmf_last_error() (thread-local).
 *   - host matrices are caller-owned, any element strides (in elements), read
 *     only unless stated.  Device state is owned by the context.
 *   - arithmetic on the device is float32 (north_star); host I/O is float64
 *     or float32.
 *   - one context drives one GPU from one host thread; contexts are not
 *     thread-safe.  With several GPUs use one process + one context per GPU
 *     and the *_partials / *_apply pair around an all-reduce (section "sharded").
 */
#ifndef CMFHIP_H
#define CMFHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cmf_ctx cmf_ctx;

enum {
    CMF_OK = 0,
    CMF_EINVAL = 1,   /* bad argument / wrong call order            */
    CMF_EHIP = 2,     /* a HIP runtime call failed                  */
    CMF_ENOMEM = 3,   /* device or host allocation failed           */
    CMF_ENODEV = 4,   /* no usable gfx950 device                    */
    CMF_EUNSUPPORTED = 5,
    CMF_ERCCL = 6     /* RCCL missing or a collective failed         */
};

enum { CMF_U = 0, CMF_V = 1, CMF_Z = 2 };           /* factor selector          */
enum { CMF_LINK_LINEAR = 0, CMF_LINK_LOGIT = 1 };   /* cmf_solvers.py:27-33     */
enum { CMF_UPD_U = 1, CMF_UPD_V = 2, CMF_UPD_Z = 4 }; /* update_U/V/Z, :252-261 */
enum { CMF_NN_U = 1, CMF_NN_V = 2, CMF_NN_Z = 4 };  /* *_non_negative, :321-326 */

/* kernel classes for cmf_kernel_time() */
enum {
    CMF_K_GEMM_NN = 0,   /* C = A   B over a data-sized A: X V, Y Z, R V, W KR   */
    CMF_K_GEMM_TN = 1,   /* C = A^T B over a data-sized A: X^T U, Y^T V, R^T U   */
    CMF_K_GEMM_NT = 2,   /* f(L R^T) - T : residual / error    */
    CMF_K_ELEMWISE = 3,  /* slab sums, MU ratio, row updates   */
    CMF_K_EIGEN = 4,     /* batched symmetric Jacobi           */
    CMF_K_GEMM_SMALL = 5,/* factor-side products: Grams, F G, grad H^-1 */
    CMF_K_SPMM = 6,      /* native CSR: A F, A^T F, sum_nnz a_ij (l_i . r_j)  */
    CMF_K_ROWHESS = 7,   /* fused per-row gradient + Hessian over the sampled rows */
    CMF_K_GEMM_PAIR = 8, /* k_pad = 128: the two data passes of an MU half-iteration as one balanced launch (X^T U with Y Z, X V with Y^T V) */
    CMF_K_TOPK = 9,      /* prediction: top-n of f(Q B^T), scores on the fp32 matrix pipe + per-row selection + merge; flops 2 nq C k */
    CMF_K_KLMU = 10,     /* Kullback-Leibler MU: fused quotient passes (T ./ (A B^T)) B, both products on the fp32 matrix pipe, and the divergence; flops 4 rows cols k per dense pass */
    CMF_K_COUNT = 11
};
/* CMF_K_COUNT is FROZEN at the eleven classes above (callers size their tables by it) and no longer counts the classes: the real
 * bound is CMF_K_END -- cmf_kernel_time accepts every class below it.  A new class goes into THIS enum, numbered on, and moves
 * CMF_K_END; the first enum does not change again.                                                                         */
enum {
    CMF_K_HALS = 11,     /* HALS sweeps (hals_sweep_kernel): F G[:, b] on the fp32 matrix pipe + the sequential part of a coordinate block; flops 2 rows k^2 per sweep */
    CMF_K_END = 12
};

const char *cmf_last_error(void);
/* sha256 of the sources the library was built from (everything under csrc/ and this header): pycmf_amd/_lib.py refuses a library whose stamp differs
 * from the sources next to it                                                                                                   */
const char *cmf_source_hash(void);
int cmf_device_count(int *count);

/* ---- context ---------------------------------------------------------- */
/* `stream` is a hipStream_t the caller already owns (e.g. torch's current
 * stream) or NULL for a context-private stream.                            */
int cmf_ctx_create(cmf_ctx **out, int device, void *stream);
int cmf_ctx_destroy(cmf_ctx *ctx);
int cmf_sync(cmf_ctx *ctx);
/* tuning knobs (A/B measurements in one process): "gemm_split" n = force the split-K factor (<= 0: heuristic),
 * "data_pass_wg" bits: the fp32 data passes with a 256-wide factor (k_pad = 256) run on the 256-thread workgroup with 128 x 128
 * wave tiles (cmf_gemm_wg256.hip.h) -- bit 0 the TN form (X^T U, Y^T V: X feeds the MFMAs from registers), bit 1 the NN form
 * (X V, Y Z); 3 both, 0 both on the 512-thread kernel; bit 2 (acts with bit 0) the TN form takes the factor from a second register
 * ring as well: no LDS, no barrier; bit 3 (acts with bit 1) the NN form does, X alone stays in LDS.  15 (default): all of them.
 * Same accumulation order: the results do not depend on it, bit for bit,
 * "sparse_mode" 0 auto | 1 dense | 2 native CSR (set before cmf_set_data_csr),
 * "row_kernel" 1 fused gather kernel | 0 masked-dense GEMMs for per-row Newton sweeps,
 * "z_logit_hessian_l2" 1 (live Python path, cmf_solvers.py:505-506) | 0 (Cython twin,
 * cmf_newton_solver.pyx:287-290: Z's logit Hessian without l2 I),
 * "safe_inverse_cholesky" 1 | 0, "graph" 1 | 0 (replay MU / linear-Newton steps from a
 * captured hipGraph; automatically off while cmf_kernel_timing is enabled),
 * "gemm_arith" 0 (fp32 MFMA, default) | 1 (k_pad = 256 data passes on the bf16 matrix pipe: every fp32 operand
 * split exactly into three bf16 planes, six cross products, fp32 accumulation; planes stay resident),
 * "row_symmetric" 4 (default) | 3 | 1 | 0 (k_pad = 256 row kernel: 0 every 32 x 32 block of H_i | 1 the blocks on or above the block
 * diagonal, raw and weighted sample images | 3 ... from one sqrt-weighted image | 4 ... with the 8 diagonal blocks as three 16 x 16
 * sub-blocks each),
 * "eig_clamp" 1 (default) | 0 | 3, "rank1_clamp" 1 (default) | 0, "refine_rows_tol_ppm" 20 (default): how the rows flagged by the
 * threshold test of _safe_invert (cmf_solvers.py:346-356) are served (cmf_newton_clamp_routes below) and which of them are redone
 * in float64 (cmf_newton_clamp_stats below),
 * "shared_hessian_f64" 1 (default) | 0: the single Hessian of a linear-link sweep is accumulated (float64 Grams on
 * the float64 matrix pipe) and inverted in float64 | float32 Grams and float32 inverse,
 * "newton_schulz" 1 | 0 (k_pad = 256: rows whose eigenvalue clamp acts go through the GEMM-only
 * spectral clamp | through the Jacobi eigen-solver),
 * "sample_row_offset_u|v|z" n = global index of this context's first U / V / Z row in the keys of
 * the device sampler (a row shard then draws what the unsharded problem draws for its rows),
 * "row_classes" -1 (automatic, default) | 0 | 2..6: linear-link sides with sg_sample_ratio < 1 -- groups of that many
 * consecutive rows share the outer-product sums of the samples they have in common (same H_i as row by row, sums in
 * another order; cmf_solvers.py:414-428 with the identity link) | every row gathers its own list,
 * "direct_newton_step" 1 (default) | 0: linear shared-Hessian sweeps with l1 = 0 whose inverse is the plain one (k > 64)
 * update F <- clamp(s (T O) H^-1) in one product | form the gradient and subtract the step,
 * "row_certificates" 1 (default) | 0: half such a group shares one threshold test of _safe_invert (cmf_solvers.py:346-356)
 * through the positive semi-definite part of their Hessians the rows have in common | every row runs its own,
 * "topk_split" n: cmf_topk / cmf_topk_queries cut the candidates into n shares (<= 0, default: as many as fill the chip); the
 * result does not depend on it.  The same option fixes the shares of cmf_rank / cmf_rank_queries, whose result does not depend on
 * it either,
 * "kl_split" n: the dense passes of cmf_mu_kl_step / cmf_kl_divergence cut the streamed dimension into n shares (<= 0, default:
 * enough to give every CU a workgroup); another n regroups the float32 sums,
 * "als_piece" n: stored entries per piece of a row in the normal-equation kernel of cmf_als_step (<= 0, default: 4096; rounded up
 * to a multiple of 32); another n regroups the float32 sums,
 * "als_cg_piece" n: stored entries per piece of a LONG row of cmf_als_cg_step -- a row with more than n stored entries (both
 * sides of a V sweep counted together) is cut into pieces of n, each summed by a workgroup of its own (n > 0: rounded up to a
 * multiple of 16; 0, default: 2048; n < 0: no row is ever cut, every row is walked by one workgroup); another n regroups the
 * float32 sums of the rows longer than the smaller of the two                                                                */
int cmf_set_option(cmf_ctx *ctx, const char *name, int64_t value);

/* ---- problem ---------------------------------------------------------- */
/* Local shard sizes: X is m x d, Y is d x p, factors have k columns.
 * (pycmf/cmf_solvers.py:132-160 argument shapes).  Allocates device state. */
int cmf_set_problem(cmf_ctx *ctx, int64_t m, int64_t d, int64_t p, int k);

/* Dense uploads; element (i,j) is at ptr[i*rs + j*cs].  which: 0 = X, 1 = Y.
 * Replaces the implicit "X, Y are ndarrays" of cmf_solvers.py:132.          */
int cmf_set_data_f64(cmf_ctx *ctx, int which, const double *ptr, int64_t rs, int64_t cs);
int cmf_set_data_f32(cmf_ctx *ctx, int which, const float *ptr, int64_t rs, int64_t cs);
/* CSR upload (scipy layout), accept_sparse=('csr','csc') of pycmf/cmf.py:679;
 * CSC is converted by the caller.  Large, genuinely sparse inputs (density < 2 %,
 * dense image > 1 GB) stay CSR on the device (A and A^T images, SpMM kernels);
 * others are expanded to the dense layout.  cmf_set_option("sparse_mode", 1|2)
 * forces dense | native.                                                     */
int cmf_set_data_csr(cmf_ctx *ctx, int which, const int64_t *indptr, const int32_t *indices,
                     const double *data, int64_t nnz);
/* Synthetic |N(0,1)| fill on the device (counter-based; value of element
 * (gi,gj) depends only on seed and its GLOBAL coordinates, so a shard can be
 * generated in place): rows [row0,row0+rows) x cols [col0,col0+cols) of the
 * global matrix land in the local matrix.  Used by bench.py.                 */
/* representation of X / Y on the device: *dense = a dense float32 image exists, *native = the CSR pair (A, A^T) is resident */
int cmf_data_layout(cmf_ctx *ctx, int which, int *dense, int *native);
/* layout of the column-blocked SpMM images of a native sparse X / Y (the products safe_sparse_dot runs at cmf_solvers.py:232, :244):
 * out[0..3] = row groups, rows cut into pieces (more non-zeros than a wave's share of a group), pieces, accumulator rows per group --
 * of A; out[4..7] the same of A^T.  Zeros where an orientation has no blocked image.                                          */
int cmf_sparse_layout(cmf_ctx *ctx, int which, int64_t *out8);
/* rows x cols block of the dense device image into a packed host array (parity tests at full BASELINE sizes) */
int cmf_get_data_block_f32(cmf_ctx *ctx, int which, int64_t row0, int64_t nrows, int64_t col0, int64_t ncols, float *host_dst);
int cmf_fill_data_synthetic(cmf_ctx *ctx, int which, uint64_t seed, int64_t row0, int64_t col0);
int cmf_fill_factor_synthetic(cmf_ctx *ctx, int which, uint64_t seed, int64_t row0, double scale);
/* the same generator with the target distributions of the logit workloads: kind 0 = |N(0,1)|,
 * 1 = sigmoid(N(0,1)) (benchmarks/benchmark_cmf.py:78), 2 = Bernoulli(param) in {0, 1} (samples/toxic_comments.ipynb labels) */
int cmf_fill_data_synthetic_kind(cmf_ctx *ctx, int which, uint64_t seed, int64_t row0, int64_t col0, int kind, double param);
/* out (host, rows_out x ncols, row-major float64) = op(A) * B with A = X (which 0) or Y (which 1),
 * op = transpose when trans != 0, B host row-major float64 (b_rows x ncols).  The big products of the
 * initialisers' randomized SVD (sklearn randomized_svd called at pycmf/cmf.py:126,:149) run through
 * this on the data already resident on the device (dense MFMA GEMM or native CSR SpMM).            */
int cmf_data_matmul_f64(cmf_ctx *ctx, int which, int trans, const double *B, int64_t b_rows, int ncols, double *out);
/* Initialisers on the device copy (pycmf/cmf.py:41-202).
 * cmf_rsvd: randomized truncated SVD of X (which 0) or Y (which 1) as sklearn.utils.extmath.randomized_svd computes it for
 * _initialize_mf (cmf.py:126, :149): `omega` is the Gaussian test matrix (cols x size row-major float64 when transpose == 0,
 * rows x size when transpose != 0 -- sklearn's 'auto' transposition -- drawn by the caller from NumPy's RandomState),
 * n_iter normalised power iterations (CholeskyQR2 in float64 in place of sklearn's LU: the same subspace), then the SVD of
 * the small matrix.  Outputs, float64 row-major: U (rows x k), S (k), Vt (k x cols).  Sign convention left to the caller.
 * cmf_data_sum: sum of all entries of X and Y (M.mean() of the 'random' / 'nndsvda' / 'nndsvdar' rules, cmf.py:111, :186). */
int cmf_rsvd(cmf_ctx *ctx, int which, int transpose, int k, int size, int n_iter, const double *omega,
             double *U, double *S, double *Vt);
int cmf_data_sum(cmf_ctx *ctx, double *sum_x, double *sum_y);
/* float64 sums of the dense device image of X / Y over blocks of 256 rows (axis 0: out[rows_pad / 256][cols_pad]) or 256 columns
 * (axis 1: out[rows_pad][cols_pad / 256]): the inputs of the per-tile checksums of the full-size parity tests -- the column sums
 * of a 256-row output tile of X^T U, X V, Y Z, Y^T V (cmf_solvers.py:232, :238, :244) are (block sums)^T times the factor        */
int cmf_data_block_sums_f64(cmf_ctx *ctx, int which, int axis, double *out);
/* read back a block of X or Y (tests) */
int cmf_get_data_f32(cmf_ctx *ctx, int which, float *ptr, int64_t rs, int64_t cs);

/* Factors (in/out, pycmf/cmf_solvers.py:195 "return U, V, Z" after in-place
 * mutation :255,:259,:263,:324).                                             */
int cmf_set_factor_f64(cmf_ctx *ctx, int which, const double *ptr, int64_t rs, int64_t cs);
int cmf_get_factor_f64(cmf_ctx *ctx, int which, double *ptr, int64_t rs, int64_t cs);

/* ---- MU solver: MUSolver.update_step, pycmf/cmf_solvers.py:248-263 ----- */
int cmf_mu_step(cmf_ctx *ctx, double l1, double l2, int update_mask);
/* cmf_mu_step AND the error metric of the factors it leaves (compute_factorization_error, cmf_solvers.py:36-42, as the loop
 * evaluates it every 10th iteration, :175-187) from the products of the step itself: ||X||^2 - 2 <U, X V> + <U^T U, V^T V> (the
 * expansion of sklearn's sparse path, :40) -- no pass over X and Y.  Falls back to cmf_residual_sq per side where the expansion
 * would cancel (e^2 < 1e-3 ||.||^2), the side is not dense or its factor is not updated.  *ex2 / *ey2 (nullable): squared
 * Frobenius residuals of the local shard, as cmf_residual_sq.                                                              */
int cmf_mu_step_error(cmf_ctx *ctx, double l1, double l2, int update_mask, double *ex2, double *ey2);

/* ---- MU solver, generalised Kullback-Leibler objective --------------------------------------------------------------------
 * The reference documents beta_loss='kullback-leibler' and does not implement it (pycmf/cmf.py:245-247).  Here:
 *   minimise  D(X || U V^T) + D(Y || V Z^T) + l1 (sum U + sum V + sum Z) + l2 / 2 (|U|^2 + |V|^2 + |Z|^2),
 *   D(T || S) = sum_{t > 0} t log(t / s) - sum t + sum s        (unweighted, like the reference's MU objective)
 * by sklearn's multiplicative update for beta_loss = 1 applied to each block, in the reference's sweep order V, U, Z
 * (cmf_solvers.py:248-263).  With EPS = 2^-23 and Q(T, A, B) = T ./ max(A B^T, EPS) (a zero of T gives an exact 0):
 *   V <- V .* [Q(X,U,V)^T U + Q(Y,V,Z) Z] ./ reg(colsum U + colsum Z, V)
 *   U <- U .* [Q(X,U,V) V] ./ reg(colsum V, U)     (new V)            Z <- Z .* [Q(Y,V,Z)^T V] ./ reg(colsum V, Z)
 *   reg(den, F) = den + l1 + l2 F, then den == 0 -> EPS               (cmf_solvers.py:212-228 with gamma = 1)
 * PRECONDITION: non-negative data and factors (not checked here; the Python layer refuses negative data).
 * The quotient is never materialised (csrc/cmf_klmu.hip.h): dense data go through a fused two-product kernel on the fp32 matrix
 * pipe, native CSR data (cmf_data_layout) through a fused gather kernel over the stored entries only; X and Y may differ in
 * layout.  No floating-point atomics: a repeated call from the same state is bit-identical.  Option "gemm_arith" has no effect
 * here.  k_pad > 256 (n_components above 256): CMF_EUNSUPPORTED.  A sweep whose data matrix has not been set: CMF_EINVAL.
 * The call leaves every option, captured graph and buffer of the Frobenius path as it was.  cmf_run is not extended: a KL fit
 * keeps its loop on the host.
 *   cmf_kl_divergence: *dx = D(X || U V^T), *dy = D(Y || V Z^T) of the factors on the device (either may be NULL), float32 per
 *   element, float64 accumulation; a native CSR side is evaluated as sum over the stored entries + colsum(A) . colsum(B)
 *   (sklearn's sparse branch of _beta_divergence) without a dense image.
 *   cmf_mu_kl_layout: out4 = { shares S of the streamed dimension in the U sweep, in the V sweep (the larger of its two passes),
 *   in the Z sweep; device scratch bytes of a full step (numerator slabs + column sums) }.  S = 1 for a native CSR side.       */
int cmf_mu_kl_step(cmf_ctx *ctx, double l1, double l2, int update_mask);
int cmf_kl_divergence(cmf_ctx *ctx, double *dx, double *dy);
int cmf_mu_kl_layout(cmf_ctx *ctx, int64_t *out4);

/* ---- MU solver, beta-divergence objective (0 <= beta <= 2) -------------------------------------------------------------------
 *   minimise  D_beta(X || U V^T) + D_beta(Y || V Z^T) + l1 (sum U + sum V + sum Z) + l2 / 2 (|U|^2 + |V|^2 + |Z|^2)
 *   d_beta(t | s) = (t^beta + (beta - 1) s^beta - beta t s^(beta - 1)) / (beta (beta - 1));  beta = 0 (Itakura-Saito):
 *   t / s - log(t / s) - 1;  beta = 1: the Kullback-Leibler term above;  t = 0: s^beta / beta
 * by sklearn's multiplicative update for that beta_loss applied to each block, sweep order V, U, Z with the new V for U and Z.
 * With EPS = 2^-23, S = A B^T and P = max(S, EPS)^(beta - 2):
 *   num = (T .* P) B      den = (S .* P) B      F <- F .* (num / reg(den, F))^gamma
 *   gamma = 1 / (2 - beta) for beta < 1, 1 for 1 <= beta <= 2          reg(den, F) = den + l1 + l2 F, then den == 0 -> EPS
 * (den takes the unclamped S: it equals sklearn's max(S, EPS)^(beta - 1) wherever S >= EPS, and an all-zero row gives an exact 0).
 * PRECONDITION: non-negative data and factors, and no zero in the data at beta = 0 (not checked here; the Python layer refuses both).
 * Both products of a sweep come from ONE pass over A B^T with two accumulator sets (csrc/cmf_betamu.hip.h; 6 m d k flops, against
 * 8 m d k for two passes); S .* P is never materialised.  Dense images only: a relation held only as native CSR gives
 * CMF_EUNSUPPORTED (give it a dense image, sparse_mode 1), and so do bound entry weights, a background weight or biases on a relation
 * the call reads, and k_pad > 256.  beta outside [0, 2], or a sweep whose data has not been set: CMF_EINVAL.  The context stays usable
 * after each refusal.  No floating-point atomics: a repeated call from the same state is bit-identical.  The call leaves every option,
 * captured graph and buffer of the other steps as it was; cmf_run is not extended.
 *   cmf_beta_divergence: *dx = D_beta(X || U V^T) = sum over the valid cells of d_beta(t | max(s, EPS)), *dy likewise (either may be
 *   NULL); terms in float32, float64 accumulation.
 *   cmf_mu_beta_products: the two products of one sweep (0 = U, 1 = V, 2 = Z) from the factors on the device into host buffers of
 *   rows x k_pad floats each (rows of that factor), the slabs of the shares summed in slab order; nothing is updated (tests, the
 *   timing tool).
 *   cmf_mu_beta_layout: out4 as cmf_mu_kl_layout (option "kl_split" forces the shares here too); the scratch is the numerator and
 *   denominator slabs, twice the KL step's.  Option "beta_route" 0 (default: the route the width ships) | 1 the dual-output pass |
 *   2 two single-output passes.                                                                                                   */
int cmf_mu_beta_step(cmf_ctx *ctx, double beta, double l1, double l2, int update_mask);
int cmf_beta_divergence(cmf_ctx *ctx, double beta, double *dx, double *dy);
int cmf_mu_beta_products(cmf_ctx *ctx, double beta, int sweep, float *num, float *den);
int cmf_mu_beta_layout(cmf_ctx *ctx, int64_t *out4);

/* ---- MU solver, Frobenius objective with per-entry weights ---------------------------------------------------------------
 * The reference lists "Add support for weight matrices on relations" as an open item (its README).  Here, with fixed
 * non-negative Wx (m x d) and Wy (d x p) -- a 0/1 mask restricts the loss to the observed entries:
 *   minimise  1/2 |sqrt(Wx) .* (X - U V^T)|^2 + 1/2 |sqrt(Wy) .* (Y - V Z^T)|^2 + l1 (sum U + sum V + sum Z) + l2 / 2 (|U|^2 + |V|^2 + |Z|^2)
 *   V <- V .* [(Wx.*X)^T U + (Wy.*Y) Z] ./ reg((Wx.*(U V^T))^T U + (Wy.*(V Z^T)) Z, V)
 *   U <- U .* [(Wx.*X) V] ./ reg((Wx.*(U V^T)) V, U)   (new V)         Z <- Z .* [(Wy.*Y)^T V] ./ reg((Wy.*(V Z^T))^T V, Z)
 *   reg(den, F) = den + l1 + l2 F, then den == 0 -> EPS = 2^-23         (cmf_solvers.py:212-228 with gamma = 1)
 * A relation without weights takes part with W == 1 (no matrix of ones is formed); with both absent this is cmf_mu_step's
 * update in another association.  The m x d product under the weights is never materialised (csrc/cmf_wmu.hip.h).
 * PRECONDITION: non-negative data, weights and factors.  which: 0 = X, 1 = Y.
 *   cmf_set_weight_f64 / _f32: dense weights of the relation's shape, element (i,j) at ptr[i*rs + j*cs].  The relation's data
 *   must be set and held dense (CMF_EINVAL otherwise); call again after the data change.  Forms the image W .* T once.
 *   cmf_set_weighted_csr: the observed pattern (scipy CSR layout, nnz = indptr[rows]) with the data and the weights on it; the
 *   loss of that relation then runs over the stored entries only (explicit zeros of either array included), cost O(nnz k) per
 *   pass, no dense image.  Held in buffers of its own: the data slot of that relation need not be set and is not read.
 *   cmf_clear_weight: back to unweighted.  cmf_set_problem drops all weights.
 *   cmf_mu_weighted_step: one iteration in the sweep order V, U, Z.  k_pad > 256: CMF_EUNSUPPORTED; a relation named by the mask
 *   that has neither data nor CSR weights: CMF_EINVAL; an unweighted relation held only as native CSR: CMF_EUNSUPPORTED (give it
 *   a dense image, sparse_mode 1).  No floating-point atomics: a repeated call from the same state is bit-identical.
 *   cmf_weighted_residual_sq: *ex = sum Wx .* (X - U V^T)^2, *ey likewise (either may be NULL), every term in float32 in the
 *   direct form, float64 accumulation.
 *   cmf_mu_weighted_layout: out4 = { shares of the streamed dimension in the U, V, Z sweeps (option "wmu_split" n forces them,
 *   as "kl_split" does for the KL passes; 1 for CSR weights); device scratch bytes of a full step }.
 *   cmf_fill_weight_synthetic: a Bernoulli(density) 0/1 mask from the counter-based generator of cmf_fill_data_synthetic as dense
 *   weights; cmf_get_weight_block_f32: a block of the dense weight image (full-size tests, the timing tool).
 * cmf_mu_step, cmf_mu_kl_step, cmf_run and cmf_residual_sq ignore weights; every option, captured graph and buffer of theirs is
 * left as it was.                                                                                                            */
int cmf_set_weight_f64(cmf_ctx *ctx, int which, const double *ptr, int64_t rs, int64_t cs);
int cmf_set_weight_f32(cmf_ctx *ctx, int which, const float *ptr, int64_t rs, int64_t cs);
int cmf_set_weighted_csr(cmf_ctx *ctx, int which, const int64_t *indptr, const int32_t *indices, const double *t_values, const double *w_values);
int cmf_clear_weight(cmf_ctx *ctx, int which);
int cmf_mu_weighted_step(cmf_ctx *ctx, double l1, double l2, int update_mask);
int cmf_weighted_residual_sq(cmf_ctx *ctx, double *ex, double *ey);
int cmf_mu_weighted_layout(cmf_ctx *ctx, int64_t *out4);
int cmf_fill_weight_synthetic(cmf_ctx *ctx, int which, uint64_t seed, double density);
int cmf_get_weight_block_f32(cmf_ctx *ctx, int which, int64_t row0, int64_t nrows, int64_t col0, int64_t ncols, float *host_dst);

/* ---- HALS solver: cyclic coordinate descent on MU's objective ---------------------------------------------------------------
 * The reference has multiplicative updates only for the non-negative Frobenius fit; sklearn's default for that objective is
 * coordinate descent.  Here:
 *   minimise  1/2 |X - U V^T|^2 + 1/2 |Y - V Z^T|^2 + l1 (sum U + sum V + sum Z) + l2 / 2 (|U|^2 + |V|^2 + |Z|^2),  U, V, Z >= 0
 * in MU's sweep order V, U, Z (cmf_solvers.py:248-263), the new V used for U and Z.  One sweep of a factor F with numerator N
 * and Gram G -- V: N = X^T U + Y Z, G = U^T U + Z^T Z;  U: N = X V, G = V^T V;  Z: N = Y^T V, G = V^T V -- runs, for every row f
 * of F on its own,
 *   for j = 0 .. k - 1:  h = G[j][j] + l2;  h == 0: f[j] stays;
 *                        f[j] <- max(0, f[j] - (sum_l f[l] G[l][j] + l2 f[j] - N[j] + l1) / h)    (l < j: already updated)
 * which is sklearn's _update_coordinate_descent without shuffling.  There is no EPS floor: exact zeros are results and can
 * become positive again.  PRECONDITION: non-negative factors (data may have any sign).
 * The products are the ones of cmf_mu_step (dense images and native CSR alike), run whole into its buffers; the sweep is
 * csrc/cmf_hals.hip.h: F G[:, b] per block b of 32 coordinates on the fp32 matrix pipe, the 32 sequential steps of the block in
 * registers.  Padding rows and columns of the factors stay zero.  No atomics: a repeated call from the same state is
 * bit-identical.  k_pad > 256 (n_components above 256), or per-entry weights bound to the context (HALS has no weighted
 * objective; it would silently ignore them): CMF_EUNSUPPORTED.  update_mask outside 1 .. 7, or a sweep whose data matrix has not
 * been set: CMF_EINVAL.  One GPU; cmf_run is not extended (a HALS fit keeps its loop on the host) and the step
 * is never captured into a graph.  cmf_mu_step's captured graph may be dropped and captured again; its results do not change.
 *   cmf_hals_sweep (tests): one sweep of factor `which` (CMF_U | CMF_V | CMF_Z) with the caller's numerator N[rows x k] and Gram
 *   G[k x k] (host, row-major float64, rounded to float32 on upload).  Needs cmf_set_problem and the factor, no data.
 * Kernel time goes to class CMF_K_HALS. */
int cmf_hals_step(cmf_ctx *ctx, double l1, double l2, int update_mask);
int cmf_hals_sweep(cmf_ctx *ctx, int which, const double *N, const double *G, double l1, double l2);

/* ---- ALS solver: per-row normal equations over the observed entries ---------------------------------------------------------
 * The standard method for a quadratic loss over an observed pattern; the reference has no counterpart (its solvers are mu and
 * newton, neither with weights).  Here:
 *   minimise  1/2 sum_{Ox} wx_ij (x_ij - u_i . v_j)^2 + 1/2 sum_{Oy} wy_jc (y_jc - v_j . z_c)^2 + l2 / 2 (|U|^2 + |V|^2 + |Z|^2)
 * in MU's sweep order V, U, Z (cmf_solvers.py:248-263), the new V used for U and Z; only the factors in update_mask are swept.
 * A relation is OBSERVED -- weights bound through cmf_set_weighted_csr: the loss runs over the stored pattern only -- or FULL --
 * no weights: every cell counts with weight 1, zeros of a sparse matrix included; dense image or native CSR.  Every row f_i of
 * the swept factor becomes the exact minimiser of its own system
 *   (sum_{c in O_i} w_ic b_c b_c^T + S + l2 I) f_i = sum_{c in O_i} w_ic t_ic b_c + N_i
 * with the sums over the observed relation(s) of the sweep and S = B^T B, N = T B of a full one (U: the X side, Z: the Y side,
 * V: both, mixed freely).  A row without observations and without a full side solves to exact zeros.  A sweep without an observed
 * side has ONE matrix for all rows: G + l2 I is inverted once in float64 and applied with one product.
 * nn_mask (CMF_NN_*): the solved rows of those factors are projected, max(0, .), as the Newton solver honours *_non_negative.
 * EXACT MINIMISATION PER ROW, AND WITH IT THE MONOTONE DESCENT OF THE OBJECTIVE, HOLDS FOR SIGNED FACTORS (nn_mask = 0) ONLY: the
 * projection of an unconstrained minimiser is not the constrained one.  cmf_hals_step and cmf_mu_step / cmf_mu_weighted_step
 * are the solvers built for non-negative factors, and cmf_als_nnls_step (below) is this step with the constrained row solve.
 * There is no l1 term.
 * The normal equations are formed by csrc/cmf_als.hip.h: gathered rows staged through LDS 32 at a time, H_i on the fp32 matrix
 * pipe from ONE sqrt(w)-scaled image, rows longer than a piece length (option "als_piece" n, default 4096, rounded up to 32) cut
 * into pieces whose partial sums are added in piece order.  No floating-point atomics: a repeated call from the same state is
 * bit-identical.  The k x k solves are the plain Cholesky route of the per-row Newton sweeps (lambda_min(H_i) >= l2: the
 * spectral clamp never acts; cmf_newton_clamp_stats stays at zero rows).  Padding rows and columns of the factors stay zero.
 *   CMF_EINVAL: l2 <= 0, update_mask outside 1 .. 7, a swept relation with neither data nor CSR weights.
 *   CMF_EUNSUPPORTED: k_pad > 256 (n_components above 256); a swept relation with DENSE weights bound (cmf_set_weight_f64 / _f32).
 * One GPU; cmf_run is not extended (an ALS fit keeps its loop on the host) and the step is never captured into a graph.
 * cmf_mu_step, cmf_mu_weighted_step, cmf_hals_step, cmf_newton_step keep their options, buffers and results; a captured graph of
 * theirs may be dropped and captured again.  The error metric of such a fit is cmf_weighted_residual_sq (observed sides) /
 * cmf_residual_sq (full sides).  Kernel time: the normal equations go to class CMF_K_ROWHESS (2 nnz k^2 flops), the solves to
 * the classes the Newton sweeps charge.
 *   cmf_als_normal (tests): the finished H_i (k_pad x k_pad, both triangles, 1 on the padding diagonal) and g_i (k_pad) of rows
 *   [row0, row0 + nrows) of factor `which`, as the step would hand them to the solver, into host memory.  The sweep must have an
 *   observed relation (CMF_EINVAL otherwise).
 *   cmf_als_layout: out4 = { piece length, pieces of the U sweep, of the V sweep, of the Z sweep } (0 for a sweep without an
 *   observed relation).
 * NON-NEGATIVE ROWS BY COORDINATE DESCENT, cmf_als_nnls_step: the step above, except that a swept factor in nn_mask is not solved
 * and projected: each of its rows runs `sweeps` (1 .. 1024) passes of cyclic coordinate descent on its own constrained problem
 *   min_{f >= 0} 1/2 f^T H_i f - g_i^T f,     per pass:  r = g_i - H_i f;  for j = 0 .. k - 1:  new = max(0, f_j + r_j / H_jj),
 *                                                        r -= (new - f_j) H_i[j, :],  f_j = new
 * from the row it has (csrc/cmf_als_nnls.hip.h: one wave per row, H_i streamed once per pass, no Cholesky, the state of the
 * Newton solves untouched).  Every coordinate step is an exact one-dimensional minimisation, so the objective descends
 * monotonically WITH non-negative factors; one pass is a weighted HALS sweep, each row under its own Gram, many passes approach
 * alternating non-negative least squares (4 is the documented choice).  There is no tolerance-based stop; a row that a whole pass
 * leaves unchanged stops, which changes no bit.  A row without information becomes exact zeros.  A swept factor outside nn_mask
 * takes the route of cmf_als_step, signed; with nn_mask = 0 the step IS cmf_als_step, byte for byte.  A factor in nn_mask whose
 * relations are all full runs the sweep of cmf_hals_step (l1 = 0) `sweeps` times on its one Gram.  Validation as cmf_als_step,
 * and CMF_EINVAL for sweeps outside 1 .. 1024.  Kernel time of the passes: class CMF_K_HALS, 2 rows k^2 sweeps flops.
 *   cmf_als_nnls_rows (tests): the kernel on the caller's nrows systems in cmf_als_normal's layout (k / k_pad of the bound
 *   problem; positive diagonals), host_f[nrows x k_pad] the start and the result.  CMF_EINVAL: a null pointer, nrows < 0, sweeps
 *   outside 1 .. 1024, no problem bound; CMF_EUNSUPPORTED: k_pad > 256.
 * SIGNED ROWS BY CONJUGATE GRADIENTS, cmf_als_cg_step: the step above, except that a swept factor that is SIGNED (outside nn_mask)
 * and has an OBSERVED relation never forms H_i: each of its rows runs cg_steps (1 .. 1024) steps of plain conjugate gradients on
 * H_i f = g_i from the row it has,
 *   r = g - H f, p = r;  per step: q = H p, alpha = (r.r)/(p.q), f += alpha p, r -= alpha q, beta = (r'.r')/(r.r), p = r' + beta p,
 * one product H_i x = sum_e w_e b_e (b_e . x) + S x + l2 x being one pass over the row's gathered factor rows (csrc/
 * cmf_als_cg.hip.h: one workgroup per row, all steps in one launch, O(nnz k) per step instead of O(nnz k^2) + k^3 / 3; no
 * normal equations, no Cholesky, the state of the Newton solves untouched).  Every step from a warm start lowers the row's
 * quadratic, so the objective still descends monotonically; the rows are no longer exact minimisers (6 steps is the documented
 * choice).  A row stops early when r.r or p.q is not a positive finite number and keeps what it has; a row without information
 * becomes exact zeros.  Rows short enough keep their gathered rows in LDS between the passes (option "als_cg_lds" n: the most
 * bytes of LDS a row may use for that; 0: every row gathers again each pass; < 0: the default, a quarter of the LDS) -- the result does
 * not depend on it, nor on anything but the row itself: a repeated call from the same state is bit-identical.
 * Everything else keeps its route and its bits: a factor in nn_mask is projected (nn_sweeps = 0) or swept by coordinate descent
 * (nn_sweeps 1 .. 1024, as cmf_als_nnls_step); a sweep whose relations are all full takes the shared float64 inverse.
 * Validation as cmf_als_step, and CMF_EINVAL for cg_steps outside 1 .. 1024 or nn_sweeps outside 0 .. 1024.  Kernel time: class
 * CMF_K_ROWHESS, 4 nnz k (cg_steps + 1) flops, plus 2 rows k^2 (cg_steps + 1) with a full side.
 * LONG ROWS (the hot columns of click, play and bag-of-words data in the V sweep): a row with more than L stored entries (option
 * "als_cg_piece", default 2048) is not walked by one workgroup.  Its entries, side 0 then side 1 in stored order, are cut into
 * pieces of L; per product H x one launch sums every piece in a workgroup of its own and a second one adds a row's pieces in piece
 * order and takes the CG step, all long rows of the sweep together: 2 (cg_steps + 1) launches, no atomics, the same formulas and
 * stop rule.  The result of such a row depends on the row and on L alone; shorter rows keep the single launch and its bits.
 *   cmf_als_cg_rows (tests): host_f[nrows x k_pad] = the rows the CG route would write for rows [row0, row0 + nrows) of the sweep
 *   of factor `which`, from the current factors, which are left unchanged.  CMF_EINVAL for a sweep without an observed relation.
 *   cmf_als_cg_last (tests, read-only): out2[0] = the long rows, out2[1] = their pieces in the last sweep of the CG route
 *   (cmf_als_cg_step or cmf_als_cg_rows) of this context; zeros before the first one.  CMF_EINVAL for a null pointer.          */
int cmf_als_step(cmf_ctx *ctx, double l2, int nn_mask, int update_mask);
int cmf_als_normal(cmf_ctx *ctx, int which, int64_t row0, int64_t nrows, double l2, float *host_H, float *host_g);
int cmf_als_layout(cmf_ctx *ctx, int64_t *out4);
int cmf_als_nnls_step(cmf_ctx *ctx, double l2, int nn_mask, int update_mask, int sweeps);
int cmf_als_nnls_rows(cmf_ctx *ctx, int64_t nrows, const float *host_H, const float *host_g, float *host_f, int sweeps);
int cmf_als_cg_step(cmf_ctx *ctx, double l2, int nn_mask, int update_mask, int cg_steps, int nn_sweeps);
int cmf_als_cg_rows(cmf_ctx *ctx, int which, int64_t row0, int64_t nrows, double l2, int cg_steps, float *host_f);
int cmf_als_cg_last(cmf_ctx *ctx, int64_t *out2);

/* ---- ALS: matrix-free NON-NEGATIVE rows by projected conjugate gradients -------------------------------------------------------
 * cmf_als_nncg_step: cmf_als_cg_step's step, except that a swept factor in nn_mask that has an OBSERVED relation never forms H_i
 * either.  Each of its rows runs nn_cg_steps (1 .. 1024) steps on  min_{f >= 0} 1/2 f^T H_i f - g_i^T f  from the row it has, with
 * the product H_i x of cmf_als_cg_step (one pass over the row's gathered factor rows; the excess weights and S under a background
 * weight, exactly as the CG route reads them):
 *   f <- max(f, 0);  r = g - H f;  p = none
 *   per step:  free_j = f_j > 0 or r_j > 0;  z = r on free, 0 elsewhere;  rho = z.z;  stop unless rho is positive and finite
 *              p = z + (rho / rho_old) p  if the step before was a free step and left the same free set,  else p = z
 *              q = H p;  pq = p.q;  stop unless positive and finite;  alpha = (p.r) / pq;  t = f + alpha p
 *              no t_j < 0:  FREE step       f = t,  r -= alpha q,  rho_old = rho,  free_old = free
 *              otherwise    PROJECTED step  f+ = max(t, 0),  d = f+ - f,  hd = H d (a second pass),  dr = d.r,  dhd = d.hd;  stop
 *                           unless both are positive and finite;  theta = dr / dhd;  theta >= 1: f = f+, r -= hd;  else
 *                           f = max(f + theta d, 0), r -= theta hd;  p = none
 * Every step is an exact line search along a descent direction that ends at or before the line's minimiser and leaves f >= 0, so
 * the objective descends monotonically WITH non-negative factors; one or two passes of O(nnz k) per step, a row is read at most
 * 2 nn_cg_steps + 1 times, no k x k scratch (csrc/cmf_als_nncg.hip.h: one workgroup per row, all steps in one launch, no atomics;
 * options "als_cg_lds" and "als_cg_piece" act as on the CG route, long rows take the piece form with 2 + 4 nn_cg_steps launches).
 * A stopped row keeps what it has, a row without information becomes exact zeros; the result of a row depends on that row (and the
 * piece length) alone and is deterministic to the bit.
 * The other factors keep their routes: a signed factor with an observed relation runs cg_steps CG steps (0: the exact rows), a
 * factor in nn_mask whose relations are all full the route nn_sweeps names.  With no factor on the new route the call IS
 * cmf_als_cg_step (cg_steps > 0), cmf_als_nnls_step (nn_sweeps > 0) or cmf_als_step, validation and bits.
 * Validation as cmf_als_step; CMF_EINVAL for cg_steps or nn_sweeps outside 0 .. 1024 or nn_cg_steps outside 1 .. 1024;
 * CMF_EUNSUPPORTED when a sweep on the new route reads a logistic relation or a relation with biases bound (cmf_als_bias_step
 * keeps its signature and its routes), and for k_pad > 256.  Kernel time: class CMF_K_ROWHESS, 4 len k flops per pass a row of len
 * stored entries actually ran (+ 2 k^2 per pass with a full side or a background); the passes stay on the device and
 * come back only with kernel timing on (behind the timed stretch) or for cmf_als_nncg_passes: a sweep waits for neither.
 *   cmf_als_nncg_rows (tests): host_f[nrows x k_pad] = the rows that route would write for rows [row0, row0 + nrows) of the sweep
 *   of factor `which` (in nn_mask or not), from the current factors, which are left unchanged.  CMF_EINVAL for a sweep without an
 *   observed relation.
 *   cmf_als_nncg_last (tests, read-only): out2[0] = the long rows, out2[1] = their pieces in the last sweep of that route;
 *   cmf_als_nncg_passes (measurement, read-only): out2[0] = the passes its rows ran, summed over the rows, out2[1] = the stored
 *   entries those passes read (sum of len x passes).  Zeros before the first sweep; CMF_EINVAL for a null pointer.              */
int cmf_als_nncg_step(cmf_ctx *ctx, double l2, int nn_mask, int update_mask, int cg_steps, int nn_cg_steps, int nn_sweeps);
int cmf_als_nncg_rows(cmf_ctx *ctx, int which, int64_t row0, int64_t nrows, double l2, int nn_cg_steps, float *host_f);
int cmf_als_nncg_last(cmf_ctx *ctx, int64_t *out2);
int cmf_als_nncg_passes(cmf_ctx *ctx, int64_t *out2);

/* ---- ALS: exact rows of few stored entries in DUAL form ---------------------------------------------------------------------
 * cmf_als_dual_step: cmf_als_step's step with a permission dual_max (0 = off, 1 .. 128).  A sweep is ELIGIBLE when it would take
 * the exact row route (observed; signed, or in nn_mask with nn_sweeps = 0 and nn_cg_steps = 0: the solved row is then projected),
 * has no shared term (every relation it reads is observed and has no background weight) and reads no logistic relation.  With
 *   a_e = sqrt(w_e) b_e  (A: n x k),   y_e = p_e / sqrt(w_e)  (0 where w_e = 0)
 * over the row's n stored entries (side 0 then side 1, stored order; p = w t with the bias terms taken off) the exact row solves
 * (A^T A + l2 I_k) f = A^T y, and the same f is  K = A A^T + l2 I_n,  K z = y,  f = A^T z.  Inside an eligible sweep a row goes
 * dual when 1 <= n <= dual_max and its class width NP(n) (the smallest of 32, 64, 128 that is >= n) is below k_pad; a row
 * without a stored entry becomes zeros; every other row takes the formed route on compact slots and ends with the bits
 * cmf_als_step gives it.  A sweep that is not eligible, and every sweep under dual_max = 0, runs what it runs without this entry
 * point: same launches, same bits.  Non-negative factors take nn_sweeps / nn_cg_steps as cmf_als_nncg_step gives them; there is
 * no cg_steps (CG would take every sweep the dual route could); with biases bound the bias blocks follow as in cmf_als_bias_step.
 * csrc/cmf_als_dual.hip.h: the symmetric Gram on the matrix pipe, the solve through the Cholesky path of the exact route on
 * NP x NP matrices (threshold l2 / 16), one accumulator chain per coordinate in stored order for f; no atomics, deterministic to
 * the bit, a row's result depends on that row alone.  Kernel time: the Gram under CMF_K_ROWHESS at 2 NP^2 k flops per row.
 * Validation as cmf_als_step; CMF_EINVAL for dual_max outside 0 .. 128 or a count outside 0 .. 1024; CMF_EUNSUPPORTED for
 * k_pad > 256 and for nn_cg_steps > 0 with biases bound.
 *   cmf_als_dual_rows (tests): host_f[nrows x k_pad] = the rows an eligible sweep of factor `which` would write for rows
 *   [row0, row0 + nrows) under dual_max (unprojected), from the current factors, which are left unchanged.  CMF_EINVAL, naming
 *   why, for a sweep that is not eligible: no observed relation, a shared term, or a logistic relation.
 *   cmf_als_dual_last (tests, read-only): out5 = rows in class 32, 64 and 128, rows left to the formed route and rows written as
 *   zeros in the last dual sweep (or cmf_als_dual_rows call).  Zeros before the first; CMF_EINVAL for a null pointer.            */
int cmf_als_dual_step(cmf_ctx *ctx, double l2, int nn_mask, int update_mask, int dual_max, int nn_sweeps, int nn_cg_steps);
int cmf_als_dual_rows(cmf_ctx *ctx, int which, int64_t row0, int64_t nrows, double l2, int dual_max, float *host_f);
int cmf_als_dual_last(cmf_ctx *ctx, int64_t *out5);

/* ---- ALS: a per-row l2 (frequency-scaled regularisation) ---------------------------------------------------------------------
 * One scalar l2 over-shrinks the rows with many stored entries or under-regularises those with few.  With a vector of positive
 * multipliers m_F per factor F in {U, V, Z} the regulariser of the ALS objective becomes
 *   l2 / 2 sum_F sum_i m_F[i] |f_i|^2,
 * and row i of a sweep of F solves the system it solves above under lambda_i = l2 m_F[i] in place of l2.  m = n_i is the
 * weighted-lambda form of Zhou, Wilkinson, Schreiber and Pan (ALS-WR); m = (n_i + alpha0 D)^nu the frequency-scaled form of
 * Rendle, Krichene, Zhang and Koren (pycmf_amd.l2_multipliers computes both on the host).
 *   cmf_set_l2_rows(ctx, which, mult): binds frows[which] multipliers for factor `which` (0 U | 1 V | 2 Z); mult = NULL clears them.
 *   CMF_EINVAL for a bad `which` and for a value that is not finite and positive, as a double or rounded to float32; the state is
 *   then unchanged.  cmf_set_problem clears all three factors' multipliers.
 *   cmf_get_l2_rows(ctx, which, mult, set): *set = 1 | 0 (bound or not), mult[frows[which]] = the doubles as given (ones when none
 *   are bound); either pointer may be NULL.
 * The device holds the multipliers as float32, rounded once, and every row kernel forms lambda_i = (float)l2 * mult[row] as ONE
 * float32 multiplication that is never fused with the addition behind it: a row under the multiplier v has, to the bit, the row the
 * same call gives it under the scalar l2' with (float)l2' = fl((float)l2 v) and nothing bound.  With nothing bound the kernels take
 * l2 itself: the launches and the bits of a context that never heard of this block.
 * HONOURED BY all six cmf_als_*_step entry points on every row route (the finished systems of the exact, coordinate-descent and
 * logistic rows; the l2 x term of the conjugate-gradient and projected conjugate-gradient rows, whole or cut into pieces; the whole
 * diagonal of the dual systems), by cmf_als_cg_rows / cmf_als_nncg_rows / cmf_als_dual_rows and by cmf_als_normal.  The exact
 * solve takes its threshold from the smallest lambda of the sweep: l2 min(m_F) / 16.  A factor WITHOUT an observed relation has one
 * matrix for all rows: with multipliers that are all equal as float32 its sweep runs under l2 m_F[0]; otherwise the step returns
 * CMF_EUNSUPPORTED and names the factor (nothing of that sweep has run; the context stays usable).
 * The bias blocks of cmf_als_bias_step keep their own regulariser bias_l2 UNSCALED; the factor sweeps inside that call honour the
 * multipliers.  NOT READ by the MU, HALS and Newton steps or by the error entry points: bind multipliers only for the ALS steps.    */
int cmf_set_l2_rows(cmf_ctx *ctx, int which, const double *mult);
int cmf_get_l2_rows(cmf_ctx *ctx, int which, double *mult, int *set);

/* ---- ALS for implicit feedback: a background weight on the cells outside the pattern ----------------------------------------
 * Clicks, plays, purchases: every stored target is 1, so a fit over the pattern alone is degenerate, and a fit with every cell at
 * weight 1 lets a click count no more than a non-click.  The standard model (Hu, Koren, Volinsky: "Collaborative Filtering for
 * Implicit Feedback Datasets") lies between the two.  For a relation with CSR weights w on its pattern O and a background weight
 * c0 >= 0 the term of the objective is
 *   1/2 sum_{O} w_ic (t_ic - a_i . b_c)^2  +  1/2 c0 sum_{(i,c) not in O} (a_i . b_c)^2,       w_ic >= c0 ON EVERY STORED ENTRY
 * -- the dense weighted objective with W = c0 and target 0 off the pattern.  With the excess weights e = w - c0 a row's system is
 *   H_i = sum_{c in O_i} e_ic b_c b_c^T + c0 B^T B + (Gram of a full side) + l2 I,    g_i = sum_{c in O_i} w_ic t_ic b_c + N_i,
 * so no cell outside the pattern is ever visited: cost O(nnz k^2) + one Gram per sweep, as without a background.  A row without
 * stored entries is an ordinary row (as under a full side): the exact route solves it to its minimiser, exact zeros when g_i = 0.
 *   cmf_set_background_weight(ctx, which, c0): `which` (0 = X, 1 = Y) must have CSR weights bound (cmf_set_weighted_csr), c0 must
 *   be finite and >= 0 (it is rounded to float32), and every stored weight must be >= c0 in float32 (a minimum taken on the
 *   device) -- CMF_EINVAL otherwise, the state unchanged.  Builds the excess weights of both orientations of the pattern next to
 *   the weights.  c0 = 0 frees them: the state of a context that never had a background.  cmf_set_weighted_csr, cmf_clear_weight,
 *   cmf_set_weight_f32 / _f64 and cmf_set_problem reset the background of the relation to 0.
 *   cmf_get_background_weight: the value in effect (0: none).
 * HONOURED BY cmf_als_step, cmf_als_nnls_step and cmf_als_cg_step on every route a sweep with an observed side takes, and by
 * cmf_als_normal / cmf_als_cg_rows (the systems and rows they return include it).  The kernels and their arithmetic are the
 * ones above: they read e where they read w, and the shared matrix S becomes sum_sides coef Gram(B_side), coef = c0 for a side
 * with a background, 1 for a full side (a V sweep can have two), each product and the sum rounded once, in the order X side, Y
 * side.  With c0 = 0 every step is the step above, byte for byte.  The CG route reads S (k_pad^2 floats) once per row and pass,
 * as a V sweep beside a full Y does; on patterns with a few very long columns (hot items) keep the exact route for V, as
 * without a background (a CG row is one workgroup however long it is).
 *   cmf_als_residual_sq: for a relation with CSR weights, with or without a background (CMF_EINVAL for a requested side without
 *   CSR weights; either pointer may be NULL),
 *     E = sum_O w (t - s)^2 + c0 (<A^T A, B^T B>_F - sum_O s^2),    s = a_i . b_c in float32,
 *   both sums over the pattern from ONE pass in float64, the trace term from float64 Grams, clamped at 0; no atomics, a repeated
 *   call is bit-identical.  With c0 = 0 it returns the bits of cmf_weighted_residual_sq, which is unchanged (pattern term only).
 * NOT HONOURED by cmf_mu_weighted_step: with a background bound on a relation it reads it returns CMF_EUNSUPPORTED (clear it
 * with cmf_set_background_weight(ctx, which, 0)).  cmf_mu_step, cmf_hals_step, cmf_newton_step and cmf_residual_sq ignore
 * weights and background alike.  Kernel time: the excess weights and S go to CMF_K_ELEMWISE, the error's pass to CMF_K_KLMU, its
 * Grams to CMF_K_GEMM_SMALL.                                                                                                 */
int cmf_set_background_weight(cmf_ctx *ctx, int which, double c0);
int cmf_get_background_weight(cmf_ctx *ctx, int which, double *c0);
int cmf_als_residual_sq(cmf_ctx *ctx, double *ex, double *ey);

/* ---- ALS for explicit ratings: a global mean, row and column biases, and the value of given cells ------------------------------
 * Ratings: "this user rates high" and "this item is liked" are offsets, not factors.  For a relation with CSR weights w on its
 * pattern O and biases enabled the term of the objective is (written for X; Y is the same with V, Z)
 *   1/2 sum_{O} w_ij (x_ij - mu - r_i - c_j - u_i . v_j)^2  +  lb/2 (|r|^2 + |c|^2),        mu FIXED, lb >= 0
 * and one iteration is block coordinate descent: the factor sweeps V, U, Z of the steps above, every sweep of a biased relation
 * reading the adjusted targets t - mu - r_i - c_j in place of t; then, per biased relation, r and then c from the new r, each the
 * exact minimiser  r_i = sum_{j in O_i} w (t - mu - c_j - u_i . v_j) / (sum_{j in O_i} w + lb).  A row without stored entries gets
 * exactly 0, and so does a row whose denominator is 0.  Every block is an exact minimisation or a CG / coordinate step that lowers
 * its quadratic: the descent stays monotone wherever it is monotone without biases.  The bias blocks follow the update mask of
 * the factor on their axis: r_x with U, c_x and r_y with V, c_y with Z -- so a fold-in of new rows fits their own biases too.
 *   cmf_set_biases(ctx, which, enable, mu, lb): `which` (0 = X, 1 = Y) must have CSR weights bound (CMF_EINVAL otherwise, and for a
 *   non-finite mu or lb < 0) and NO background weight (CMF_EUNSUPPORTED; cmf_set_background_weight with c0 > 0 on a biased relation
 *   is refused the same way; the state is unchanged in both cases).  Allocates zeroed r and c, the adjusted targets of both
 *   orientations of the pattern and the piece lists.  enable = 0 frees all of it: the state of a context that never had biases.
 *   cmf_set_weighted_csr, cmf_clear_weight, cmf_set_weight_f32 / _f64 and cmf_set_problem drop the biases of the relation.
 *   cmf_get_biases: mu, lb and whether biases are bound (any pointer may be NULL).
 *   cmf_set_bias_f64 / cmf_get_bias_f64(ctx, which, axis, v): the row (axis 0) or column (axis 1) biases, rounded to float32.
 *   cmf_als_bias_step(ctx, l2, nn_mask, update_mask, cg_steps, nn_sweeps): runs the sweeps of cmf_als_cg_step with the same
 *   arguments on the adjusted targets (cg_steps = 0: the exact rows; cg_steps = 0 and nn_sweeps = 0: cmf_als_step's routes), then
 *   the bias sweeps update_mask allows, then rewrites the adjusted targets (they are rewritten whenever the biases change: by
 *   this step, cmf_set_biases and cmf_set_bias_f64, so every entry point finds them current).  Validation as cmf_als_cg_step, except that cg_steps may be 0.  With no relation
 *   biased it is that step, byte for byte.
 *   cmf_als_bias_rows (tests): host_out = the biases one bias sweep of `which` along `axis` would write from the current state;
 *   nothing is changed.  cmf_als_bias_targets (tests): the adjusted targets bt and bp = w bt of the pattern (image 0) or its
 *   transpose (image 1) in stored order into buffers of nnz floats (either pointer may be NULL; CMF_EINVAL unless nnz is the number
 *   of stored entries of the pattern).
 *   cmf_predict_pairs(ctx, which, link, n, rows, cols, out): out[q] = f(mu + r[rows[q]] + c[cols[q]] + a . b) in float32 for n
 *   arbitrary cells, a . b = U V^T (which = 0) or V Z^T (1), the bias terms only when biases are bound on `which`, f the identity
 *   (CMF_LINK_LINEAR) or the sigmoid (CMF_LINK_LOGIT).  Needs the factors only and changes nothing.  CMF_EINVAL: an index outside
 *   the relation (checked on the host); CMF_EUNSUPPORTED: k_pad > 256.
 * The kernels (csrc/cmf_als_bias.hip.h): a bias sweep cuts every row into pieces of at most L stored entries (option
 * "als_bias_piece": 0 the default, 2048; > 0 rounded up to 16; < 0 every row is one piece), one workgroup per piece, the lane groups
 * of k_pad / 4 lanes dealing its entries round-robin; each term in float32, sums in float64, groups added in group order, pieces in
 * piece order by a second launch.  No lane group ever walks a whole long row (hot items).  A row's bias depends on the row and on
 * L alone; no atomics: a repeated call from the same state is bit-identical.  The adjusted targets are rewritten with each
 * operation rounded once in float32.  The row kernels of the sweeps are unchanged: they read w (t - mu - r - c) where they read w t.
 * HONOURED BY cmf_als_bias_step and cmf_predict_pairs, and by cmf_als_residual_sq, which reads the adjusted targets where it reads
 * t (with no biases bound it returns the bits it returned before).  cmf_als_step, cmf_als_nnls_step and cmf_als_cg_step sweep the
 * factors on the adjusted targets too but never move the biases.  cmf_weighted_residual_sq is unchanged (no bias terms).
 * NOT HONOURED by cmf_mu_weighted_step: with biases bound on a relation it reads it returns CMF_EUNSUPPORTED (clear them with
 * cmf_set_biases(ctx, which, 0, 0, 0)).  One GPU; cmf_run is not extended.  Kernel time: the bias passes and cmf_predict_pairs
 * go to CMF_K_KLMU, the rewrite of the targets to CMF_K_ELEMWISE.                                                            */
int cmf_set_biases(cmf_ctx *ctx, int which, int enable, double mu, double lb);
int cmf_get_biases(cmf_ctx *ctx, int which, double *mu, double *lb, int *enabled);
int cmf_set_bias_f64(cmf_ctx *ctx, int which, int axis, const double *v);
int cmf_get_bias_f64(cmf_ctx *ctx, int which, int axis, double *v);
int cmf_als_bias_step(cmf_ctx *ctx, double l2, int nn_mask, int update_mask, int cg_steps, int nn_sweeps);
int cmf_als_bias_rows(cmf_ctx *ctx, int which, int axis, float *host_out);
int cmf_als_bias_targets(cmf_ctx *ctx, int which, int image, int64_t nnz, float *host_bt, float *host_bp);
int cmf_predict_pairs(cmf_ctx *ctx, int which, int link, int64_t n, const int64_t *rows, const int64_t *cols, float *out);

/* ---- ALS with a logistic loss: reweighted row systems over an observed pattern ------------------------------------------------
 * A relation with CSR weights may be fitted as sigmoid(a . b): labels, clicks, thumbs up / down on the cells that were observed.
 * Its term of the ALS objective becomes the weighted cross-entropy over the stored pattern,
 *   sum_O w [softplus(a . b) - t (a . b)],     t in [0, 1] (soft labels allowed), w >= 0,
 * while the other relation keeps whatever it is (Frobenius observed, Frobenius full, or logistic too); the l2 term is unchanged.
 * The Jaakkola-Jordan bound  w [softplus(s) - t s] <= 1/2 w kappa(xi) s^2 - w (t - 1/2) s + const,  kappa(xi) = tanh(xi / 2) / (2 xi)
 * in (0, 1/4], is tight at s = +-xi.  With xi the score under the CURRENT row, the minimiser of the bound for row i solves
 *   (sum_{e in O_i} w_e kappa_e b_e b_e^T + S + l2 I) f_i = sum_{e in O_i} w_e (t_e - 1/2) b_e + N_i
 * -- cmf_als_step's system with w kappa for w and w (t - 1/2) for w t; S, N from a full Frobenius side as there.  EVERY ROW SOLVE
 * LOWERS THE TRUE OBJECTIVE: the Cholesky rows of cmf_als_step with signed factors, and the coordinate-descent rows of
 * cmf_als_nnls_step with non-negative ones (they start from the current row and never raise the bound).  No step size, no clamp.
 * (With nn_mask and sweeps = 0 the solved row is only projected, as for the Frobenius loss: no descent guarantee.)
 *   cmf_set_relation_loss(ctx, which, kind): `which` 0 = X | 1 = Y, kind CMF_LOSS_FROBENIUS (0, the default) | CMF_LOSS_LOGISTIC
 *   (1).  CMF_EINVAL for another `which` or `kind`.  Cleared by cmf_set_problem.  cmf_get_relation_loss reads it back (CMF_EINVAL
 *   for a null output).  The targets are not inspected: the caller keeps them in [0, 1].
 * HONOURED BY cmf_als_step, cmf_als_nnls_step and cmf_als_normal, which returns the majoriser's system at the current row (tests).
 * With no logistic relation they launch exactly what they launch without this block.  A step (or cmf_als_normal) that sweeps a
 * logistic relation returns CMF_EUNSUPPORTED when the relation has no CSR weights bound (full, or dense weights: the logistic loss
 * over every cell is not built), a background weight, or biases; cmf_als_cg_step / cmf_als_cg_rows (the conjugate-gradient rows
 * would need a per-entry reweighting pass of their own) and cmf_als_bias_step return CMF_EUNSUPPORTED whenever they sweep one.
 * NOT HONOURED by the MU, HALS and Newton steps, cmf_weighted_residual_sq and cmf_als_residual_sq: they read the relation as the
 * Frobenius one it also is.  One GPU; cmf_run is not extended.
 *   cmf_als_logistic_loss(ctx, lx, ly): *lx / *ly = sum_O w [max(s, 0) + log1p(exp(-|s|)) - t s] of X / Y with the factors on the
 *   device, 0 for a Frobenius relation; a null pointer skips that side.  CMF_EUNSUPPORTED as above for a logistic relation that is
 *   not observed; k_pad > 256.
 * The kernels: the LG = true instance of als_normal_kernel (csrc/cmf_als.hip.h) is the normal-equation kernel with the current row in registers
 * beside every gathered row -- per gathered row one k-long dot product, a fixed-order lane reduction and one tanh; a Frobenius
 * side's pieces of a mixed V sweep run in the same launch.  The loss cuts every row into pieces of at most 2048 stored entries,
 * float64 partial sums added in piece order behind a kernel boundary.  No atomics: a repeated call from the same state is
 * bit-identical.  Kernel time: the normal equations go to CMF_K_ROWHESS (2 nnz k^2 + 2 nnz k flops), the loss to CMF_K_KLMU.   */
enum { CMF_LOSS_FROBENIUS = 0, CMF_LOSS_LOGISTIC = 1 };
int cmf_set_relation_loss(cmf_ctx *ctx, int which, int kind);
int cmf_get_relation_loss(cmf_ctx *ctx, int which, int *kind);
int cmf_als_logistic_loss(cmf_ctx *ctx, double *lx, double *ly);

/* ---- ALS with a Huber loss on an observed relation (csrc/cmf_als_reweight.hip.h) ----
 * A relation with CSR weights may be fitted under  sum_O w rho_d(t - a . b),  rho_d(r) = r^2 / 2 for |r| <= d and d (|r| - d / 2)
 * beyond: a stored entry far off the model pulls its row and its column with a bounded force.  The half-quadratic majoriser
 * rho_d(r) <= rho_d(r0) + omega(r0) (r^2 - r0^2) / 2, omega(r) = min(1, d / |r|), tight at the residual r0 under the CURRENT row,
 * turns a row's problem into the ALS row problem under the weights w omega on the same targets.  ONE pass (als_huber_pass_kernel)
 * in front of every sweep writes w omega and w t omega per stored entry of the image the sweep reads, and the sweep's route --
 * exact, coordinate descent, conjugate gradients signed or projected, dual, and the bias blocks -- reads them where it reads w and
 * w t, for that sweep only; no row kernel changes.  Every route starts at the current row and never raises its quadratic, so every
 * sweep lowers the objective (a non-negative factor that is only projected carries no guarantee, as without this block).  An entry
 * with |r| <= d keeps the bits of w and w t: while no residual exceeds d every entry point gives the bits it gives without a delta.
 *   cmf_set_huber_delta(ctx, which, delta): `which` 0 = X | 1 = Y; delta > 0 (finite, in float32 too) puts the relation under the
 *   Huber loss, 0 takes it back.  CMF_EINVAL otherwise.  Cleared by cmf_set_problem; kept when the weights are bound again.
 *   cmf_get_huber_delta reads it back (the float32 value; CMF_EINVAL for a null output).
 * HONOURED BY every ALS step (cmf_als_step, _nnls_, _cg_, _nncg_, _bias_, _dual_step), the row entries cmf_als_cg_rows,
 * cmf_als_nncg_rows, cmf_als_dual_rows, cmf_als_bias_rows and cmf_als_normal (the majoriser's system at the current row).  With no
 * delta set they launch exactly what they launch without this block.  Each returns CMF_EUNSUPPORTED when a Huber relation it sweeps
 * has no CSR weights bound (the Huber loss over every cell is not built), a background weight, or a logistic loss; the other
 * relation may be anything it can be without this block.  NOT HONOURED by the MU, HALS and Newton steps, cmf_weighted_residual_sq,
 * cmf_als_residual_sq and cmf_als_logistic_loss, which read the relation's weights as bound.  One GPU; cmf_run is not extended.
 *   cmf_als_huber_loss(ctx, lx, ly): *lx / *ly = sum_O w rho_d(t - a . b) of X / Y with the factors on the device (under biases: the
 *   adjusted targets), 0 for a relation without a delta; a null pointer skips that side.  CMF_EUNSUPPORTED as above; k_pad > 256.
 *   cmf_als_huber_weights(ctx, which, t, nnz, w_eff, p_eff) (test entry): w omega and w t omega of image t (0 the pattern, 1 its
 *   transpose, each in its stored order) at the current factors, nnz floats each; a null pointer skips that array.  CMF_EINVAL for
 *   a relation without a delta, or when nnz is not the number of stored entries (the size of the caller's buffers, as in
 *   cmf_als_bias_targets).
 * The kernel cuts every row into pieces of at most 2048 stored entries, one 256-thread workgroup each: the row in registers, four
 * gathered rows in flight per lane group, the score in float32 in the fixed order of the lane reduction, omega by a true division.
 * The loss adds float64 partial sums in piece order behind a kernel boundary.  No atomics: a repeated call from the same state is
 * bit-identical.  Kernel time: both forms of the pass go to CMF_K_KLMU (2 nnz k_pad flops).                                    */
int cmf_set_huber_delta(cmf_ctx *ctx, int which, double delta);
int cmf_get_huber_delta(cmf_ctx *ctx, int which, double *delta);
int cmf_als_huber_loss(cmf_ctx *ctx, double *lx, double *ly);
int cmf_als_huber_weights(cmf_ctx *ctx, int which, int t, int64_t nnz, float *w_eff, float *p_eff);

/* ---- ALS with a logistic loss on every route: the reweighting as a pass of its own (csrc/cmf_als_reweight.hip.h) ----
 * By default a logistic relation (cmf_set_relation_loss) is reweighted inside the normal-equation kernel, so only the routes that
 * form the k x k systems honour it.  Under this flag the relation is reweighted like a Huber one instead: ONE pass
 * (als_logit_pass_kernel) in front of every sweep writes  w kappa(xi)  per stored entry of the image the sweep reads, xi the score
 * under the CURRENT row, next to  w t - w / 2  (written once per bound pattern), and the sweep's route -- exact, coordinate
 * descent, conjugate gradients signed or projected, dual -- reads them where it reads w and w t, for that sweep only; no row kernel
 * changes.  Every route starts at the current row and never raises the Jaakkola-Jordan bound, so every sweep lowers the objective
 * (a non-negative factor that is only projected carries no guarantee, as without this block).
 *   cmf_set_logit_pass(ctx, which, enable): `which` 0 = X | 1 = Y (CMF_EINVAL otherwise); enable != 0 sets the flag, 0 clears it and
 *   drops what the pass built.  It may be set before or after cmf_set_relation_loss and acts only while the relation is logistic:
 *   on a Frobenius relation every entry point gives the bits it gives without it.  Cleared by cmf_set_problem; kept when the
 *   weights are bound again.  cmf_get_logit_pass reads it back (CMF_EINVAL for a null output).
 * HONOURED BY every ALS step (cmf_als_step, _nnls_, _cg_, _nncg_, _dual_step) and the row entries cmf_als_cg_rows,
 * cmf_als_nncg_rows, cmf_als_dual_rows and cmf_als_normal (the majoriser's system at the current row).  For routing such a relation
 * counts as a Frobenius one: a V sweep may read a passed logistic X, a fused logistic Y and a Frobenius relation in one launch.
 * With the flag clear every entry point launches and refuses exactly what it does without this block.  Refused with the flag as
 * without it (CMF_EUNSUPPORTED): a logistic relation without CSR weights, with a background weight, with biases, or with a Huber
 * delta; k_pad > 256.  cmf_als_logistic_loss, the residuals and every non-ALS step read the relation as bound.  One GPU; cmf_run is
 * not extended.
 *   cmf_als_logit_weights(ctx, which, t, nnz, w_eff, p_eff) (test entry): w kappa and w t - w / 2 of image t (0 the pattern, 1 its
 *   transpose, each in its stored order) at the current factors, nnz floats each; a null pointer skips that array.  CMF_EINVAL for
 *   a relation that is not logistic or whose flag is clear, or when nnz is not the number of stored entries.
 * The kernel has the layout of the Huber pass (pieces of at most 2048 stored entries, one 256-thread workgroup each, the row in
 * registers, four gathered rows in flight per lane group, the score in float32 in the fixed order of the lane reduction), kappa =
 * |s| < 1e-4 ? 1/4 : tanh(s / 2) / (2 s) by a true division -- the expression of the fused kernel.  No atomics: a repeated call from
 * the same state is bit-identical.  Kernel time: CMF_K_KLMU (2 nnz k_pad flops).                                                */
int cmf_set_logit_pass(cmf_ctx *ctx, int which, int enable);
int cmf_get_logit_pass(cmf_ctx *ctx, int which, int *enabled);
int cmf_als_logit_weights(cmf_ctx *ctx, int which, int t, int64_t nnz, float *w_eff, float *p_eff);

/* sharded form: rank g holds rows of X/U and columns of
 * Y/Z, V replicated.  buf is a DEVICE buffer of cmf_v_buf_elems() floats:
 *   [ X_g^T U_g + Y_g Z_g  (d_pad x k_pad) | U_g^T U_g + Z_g^T Z_g (k_pad x k_pad) ]
 * The caller all-reduces it (RCCL) between the two calls.
 * cmf_solvers.py:242-246 (V numerator/denominator).                        */
int cmf_v_buf_elems(cmf_ctx *ctx, int64_t *n);
int cmf_mu_v_partials(cmf_ctx *ctx, float *dev_buf);
/* (tests, read-only) the fp32 data passes with a 256-wide factor this context has launched so far, by kernel form: out5[0] the
 * 512-thread gemm_kernel, [1] / [2] the TN / NN form of the 256-thread workgroup, [3] / [4] their forms with the factor in a
 * register ring (option "data_pass_wg").  Launches are counted where they are issued: a replayed graph adds none.           */
int cmf_data_pass_launches(cmf_ctx *ctx, int64_t *out5);
/* (tests, read-only) what the routes of cmf_mu_step and of the row-blocked entry points below have launched on this context so
 * far, by form: out8[0] gemm_kernel with the fused EPI_MU epilogue (256-row tiles), [1] factor_update_kernel (64-row tiles, any
 * epilogue), [2] factor_update2_kernel (U and Z in one launch), [3] gemm_pair_kernel (two data passes in one launch), [4] small
 * Grams (one per gram32_partial_kernel + gram32_reduce_kernel pair), [5] sum_slabs_kernel (any caller), [6] mu_apply_kernel,
 * [7] copies of the column-tile image of an in-place fused update over its factor (option "narrow_update").  Counted where the
 * launches are issued: a replayed graph adds none.  The counters change no launch and no result.                            */
int cmf_mu_route_launches(cmf_ctx *ctx, int64_t *out8);
/* the partial of cmf_mu_v_partials for a 256-aligned block of V rows only (dense X, Y), the Gram part when with_gram: lets a
 * sharded driver compute block c + 1 while block c is all-reduced in the background (cmf_comm_allreduce_f32_bg)              */
int cmf_mu_v_partials_rows(cmf_ctx *ctx, float *dev_buf, int64_t row0, int64_t nrows, int with_gram);
int cmf_mu_v_apply(cmf_ctx *ctx, const float *dev_buf, double l1, double l2);
int cmf_mu_uz_update(cmf_ctx *ctx, double l1, double l2, int update_mask);
/* row-blocked V update: the same single sum over the ranks, cut in two around the epilogue (SURVEY.md 8(e) "Partitioning": reduce-
 * scatter + epilogue + all-gather).  Block r of V = rows [r B, (r + 1) B), B = block_rows (a multiple of 256, world * B >= d_pad;
 * cmf_mu_blocked_layout also grows the allocation behind V to world * B rows so that the all-gather runs in place on
 * cmf_factor_dev_ptr(V) -- query that pointer AFTER this call).  Per iteration:
 *   cmf_mu_v_partials_split(P, G)                     P: pbuf_elems floats, zero beyond d_pad rows; G: k_pad^2 floats
 *   all-reduce G (k_pad^2), reduce-scatter P (block_rows * k_pad per rank)
 *   cmf_mu_v_apply_rows(P + r B k_pad, G, r B, rows)  rows = the part of block r inside d_pad (may be 0)
 *   cmf_mu_gram_v_rows(r B, rows, G2); all-reduce G2; all-gather V (block_rows * k_pad per rank)
 *   cmf_mu_uz_update_gram(G2, ...)
 * cmf_solvers.py:242-246, :230-240; the sums over rows are the same sums, regrouped.                                          */
int cmf_mu_blocked_layout(cmf_ctx *ctx, int world, int64_t *block_rows, int64_t *pbuf_elems);
int cmf_mu_v_partials_split(cmf_ctx *ctx, float *dev_P, float *dev_G);
int cmf_mu_v_apply_rows(cmf_ctx *ctx, const float *dev_P_rows, const float *dev_G, int64_t row0, int64_t nrows, double l1, double l2);
int cmf_mu_gram_v_rows(cmf_ctx *ctx, int64_t row0, int64_t nrows, float *dev_G2);
int cmf_mu_uz_update_gram(cmf_ctx *ctx, const float *dev_G2, double l1, double l2, int update_mask);

/* ---- Newton solver: NewtonSolver.update_step, cmf_solvers.py:510-522 --- */
/* sample index lists (parity mode): for sg_ratio < 1 the caller passes the
 * indices the reference would have drawn (cmf_solvers.py:328-344), row after
 * row, as int32: u_idx[m][su] over d, z_idx[p][su] over d,
 * vx_idx[d][sm] over m, vy_idx[d][sp] over p.  NULL when sg_ratio == 1.
 * Every list must hold DISTINCT indices (the reference's permutation()[:s] never repeats one): the shared-partial-sum form of
 * linear sampled sides counts a repeated index once, the row-by-row form once per occurrence.                              */
int cmf_newton_step(cmf_ctx *ctx, double alpha, double l1, double l2,
                    int x_link, int y_link, int nn_mask, int update_mask,
                    double hessian_pertubation, double sg_ratio,
                    const int32_t *u_idx, const int32_t *z_idx,
                    const int32_t *vx_idx, const int32_t *vy_idx);

/* Throughput mode of sg_ratio < 1: the per-row samples (exactly int(n*ratio) distinct
 * candidates per row, uniform) are drawn on the device from a counter-based generator keyed by
 * (seed, sweep, row) -- same distribution as cmf_solvers.py:328-344, not NumPy's stream.       */
int cmf_newton_step_device_sampled(cmf_ctx *ctx, double alpha, double l1, double l2,
                                   int x_link, int y_link, int nn_mask, int update_mask,
                                   double hessian_pertubation, double sg_ratio, uint64_t seed);

/* the index lists that throughput mode draws for rows [row0, row0 + nrows) of one sweep (0: U, lists over d; 1: Z, over d;
 * 2: V / X side, over m; 3: V / Y side, over p): int(n * sg_ratio) ascending indices per row into host memory        */
int cmf_sample_lists(cmf_ctx *ctx, int sweep, uint64_t seed, double sg_ratio, int64_t row0, int64_t nrows, int32_t *host_out);

/* sharded Newton, linear links and sg_ratio == 1 only (same buffer shape as
 * the MU pair: gradient partial | Gram partial).                            */
int cmf_newton_uz_update(cmf_ctx *ctx, double alpha, double l1, double l2,
                         int nn_mask, int update_mask, double hessian_pertubation);
int cmf_newton_v_partials(cmf_ctx *ctx, double alpha, float *dev_buf);
int cmf_newton_v_apply(cmf_ctx *ctx, const float *dev_buf, double l1, double l2,
                       int nn_mask, double hessian_pertubation);

/* The same V sweep in its re-associated, cond(H)-independent form (default of cmf_newton_step; option
 * "newton_reassoc"): the reference's  V - grad Hinv  with  grad = (V G - P) + l1 sign V + l2 V,  H = G + l2 I
 * (cmf_solvers.py:436-450, :321-326) is evaluated as  V (I - H Hinv) + P' - l1 sign(V) Hinv  with
 * P' = X^T (alpha U Hinv) + Y ((1 - alpha) Z Hinv), Hinv applied to the factors in float64 BEFORE the float32 data pass.
 * A row-sharded run sums two buffers over the ranks: gbuf (k_pad^2 float64, device) between _gram and _products, pbuf
 * (d_pad * k_pad float32, device, clobbered by _finish) between _products and _finish.                                   */
int cmf_newton_v_gram(cmf_ctx *ctx, double alpha, double *dev_gbuf);
int cmf_newton_v_products(cmf_ctx *ctx, double alpha, double l2, double hessian_pertubation,
                          const double *dev_gbuf, float *dev_pbuf);
int cmf_newton_v_finish(cmf_ctx *ctx, float *dev_pbuf, double l1, int nn_mask);

/* ---- error metric: compute_factorization_error, cmf_solvers.py:36-42 --- */
/* squared Frobenius residuals of the local shard:
 *   *ex2 = ||X - f(U V^T)||^2, *ey2 = ||Y - f(V Z^T)||^2                    */
int cmf_residual_sq(cmf_ctx *ctx, int x_link, int y_link, double *ex2, double *ey2);
int cmf_data_sq(cmf_ctx *ctx, double *x2, double *y2);  /* ||X||^2, ||Y||^2 */

/* ---- prediction: the n best entries per row / column of X^ = f(U V^T), Y^ = f(V Z^T) ----------------------------------------
 * What a user of a fitted model asks next: for this row, which columns does the model score highest?  The reference stops at the
 * three factor arrays; its only consumer of them is the host argsort of pycmf/analysis.py:3-16 (top terms of a topic), and a user
 * writes np.argpartition(U @ V.T, ...).  Here the product is never materialised: scores are formed tile by tile on the fp32 matrix
 * pipe from the float32 factor blocks the context holds, every query keeps its n best in on-chip memory, and nq x n pairs leave
 * the device (csrc/cmf_topk.hip.h).
 *   cmf_topk: queries = rows `rows[0 .. nq)` of factor `query` (may repeat; rows == NULL: all its rows, nq ignored), candidates =
 *   all rows of factor `cand`.  (query, cand) = (U, V): per row of X^ its best columns; (V, U): per column of X^ its best rows;
 *   (V, Z) / (Z, V): the same of Y^.  Any other pair is CMF_EINVAL.
 *   cmf_topk_queries: the same with caller-supplied query vectors (host float64, nq x k, element (i, t) at Q[i * rs + t * cs] as in
 *   cmf_set_factor_f64): rows folded in by a transform, or the k unit vectors (the top rows of a factor's COLUMNS).  Any `cand`.
 * Result (host, nq x n, row-major): idx[i][t] = the candidate with the t-th largest f(q_i . F[cand]_j), val[i][t] = that value;
 * link = CMF_LINK_LINEAR | CMF_LINK_LOGIT (f = sigmoid; monotone, so the selection runs on the raw score).  The order is total:
 * larger raw float32 score first, equal scores: smaller j first (-0 = +0; a NaN score is never selected).  Every score is one
 * float32 fma chain in a fixed k order, so a query's result is bit-identical when the call is repeated, whichever other queries
 * are in the call and however the candidates are split over workgroups.
 * Exclusion (nullable, both or neither): host CSR over the nq queries -- query i skips the candidates
 * excl_indices[excl_indptr[i] .. excl_indptr[i + 1]), strictly ascending and inside [0, candidates) (checked, CMF_EINVAL).  A query
 * with fewer than n candidates left gets idx = -1, val = -inf in the remaining places.
 * 1 <= n <= min(CMF_TOPK_MAX_N, candidates), otherwise CMF_EINVAL (no truncation).  Needs cmf_set_problem and the factors, no data;
 * modifies no factor, data, option, captured graph or RNG state.  n_components <= 256 (k_pad <= 256).  One GPU: the sharded form
 * (candidates cut over ranks, lists merged) is not built.
 * cmf_topk_layout: how such a call is laid out -- out4 = { queries per workgroup, candidate shares S, queries per launch,
 * device scratch bytes } for nq queries against factor `cand` (excl_nnz < 0: no exclusion lists; own_queries: cmf_topk_queries). */
#define CMF_TOPK_MAX_N 128
int cmf_topk(cmf_ctx *ctx, int query, int cand, int link, const int64_t *rows, int64_t nq, int n,
             const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *idx, float *val);
int cmf_topk_queries(cmf_ctx *ctx, const double *Q, int64_t rs, int64_t cs, int64_t nq, int cand, int link, int n,
                     const int64_t *excl_indptr, const int32_t *excl_indices, int32_t *idx, float *val);
int cmf_topk_layout(cmf_ctx *ctx, int64_t nq, int cand, int n, int64_t excl_nnz, int own_queries, int64_t *out4);

/* ---- held-out ranking evaluation: the exact rank of held-out entries under cmf_topk's order ----
 * How good are the rankings on entries held back from training?  Every ranking metric (recall@n, NDCG@n, MRR, MAP, AUC) is a
 * function of one integer per held-out entry (i, j): its rank.  It is a count over the same score tiles cmf_topk streams, so it is
 * computed exactly, in integers, without the product (csrc/cmf_rank.hip.h).  The reference has no counterpart.
 *   Queries and candidates: as cmf_topk / cmf_topk_queries (the four factor pairs, `rows` -- may repeat; NULL: all rows, nq
 *   ignored --, or caller-supplied vectors).
 *   Held-out entries: host CSR over the nq queries, held_indptr int64[nq + 1], held_indices int32 -- strictly ascending per query,
 *   inside [0, candidates) (checked, CMF_EINVAL).  Exclusion lists (nullable, both or neither): as cmf_topk's.
 *   Order: cmf_topk's, bit for bit -- larger raw float32 score first, -0 counts as +0, equal scores by smaller candidate index, a
 *   NaN-scored candidate is absent.  There is no link argument: the links are monotone.
 *   rank(i, j) = the number of candidates c != j of query i that are not in i's exclusion list and precede j in that order.
 *   0-based: rank r < n <=> j is entry r of cmf_topk's list under the same exclusion list.  Whether j itself is in the exclusion
 *   list is ignored here.  A held-out entry whose own score is NaN gets rank -1.
 * Outputs (host): rank int32[held_nnz] and score float32[held_nnz] (the raw score; nullable) in the order of held_indices,
 * eligible int32[nq] = candidates - length of the query's exclusion list.
 * Every score -- a held-out entry's own included -- is the fma chain of cmf_topk (the same matrix instruction sequence and k
 * pairing), so ranks and cmf_topk agree bit for bit; counts are integers, summed without atomics: the result is bit-identical when
 * the call is repeated, whichever other queries are in the call and however the candidates are split ("topk_split" fixes the
 * number of shares S of these calls too).  A query with more than HB held-out entries is scanned as several virtual queries.
 * Needs cmf_set_problem and the factors, no data; modifies no factor, data, option, captured graph or RNG state.  k_pad <= 256.
 * One GPU.  Kernel time goes to class CMF_K_TOPK, 2 (virtual queries) C k flops per scan.
 * cmf_rank_layout: out4 = { HB, candidate shares S, virtual queries per launch, device scratch bytes } for nq queries with held_nnz
 * held-out entries against factor `cand` (excl_nnz < 0: no exclusion lists; own_queries: cmf_rank_queries). */
int cmf_rank(cmf_ctx *ctx, int query, int cand, const int64_t *rows, int64_t nq,
             const int64_t *held_indptr, const int32_t *held_indices,
             const int64_t *excl_indptr, const int32_t *excl_indices,
             int32_t *rank, float *score, int32_t *eligible);
int cmf_rank_queries(cmf_ctx *ctx, const double *Q, int64_t rs, int64_t cs, int64_t nq, int cand,
             const int64_t *held_indptr, const int32_t *held_indices,
             const int64_t *excl_indptr, const int32_t *excl_indices,
             int32_t *rank, float *score, int32_t *eligible);
int cmf_rank_layout(cmf_ctx *ctx, int64_t nq, int cand, int64_t held_nnz, int64_t excl_nnz, int own_queries, int64_t *out4);

/* ---- batched safe inverse (exposed for tests): _safe_invert :346-356 --- */
/* H: n symmetric k x k float64 matrices (host), out: Q diag(1/max(|l|,pert)) Q^T */
int cmf_safe_invert_batch(cmf_ctx *ctx, const double *H, double *out, int n, int k, double pert);
/* The step of _row_newton_update (:321-326) for n independent rows: out_b = g_b * safe_inverse(H_b) (H: n symmetric k x k
 * float64 host matrices, g / out: n x k), through the float32 path the per-row sweeps take.  method 0: the sweeps' own dispatch
 * (Cholesky where lambda_min >= pert, the clamp path for the rest); 1: every matrix through the tridiagonal eigen-solve
 * (cmf_eigclamp.hip.h; 64 < k <= 256), lam (nullable, n x k) receives its eigenvalues in the order the QL iteration left them. */
int cmf_safe_solve_batch(cmf_ctx *ctx, const double *H, const double *g, double *out, double *lam, int n, int k,
                         double pert, int method);

/* Conditioning record of the per-row Newton sweeps.  The spectral clamp of _safe_invert (pycmf/cmf_solvers.py:346-356) acts on a
 * row's Hessian only when its smallest eigenvalue is below `pert`; on the device that Hessian is a float32 matrix, whose
 * eigenvalues are resolved to about eps32 * ||H||, so the clamped directions of the inverse carry a relative error of the order
 * eps32 * ||H|| / pert (the reference works in float64).  rows = matrices the float32 clamp acted on since the last reset,
 * max_ratio = the largest ||H||_F / pert among them (0 when there were none).  The stated tolerances hold
 * for max_ratio up to ~1e4.  Clamped rows above 3e3 (option "refine_rows_ratio"; plain solves above a condition estimate of 1e3,
 * "refine_rows_cond") are REDONE IN FLOAT64 (Hessian from float64 sums,
 * float64 clamp, float64 step; option "refine_rows", default on, at most "refine_rows_max" = 16384 rows per sweep, k <= 256) and
 * counted in `refined` instead; only rows left in float32 enter rows / max_ratio, and the estimator warns when max_ratio
 * exceeds 1e4.  The shared Hessians of the linear unsampled sweeps are formed and clamped in float64 and never appear here.
 * plain_cond: the largest condition estimate max H_ii / min L_ii^2 (<= cond(H)) over ALL rows solved by plain Cholesky -- rows above
 * the refinement ratio by that estimate are refined too; the ones left in float32 also enter max_ratio. */
int cmf_newton_clamp_stats(cmf_ctx *ctx, int64_t *rows, double *max_ratio, int64_t *refined, double *plain_cond, int reset);
/* Which route the rows flagged by the threshold test took through _safe_invert's clamp (pycmf/cmf_solvers.py:346-356) since the
 * context was created: eigen_rows through the tridiagonal eigen-solve (Householder + QL, any spectrum), rank1_rows through the
 * rank-one shortcut (one eigenvalue above pert, every other one certified below it by a Cholesky factorisation of
 * (pert - delta) I - (H - lambda_1 q q^T); positive semi-definite Hessians at k_pad = 256; option "rank1_clamp", default on). */
int cmf_newton_clamp_routes(cmf_ctx *ctx, int64_t *eigen_rows, int64_t *rank1_rows);

/* float64 path of the ONE shared Hessian of a linear-link sweep (cmf_solvers.py:407-410, :448-450): H is k x k
 * float64 on the host, k = the problem's n_components; out = Q diag(1/max(|l|,pert)) Q^T computed in float64 on
 * the device (positive semi-definite H), returned after its rounding to float32 (the form the step product uses) */
int cmf_safe_invert_f64(cmf_ctx *ctx, const double *H, double *out, int k, double pert);

/* ---- measurement ------------------------------------------------------ */
/* when enabled every kernel launch is bracketed by hipEvents on the context's
 * stream; cmf_kernel_time returns accumulated ms, launch count and algorithmic
 * flops (2*M*N*K of every GEMM launched, 0 for the other classes) per class.
 * enable = 2: only the data-pass classes (GEMM_NN, GEMM_TN, SPMM, ROWHESS) are
 * bracketed -- an event pair costs a few microseconds of stream serialisation per
 * launch, 7 % of a 0.9 ms iteration with 11 launches                          */
int cmf_kernel_timing(cmf_ctx *ctx, int enable);
int cmf_kernel_time(cmf_ctx *ctx, int kernel_class, double *ms, int64_t *launches, double *flops);
int cmf_kernel_timing_reset(cmf_ctx *ctx);
/* per-row Newton accounting since the last reset, counted while timing is enabled: `credited` = sample rows of the
 * algorithm (sum over updated rows of their list lengths, pycmf/cmf_solvers.py:414-428 runs one outer product per such
 * pair), `gathered` = sample rows that actually went through the outer-product kernel (fewer when linear sampled sides
 * share partial sums between rows: option "row_classes")                                                           */
int cmf_rowhess_samples(cmf_ctx *ctx, double *credited, double *gathered);
/* stream markers (bench.py's per-iteration time series, auditable beside the whole-region clock): cmf_marker records an
 * event on the launch stream; cmf_marker_times waits for the stream, writes the elapsed ms of every marker since the
 * first one (at most cap entries), stores the marker count in *n and clears the list                                */
int cmf_marker(cmf_ctx *ctx);
int cmf_marker_times(cmf_ctx *ctx, double *ms, int64_t cap, int64_t *n);
/* the hipStream_t the context launches on (its own, or the one given to cmf_ctx_create): a caller that enqueues
 * collectives between the *_partials / *_apply calls orders them on this stream                                      */
int cmf_get_stream(cmf_ctx *ctx, void **stream);
/* diagnostic: one X*V data pass with s_memtime / s_memrealtime stamps around the main loop;
 * median in-kernel shader clock (GHz) and main-loop duration (us) over the workgroups        */
int cmf_debug_clock(cmf_ctx *ctx, double *ghz, double *loop_us);
/* padded device geometry (m_pad, d_pad, p_pad, k_pad) */
int cmf_get_geometry(cmf_ctx *ctx, int64_t *m_pad, int64_t *d_pad, int64_t *p_pad, int *k_pad);
/* device pointers of the factor blocks (float32, row-major, ld = k_pad) */
int cmf_factor_dev_ptr(cmf_ctx *ctx, int which, float **ptr);
/* zero-filled device scratch owned by the context: the partial / staging buffer of the sharded entry points when the
 * caller brings no device allocator (bench.py at N = 1 runs without PyTorch); freed by cmf_scratch_free, by the next
 * cmf_set_problem or by cmf_ctx_destroy                                                                             */
int cmf_scratch_alloc(cmf_ctx *ctx, int64_t bytes, void **dev_ptr);
int cmf_scratch_free(cmf_ctx *ctx, void *dev_ptr);
/* device-to-device copies of all valid rows of a factor, k_pad floats per row, on the context's stream:
 * what a row-sharded Newton driver exchanges between its U/Z-sweep and V-sweep contexts
 * (the reference keeps U, V, Z in one address space: cmf_solvers.py:510-522)                      */
int cmf_export_factor_rows(cmf_ctx *ctx, int which, float *dev_dst);
int cmf_import_factor_rows(cmf_ctx *ctx, int which, const float *dev_src);


/* ---- the outer loop: _IterativeCMFSolver.fit_iterative_update, pycmf/cmf_solvers.py:132-195 --------------------------------
 * error at init (:170); for n_iter = 1 .. max_iter: one update_step (:172) -- cmf_mu_step, cmf_newton_step, or
 * cmf_newton_step_device_sampled(seed + n_iter) when sg_ratio < 1 (host-drawn index lists cannot enter here: that configuration
 * keeps its loop on the host) --; every check_every-th iteration (the reference: 10) when tol > 0 the error
 * alpha_err ||X - f(U V^T)||_F + (1 - alpha_err) ||Y - f(V Z^T)||_F (:128-130) and the stopping test
 * (previous - error) / error_at_init < tol (:183-186).  *n_iter = the iteration the loop stopped at (max_iter when it ran out,
 * exactly Python's loop variable).  err_trace / time_trace (nullable, trace_cap entries each): the error at init and at every
 * check, and the seconds since the call started at those points; *n_trace = how many there were.  One 16-byte read-back per
 * check is all that crosses the boundary; the step body is replayed from a hipGraph where it is a fixed launch sequence.      */
enum { CMF_SOLVER_MU = 0, CMF_SOLVER_NEWTON = 1 };
typedef struct {
    int solver;                 /* CMF_SOLVER_MU | CMF_SOLVER_NEWTON */
    double l1, l2;
    double alpha;               /* Newton: weight of the X side (cmf_solvers.py:510-522); MU: unused */
    double alpha_err;           /* weight of the X side in the error metric (MU: the constructor default 0.5, :99) */
    int x_link, y_link;         /* CMF_LINK_* (MU: both linear) */
    int nn_mask, update_mask;
    double hessian_pertubation, sg_ratio;
    uint64_t seed;              /* device sampler: iteration n_iter draws under seed + n_iter */
} cmf_run_params;
int cmf_run(cmf_ctx *ctx, const cmf_run_params *params, int max_iter, double tol, int check_every, int *n_iter,
            double *err_trace, double *time_trace, int trace_cap, int *n_trace);

/* ---- collectives of the sharded solvers: RCCL over xGMI, one communicator per context -------------
 * The reference is single-process; what is replaced here is the sum over row blocks hidden in its products
 * (cmf_solvers.py:242-246: X^T U + Y Z and U^T U + Z^T Z are sums over the rows each rank owns).  librccl.so.1 is loaded on the
 * first call (no link-time dependency).  Every collective is enqueued on the context's stream.  Bootstrap: one rank calls
 * cmf_comm_unique_id and hands the 128 bytes to the others out of band (pycmf_amd/comm.py: a file next to the job), then every
 * rank calls cmf_comm_init on its own context (one process per GPU).                                                        */
#define CMF_COMM_ID_BYTES 128
int cmf_comm_unique_id(char *id128);
int cmf_comm_init(cmf_ctx *ctx, int rank, int world, const char *id128);
int cmf_comm_destroy(cmf_ctx *ctx);                 /* also done by cmf_ctx_destroy */
int cmf_comm_info(cmf_ctx *ctx, int *rank, int *world);
/* in-place sum over the ranks (device memory): the (d + k) k partial buffer of cmf_mu_v_partials / cmf_newton_v_partials, the
 * d k buffer of cmf_newton_v_products (float32); the k^2 Gram of cmf_newton_v_gram (float64)                                */
int cmf_comm_allreduce_f32(cmf_ctx *ctx, float *dev_buf, int64_t n);
int cmf_comm_allreduce_f64(cmf_ctx *ctx, double *dev_buf, int64_t n);
/* the float32 all-reduce in the background: on a side stream, behind what the context's stream holds at the call; kernels
 * launched on the context's stream afterwards overlap with it.  cmf_comm_join: the context's stream waits for all of them.
 * cmf_comm_exposed_ms: time that stream spent waiting in joins (while cmf_comm_timing) -- the exposed part; the rest of the
 * collectives' duration (cmf_comm_stats) was hidden under compute                                                              */
int cmf_comm_allreduce_f32_bg(cmf_ctx *ctx, float *dev_buf, int64_t n);
int cmf_comm_join(cmf_ctx *ctx);
int cmf_comm_exposed_ms(cmf_ctx *ctx, double *ms, int reset);
/* in-place all-gather of equal chunks (factor rows of the row-sharded Newton): rank r's elems_per_rank floats already sit at
 * dev_full + r * elems_per_rank                                                                                             */
int cmf_comm_allgather_f32(cmf_ctx *ctx, float *dev_full, int64_t elems_per_rank);
/* in-place reduce-scatter of equal chunks: every rank holds world * elems_per_rank floats; afterwards chunk `rank` of the rank's
 * own buffer is the sum over the ranks of that chunk.  With cmf_comm_allgather_f32 on the updated rows it is the ONE all-reduce of
 * the MU V update (cmf_solvers.py:242-246) cut in two around the row-blocked epilogue (cmf_mu_v_apply_rows)                   */
int cmf_comm_reduce_scatter_f32(cmf_ctx *ctx, float *dev_full, int64_t elems_per_rank);
/* ncclGroupStart / ncclGroupEnd around the collectives enqueued in between: ONE launch point on the context's stream.  The
 * row-blocked MU iteration (cmf_solvers.py:242-246 cut around the epilogue) is two groups: {all-reduce of U^T U + Z^T Z,
 * reduce-scatter of X^T U + Y Z} and {all-reduce of the ranks' shares of V^T V, all-gather of V}.  cmf_comm_launch_points:
 * collectives outside groups + groups since the last cmf_comm_stats(reset)                                                    */
int cmf_comm_group_start(cmf_ctx *ctx);
int cmf_comm_group_end(cmf_ctx *ctx);
int cmf_comm_launch_points(cmf_ctx *ctx, int64_t *n);
/* what RCCL reports about the communicator (ncclCommCount, ncclCommUserRank) -- not what the launcher's environment says   */
int cmf_comm_count(cmf_ctx *ctx, int *ranks_seen, int *rank_seen);
/* at most 16 host scalars, op 0 = sum, 1 = max; waits for the result (convergence test on the global error, the slowest
 * rank's clock of bench.py); cmf_comm_barrier = one such reduction                                                          */
int cmf_comm_allreduce_host_f64(cmf_ctx *ctx, double *vals, int n, int op);
int cmf_comm_barrier(cmf_ctx *ctx);
/* accounting: calls and payload bytes since the last reset; with cmf_comm_timing(1) also the milliseconds the collectives
 * occupied the stream (events around each one, waiting for the slowest rank included)                                       */
int cmf_comm_timing(cmf_ctx *ctx, int enable);
int cmf_comm_stats(cmf_ctx *ctx, int64_t *calls, int64_t *bytes, double *ms, int reset);
/* the same per kind of collective (no reset: read before cmf_comm_stats(..., 1))                                            */
enum { CMF_COMM_ALLREDUCE_F32 = 0, CMF_COMM_ALLREDUCE_F64 = 1, CMF_COMM_ALLGATHER_F32 = 2, CMF_COMM_REDUCE_SCATTER_F32 = 3, CMF_COMM_GROUP = 4, CMF_COMM_KINDS = 5 };
int cmf_comm_stats_kind(cmf_ctx *ctx, int kind, int64_t *calls, int64_t *bytes, double *ms);
/* dev[0 .. n) *= factor on the context's stream (the measurement double of the collectives stands in for the peers with the
 * rank's own partial times the world size: finite iterates without a communicator)                                           */
int cmf_scale_f32(cmf_ctx *ctx, float *dev, int64_t n, double factor);
/* raw copies between caller-held device pointers (scratch, partial buffers) and host memory on the context's stream; both wait */
int cmf_copy_to_host(cmf_ctx *ctx, const void *dev, void *host, int64_t bytes);
int cmf_copy_from_host(cmf_ctx *ctx, void *dev, const void *host, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* CMFHIP_H */
