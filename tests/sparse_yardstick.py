"""NumPy float64 yardstick for the native CSR kernels taken one product at a time (csrc/cmf_sparse.hip.h): the row-gather SpMM
out = op(A) B and the SDDMM behind the error metric of a sparse side, ||A - f(L R^T)||^2.  No device, no project code.

Two families of inputs:

  exact   matrix values in {+-1/2, +-1, +-2, 4}, operand entries integers in [-8, 8], factors whose entries are +-2^e with
          e in {-1, 0, 1}: every term is a multiple of 1/8 and every partial sum, in any order, stays far below 2^24 of them, so
          float32 arithmetic in ANY order of summation gives the float64 value bit for bit -- a kernel is compared with ==
  random  float32-rounded, signed, magnitudes kept away from zero -- a kernel is held to a per-element rounding bound

and the bounds:

  product_bound    (L + 16) 2^-24 sum|terms| per output element, L the stored length of the row that is summed: L float32
                   products added in any order (gamma_L of the textbook analysis), the partial sums of up to 16 pieces added
                   afterwards (the rule test_rows_cut_into_pieces of test_gpu_als.py holds the ALS systems to)
  residual_bound   for the linear expansion ||A||^2 - 2 sum_nnz a (l . r) + <L^T L, R^T R> as sparse_residual_sq evaluates it

The case builders of the GPU tests live here too, so that tests/test_sparse_yardstick_host.py can check on the CPU that every
case is one in which a dropped or doubled entry cannot hide below the bound."""
import numpy as np
import scipy.sparse as sp

U24 = 2.0 ** -24
EXACT_VALUES = np.array([-0.5, 0.5, -1.0, 1.0, -2.0, 2.0, 4.0])


def f32(a):
    """Rounded to float32, kept as float64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def pad_k(k):
    """The padded width of an operand of k columns (cmf_set_problem, cmf_data_matmul_f64)."""
    return 32 if k <= 32 else 64 if k <= 64 else 128 if k <= 128 else (k + 255) // 256 * 256


# ------------------------------------------------------------------ inputs
def pattern(lengths, cols, rng, avoid=()):
    """(indptr, indices) of a CSR pattern whose row i holds lengths[i] distinct ascending columns of range(cols), none of them
    in ``avoid``."""
    allowed = np.setdiff1d(np.arange(cols), np.asarray(avoid, dtype=np.int64))
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.max(initial=0) <= allowed.size, "a row is longer than the columns it may use"
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    rows = [np.sort(rng.choice(allowed, n, replace=False)) for n in lengths]
    return indptr, (np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64))


def values(n, family, rng, unit=False):
    """n matrix values: the exact family, or signed float32 with magnitudes in [0.5, 1.5) (``unit``: in (0, 1), logit targets)."""
    if family == "exact":
        return rng.choice(EXACT_VALUES, n)
    if unit:
        return f32(0.05 + 0.9 * rng.rand(n))
    return f32((0.5 + rng.rand(n)) * rng.choice([-1.0, 1.0], n))


def matrix(lengths, cols, family, rng, avoid=(), unit=False):
    """CSR matrix (float64 container) with the given row lengths and value family."""
    indptr, indices = pattern(lengths, cols, rng, avoid)
    return sp.csr_matrix((values(indices.size, family, rng, unit), indices, indptr), shape=(len(lengths), cols))


def operand(rows, cols, family, rng):
    """Right-hand side of a product.  exact: integers in [-8, 8].  random: signed float32, magnitudes in [1/32, 1/16) with one
    entry per row, at column row % cols, in [1, 2): the column in which the row's matrix entries stand out against the
    rounding bound of even a row of 3000 terms (see single_entry_visibility)."""
    if family == "exact":
        return rng.randint(-8, 9, (rows, cols)).astype(np.float64)
    B = (1.0 + rng.rand(rows, cols)) / 32.0
    B[np.arange(rows), np.arange(rows) % cols] = 1.0 + rng.rand(rows)
    return f32(B * rng.choice([-1.0, 1.0], (rows, cols)))


def exact_factor(rows, k, period, salt):
    """Power-of-two rows in the manner of _exact_factor of test_gpu_als.py, but not one-hot: row j holds +-2^e, e in
    {-1, 0, 1}, at every column c with (c + j + salt) % period == 0.  Two factors with coprime periods meet in about
    k / (period_L period_R) columns for EVERY pair of rows, so no stored entry has an empty dot product at k = 1000 (the three
    entries per row of _exact_factor would almost never meet a row of the other factor there).  Asymmetric in row and column."""
    j, c = np.meshgrid(np.arange(rows), np.arange(k), indexing="ij")
    mag = 2.0 ** ((c + 2 * j) % 3 - 1)
    sign = np.where((7 * c + j) % 5 < 2, -1.0, 1.0)
    return np.where((c + j + salt) % period == 0, sign * mag, 0.0)


def random_factor(rows, k, rng, scale=0.125):
    """Signed float32 factor for the SDDMM.  One column (k // 2) carries magnitudes in [0.75, 1) * scale, the others fall off as
    scale / (8 (1 + distance)): a dot product of two such rows does not cancel (|l . r| is within a tenth of |l| . |r|), which
    is what keeps one stored entry of 1300 above the rounding bound of the whole cross term at k_pad = 1024."""
    c0 = k // 2
    F = (0.75 + 0.25 * rng.rand(rows, k)) / (8.0 * (1.0 + np.abs(np.arange(k) - c0)))[None, :]
    F[:, c0] = 0.75 + 0.25 * rng.rand(rows)
    return f32(scale * F * rng.choice([-1.0, 1.0], (rows, k)))


def logit_factor(rows, k, signs, rng, dot=2.0):
    """Signed float32 factor for the logit SDDMM: entry (j, c) is signs[c] * sqrt(dot / k) * [0.75, 1.25).  Two factors built on
    the same column signs have l . r of about +dot for every pair of rows, every column adding its share with the same sign: a
    part of the columns missing from the dot products moves every sigmoid the same way, and the sum cannot hide it."""
    return f32(np.asarray(signs, dtype=np.float64)[None, :] * np.sqrt(dot / k) * (0.75 + 0.5 * rng.rand(rows, k)))


# ------------------------------------------------------------------ SpMM
def product(A, B, trans=False):
    """op(A) B in float64."""
    A = sp.csr_matrix(A, dtype=np.float64)
    return np.asarray((A.T.tocsr() if trans else A) @ np.asarray(B, dtype=np.float64))


def abs_product(A, B, trans=False):
    """sum |terms| of every output element."""
    return product(abs(sp.csr_matrix(A, dtype=np.float64)), np.abs(B), trans)


def stored_lengths(A, trans=False):
    """Stored entries of every row of op(A)."""
    A = sp.csr_matrix(A)
    return np.bincount(A.indices, minlength=A.shape[1]) if trans else np.diff(A.indptr)


def product_bound(L, abs_terms):
    """(L + 16) 2^-24 sum|terms|; L per output row (a vector) or one number."""
    L = np.asarray(L, dtype=np.float64)
    return (L.reshape(-1, 1) + 16.0) * U24 * abs_terms if L.ndim else (L + 16.0) * U24 * abs_terms


def worst_ratio(got, A, B, trans=False):
    """max |got - product| / product_bound over the elements whose bound is not zero; where it is zero (no stored entry, or only
    zero terms) the element has to be exactly zero, else the ratio is inf."""
    ref = product(A, B, trans)
    bound = product_bound(stored_lengths(A, trans), abs_product(A, B, trans))
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if (err[bound == 0] != 0).any():
        return np.inf
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


def product_f32(A, B, trans=False, order="forward", pieces=3):
    """op(A) B with float32 products and float32 sequential sums, in one of three orders per output row: its stored entries
    ``forward``, in ``reverse``, or ``interleaved``: piece i takes every pieces-th entry from the i-th on (the cut of
    bcsr_build_upload), each piece summed forward, the pieces added in order."""
    M = sp.csr_matrix(A, dtype=np.float64)
    M = M.T.tocsr() if trans else M
    M.sort_indices()
    B32 = np.asarray(B, dtype=np.float32)
    out = np.zeros((M.shape[0], B32.shape[1]), dtype=np.float32)
    seq = lambda T: np.add.accumulate(T, axis=0, dtype=np.float32)[-1] if len(T) else np.zeros(B32.shape[1], dtype=np.float32)
    for i in range(M.shape[0]):
        lo, hi = M.indptr[i], M.indptr[i + 1]
        T = M.data[lo:hi].astype(np.float32)[:, None] * B32[M.indices[lo:hi]]
        if order == "forward":
            out[i] = seq(T)
        elif order == "reverse":
            out[i] = seq(T[::-1])
        else:
            out[i] = seq(np.stack([seq(T[s::pieces]) for s in range(pieces)]))
    return out.astype(np.float64)


def single_entry_visibility(A, B, trans=False):
    """For every stored entry of A: the largest, over the output elements it feeds, of |its term| / product_bound of that
    element -- how far removing (or doubling) that entry alone would move the product, in units of the bound.  Returns the
    smallest of these over the entries."""
    M = sp.csr_matrix(A, dtype=np.float64)
    M = (M.T.tocsr() if trans else M).tocoo()
    bound = product_bound(stored_lengths(A, trans), abs_product(A, B, trans))
    worst = np.inf
    for lo in range(0, M.nnz, 4096):
        r, c, v = M.row[lo:lo + 4096], M.col[lo:lo + 4096], M.data[lo:lo + 4096]
        term = np.abs(v)[:, None] * np.abs(np.asarray(B, dtype=np.float64)[c])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(term > 0, term / bound[r], 0.0)
        worst = min(worst, float(ratio.max(axis=1).min()))
    return worst


# ------------------------------------------------------------------ SDDMM / error metric
def residual_sq(A, L, R, link="linear"):
    """||A - f(L R^T)||^2 over all cells, directly."""
    P = np.asarray(L, dtype=np.float64) @ np.asarray(R, dtype=np.float64).T
    if link == "logit":
        P = 1.0 / (1.0 + np.exp(-P))
    D = sp.csr_matrix(A, dtype=np.float64).toarray() - P
    return float((D * D).sum())


def cross_terms(A, L, R):
    """a_ij (l_i . r_j) of every stored entry, and |a_ij| (|l_i| . |r_j|), float64, in CSR order."""
    M = sp.csr_matrix(A, dtype=np.float64).tocoo()
    L, R = np.asarray(L, dtype=np.float64), np.asarray(R, dtype=np.float64)
    return M.data * (L[M.row] * R[M.col]).sum(axis=1), np.abs(M.data) * (np.abs(L[M.row]) * np.abs(R[M.col])).sum(axis=1)


def residual_bound(A, L, R):
    """Rounding bound of the LINEAR expansion as sparse_residual_sq evaluates it:
        2^-24 [2 (k_pad + L_max + 16) C_abs + (rows_L + rows_R + 32) Q_abs],
    C_abs = sum_nnz |a| (|l| . |r|), Q_abs = <|L|^T |L|, |R|^T |R|>.  The cross term is a float32 dot product of k_pad terms per
    stored entry (k_pad roundings), added per lane over a row in float32 (at most L_max, the longest row), the lanes then in
    float64; it enters the result twice.  The two Grams are float32 sums over the padded factor rows (rows rounded up to 256),
    32 for however the matrix pipe orders them; each Gram's error multiplies the other's magnitude.  ||A||^2, the inner product of
    the Grams and the final sum are float64."""
    M = sp.csr_matrix(A)
    L, R = np.abs(np.asarray(L, dtype=np.float64)), np.abs(np.asarray(R, dtype=np.float64))
    c_abs = cross_terms(A, L, R)[1].sum()
    q_abs = float(((L.T @ L) * (R.T @ R)).sum())
    lmax = int(np.diff(M.indptr).max(initial=0))
    rup = lambda n: (n + 255) // 256 * 256
    return U24 * (2.0 * (pad_k(L.shape[1]) + lmax + 16) * c_abs + (rup(L.shape[0]) + rup(R.shape[0]) + 32) * q_abs)


def residual_sq_f32(A, L, R):
    """The linear expansion with float32 dot products, float32 row sums and float32 Grams (NumPy's own orders), the rest in
    float64 -- the arithmetic of sparse_residual_sq in another order."""
    M = sp.csr_matrix(A, dtype=np.float64)
    M.sort_indices()
    L32, R32 = np.asarray(L, dtype=np.float32), np.asarray(R, dtype=np.float32)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    dots = (L32[rows] * R32[M.indices]).sum(axis=1, dtype=np.float32)
    terms = M.data.astype(np.float32) * dots
    cross = 0.0
    for i in range(M.shape[0]):
        cross += float(terms[M.indptr[i]:M.indptr[i + 1]].sum(dtype=np.float32))
    q = float(((L32.T @ L32).astype(np.float64) * (R32.T @ R32).astype(np.float64)).sum())
    return float((f32(M.data) ** 2).sum()) - 2.0 * cross + q


def residual_sq_logit_f32(A, L, R):
    """||A||^2 - 2 sum_nnz a sigmoid(l . r) + sum_all sigmoid(l . r)^2 with float32 dot products and sigmoids, float64 sums."""
    M = sp.csr_matrix(A, dtype=np.float64).tocoo()
    L32, R32 = np.asarray(L, dtype=np.float32), np.asarray(R, dtype=np.float32)
    S = (np.float32(1) / (np.float32(1) + np.exp(-(L32 @ R32.T)))).astype(np.float32)
    return float((M.data ** 2).sum() - 2.0 * (M.data * S[M.row, M.col].astype(np.float64)).sum() + (S.astype(np.float64) ** 2).sum())


def logit_lane_visibility(A, L, R):
    """sddmm_cross_kernel spreads the k_pad columns of a dot product over GL = min(64, k_pad / 4) lanes (lane g holds columns
    4 (g + GL c) .. + 3 of every chunk c) and, under the logit link, adds the lanes by log2(GL) exchange steps before the sigmoid.
    For every step (distance off = 1, 2, .. GL / 2) that moves real columns: the root of the squared residual with the columns of
    the lanes g & off != 0 missing from the dot products of the cross term, as a relative distance from the true root.  Returns
    the smallest of them: how far the least visible lost exchange step moves what the test compares."""
    M = sp.csr_matrix(A, dtype=np.float64).tocoo()
    L, R = np.asarray(L, dtype=np.float64), np.asarray(R, dtype=np.float64)
    k = L.shape[1]
    gl = min(64, pad_k(k) // 4)
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))
    rest = float((M.data ** 2).sum() + (sig(L @ R.T) ** 2).sum())
    root = np.sqrt(rest - 2.0 * (M.data * sig((L[M.row] * R[M.col]).sum(axis=1))).sum())
    lane = (np.arange(k) // 4) % gl
    least = np.inf
    off = 1
    while off < gl:
        keep = (lane & off) == 0
        if not keep.all():
            cross = (M.data * sig((L[M.row][:, keep] * R[M.col][:, keep]).sum(axis=1))).sum()
            least = min(least, abs(np.sqrt(max(rest - 2.0 * cross, 0.0)) - root) / root)
        off *= 2
    return least


# ------------------------------------------------------------------ the cases of tests/test_gpu_sparse_products.py
ROW_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 33, 70, 300)        # the 4-way unroll of spmm_csr_kernel and its tail of 0 .. 3
ROW_SHAPE = (77, 300, 45)                               # 77 rows: no multiple of 1, 2, 4 or 8 rows per wave
ROW_WIDTHS = (7, 40, 100, 200, 300, 600, 1000)          # pad to 32, 64, 128, 256, 512, 768, 1024


def row_case(family):
    """X (77 x 300) and Y (300 x 45) of the row-kernel test.  X: row lengths cycling through ROW_LENGTHS over the first 70 rows,
    the last 7 rows empty.  A row of 300 entries fills all 300 columns, so X cannot also have an empty column; Y carries it (its
    column 17 and its last 9 rows are empty, lengths cycling through 0 .. 45 otherwise), and Y^T B walks it as an empty row in
    the middle of the transposed image."""
    m, d, p = ROW_SHAPE
    rng = np.random.RandomState(41 if family == "exact" else 43)
    X = matrix(np.concatenate([np.resize(ROW_LENGTHS, 70), np.zeros(7, dtype=np.int64)]), d, family, rng)
    ylen = np.concatenate([np.resize([0, 1, 2, 3, 5, 8, 13, 44], d - 9), np.zeros(9, dtype=np.int64)])
    Y = matrix(ylen, p, family, rng, avoid=(17,))
    return X, Y


def row_operand(which, trans, width, family):
    m, d, p = ROW_SHAPE
    rows = ((d, m), (p, d))[which][1 if trans else 0]
    rng = np.random.RandomState(1000 * width + 10 * which + int(trans) + (0 if family == "exact" else 5))
    return operand(rows, width, family, rng)


BLOCK_SHAPE = (100, 3072)
BLOCK_COLS = 64
BLOCK_EMPTY = 10                                         # the 64-column block without entries: columns 640 .. 703
BLOCK_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 129)      # the 16-gather chunks and the 64-entry metadata batches
BLOCK_HOT = (1280, 1281, 2049, 3000)                     # not split / two pieces / three pieces / three pieces at a share of 1024


def blocked_case(family):
    """M (100 x 3072) of the blocked-kernel test: rows 3, 31, 58 and 96 hold BLOCK_HOT entries, the others cycle through
    BLOCK_LENGTHS (mean row length about 115 < 128: a piece stays at its floor of 1024 entries), no entry in column block 10."""
    rows, cols = BLOCK_SHAPE
    rng = np.random.RandomState(51 if family == "exact" else 53)
    lengths = np.resize(BLOCK_LENGTHS, rows)
    lengths[[3, 31, 58, 96]] = BLOCK_HOT
    assert lengths.mean() < 128
    return matrix(lengths, cols, family, rng, avoid=np.arange(BLOCK_EMPTY * BLOCK_COLS, (BLOCK_EMPTY + 1) * BLOCK_COLS))


def blocked_operand(rows, width, family):
    return operand(rows, width, family, np.random.RandomState(7 * rows + width + (0 if family == "exact" else 3)))


def split_layout(lengths, rows_per_group):
    """(split rows, pieces, share) that bcsr_build_upload gives rows of these lengths: share = max(1024, floor(nnz / rows *
    G / 32)); a row longer than share + share / 4 is cut into ceil(len / share) pieces."""
    lengths = np.asarray(lengths, dtype=np.int64)
    share = max(1024, int(lengths.sum() / max(len(lengths), 1) * rows_per_group / 32))
    cut = lengths[lengths > share + share // 4]
    return int(cut.size), int(((cut + share - 1) // share).sum()), share


SDDMM_SHAPE = (130, 170, 40)
SDDMM_KS = (7, 40, 100, 200, 300, 600, 1000)


def sddmm_case(k, family, link="linear"):
    """X (130 x 170, about 6 % dense: row lengths 0 .. 20 with rows of length 0 inside and a trailing empty row), Y (170 x 40)
    and the three factors.  Under the logit link the family is "random" whatever is asked for: targets in (0, 1), factors by
    logit_factor (signed, every dot product about +2)."""
    m, d, p = SDDMM_SHAPE
    unit = link == "logit"
    if unit:
        family = "random"
    rng = np.random.RandomState(61 + k + (0 if family == "exact" else 1000) + (5000 if unit else 0))
    xlen = rng.randint(1, 21, m)
    xlen[[5, 64, 65, m - 1]] = 0
    ylen = rng.randint(0, 8, d)
    ylen[d - 1] = 0
    X = matrix(xlen, d, family, rng, unit=unit)
    Y = matrix(ylen, p, family, rng, unit=unit)
    if family == "exact":
        F = [exact_factor(m, k, 2, 1), exact_factor(d, k, 3, 0), exact_factor(p, k, 2, 0)]
    elif unit:
        signs = rng.choice([-1.0, 1.0], k)
        F = [logit_factor(n, k, signs, rng) for n in (m, d, p)]
    else:
        F = [random_factor(n, k, rng) for n in (m, d, p)]
    return X, Y, F
