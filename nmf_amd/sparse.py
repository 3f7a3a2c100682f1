"""Sparse input (scipy.sparse matrices and arrays of any format) for MUR.

`normalise` turns the caller's matrix into a canonical CSR copy -- duplicates summed, stored zeros dropped, column
indices sorted -- and validates it; `arrays` gives the three arrays nmfx_upload_csr takes (include/nmfx.h).  The
caller's matrix is never modified."""
import numpy as np
import scipy.sparse as sp

MAX_K = 256          # components on sparse input (kernels_sparse.hip keeps k padded to at most 256)


def is_sparse(x):
    return sp.issparse(x)


def reject(x, method):
    """The solvers other than MUR raise before any device work on sparse input."""
    if is_sparse(x):
        raise TypeError(f"sparse input: method='mur' only (got method='{method}'); pass x.toarray() to run {method}")


def normalise(x, k):
    """Canonical CSR copy of `x` with float32 (if `x` is float32) or float64 values.  Raises ValueError for k outside
    [1, 256] and for negative stored entries."""
    if x.ndim != 2:
        raise ValueError('sparse input must be 2-D')
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f'sparse input supports 1 <= k <= {MAX_K} components (got k = {k})')
    if x.shape[0] >= 2 ** 31 or x.shape[1] >= 2 ** 31:
        raise ValueError('sparse input: each dimension must be below 2^31')
    if np.issubdtype(x.dtype, np.complexfloating):
        raise TypeError('sparse input must be real')
    c = sp.csr_matrix(x, dtype=np.float32 if x.dtype == np.float32 else np.float64, copy=True)
    c.sum_duplicates()
    c.eliminate_zeros()
    c.sort_indices()
    if c.nnz and np.min(c.data) < 0:
        raise ValueError('sparse input has negative entries.  The reference lifts negative data by its minimum '
                         '(nmf/mur.py:99-101), which makes the matrix dense: pass x.toarray() for that behaviour')
    return c


def arrays(c):
    """(row_ptr int64, col_idx int32, values f32 / f64), contiguous, of a matrix from `normalise`."""
    return (np.ascontiguousarray(c.indptr, dtype=np.int64), np.ascontiguousarray(c.indices, dtype=np.int32),
            np.ascontiguousarray(c.data))


def objective(c, w, h, kind='eu', chunk=1 << 20):
    """nmf/utils.py:18-33 of (x, w h) in float64 on the host, from the non-zeros of `c` (CSR) plus k x k / k-sized terms
    -- the decomposition the device records ("Sparse V"); w h is formed at the non-zeros only, `chunk` of
    them at a time:
        eu  1/2 [ ||x||^2 - 2 Sum_nz x wh + <w^T w, h h^T> ]
        kl  Sum_nz [x log(x / wh) - x] + Sum_c colsum(w)_c rowsum(h)_c       (inf / nan log terms -> 0)"""
    w = np.asarray(w, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    rows = np.repeat(np.arange(c.shape[0]), np.diff(c.indptr))
    cols, x = c.indices, c.data.astype(np.float64)
    s = 0.0
    for a in range(0, c.nnz, chunk):
        b = min(c.nnz, a + chunk)
        wh = np.einsum('ij,ji->i', w[rows[a:b]], h[:, cols[a:b]])
        xa = x[a:b]
        if kind == 'eu':
            s += float(np.dot(xa, wh))
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                t = xa * np.log(xa / wh)
            t = np.where(t == np.inf, 0, t)
            t = np.where(np.isnan(t), 0, t)
            s += float(np.sum(t - xa))
    if kind == 'eu':
        return 0.5 * (float(np.dot(x, x)) - 2.0 * s + float(np.sum((w.T @ w) * (h @ h.T))))
    if kind == 'kl':
        return s + float(np.dot(w.sum(axis=0), h.sum(axis=1)))
    raise KeyError('Distance type unknown: use "kl" or "eu"')
