"""Masked input for MUR: factorize only the observed entries of V (`mur(x, k, mask=...)`).

`observed` turns the caller's data and mask into the canonical CSR of the observed entries -- sorted, one entry per
observed position, stored zeros KEPT (an observed zero is data) -- which a masked engine (nmfx_set_masked) takes as its
observed set; `objective` scores factors on any observed set on the host, e.g. held-out entries.  Values at unobserved
positions are never read, and neither `x` nor `mask` is modified."""
import numpy as np
import scipy.sparse as sp

from . import losses
from .sparse import MAX_K

ROWS = 1024          # rows of a dense mask handled at a time (no m x n temporaries)


def check_k(k):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f'masked input supports 1 <= k <= {MAX_K} components (got k = {k})')


def value_dtype(x):
    if np.issubdtype(x.dtype, np.complexfloating):
        raise TypeError('masked input must be real')
    return np.float32 if x.dtype == np.float32 else np.float64


def _positions(mask, shape):
    """(row_ptr int64 [m + 1], col_idx int32) of the non-zero mask entries, row by row, columns ascending."""
    m = shape[0]
    if sp.issparse(mask):
        p = sp.csr_matrix(mask, copy=True)
        p.sum_duplicates()                   # (a position's mask value is the sum of its duplicates, as scipy reads it)
        p.eliminate_zeros()
        p.sort_indices()
        return p.indptr.astype(np.int64), p.indices.astype(np.int32)
    counts, cols = [np.zeros(1, dtype=np.int64)], []
    for a in range(0, m, ROWS):
        r, c = np.nonzero(mask[a:a + ROWS])
        counts.append(np.bincount(r, minlength=min(m, a + ROWS) - a).astype(np.int64))
        cols.append(c.astype(np.int32))
    return np.cumsum(np.concatenate(counts)), np.concatenate(cols) if cols else np.zeros(0, np.int32)


def _values(x, row_ptr, col_idx, dtype):
    """x at the observed positions: dense `x` a block of rows at a time; sparse `x` by a sorted search of its
    (row, column) keys, 0 where a position is not stored."""
    m = x.shape[0]
    out = np.empty(col_idx.size, dtype=dtype)
    if sp.issparse(x):
        c = sp.csr_matrix(x, copy=True)
        c.sum_duplicates()
        c.sort_indices()
        n = np.int64(x.shape[1])
        xkeys = np.repeat(np.arange(m, dtype=np.int64), np.diff(c.indptr)) * n + c.indices.astype(np.int64)
        for a in range(0, m, ROWS):
            b = min(m, a + ROWS)
            e0, e1 = row_ptr[a], row_ptr[b]
            keys = np.repeat(np.arange(a, b, dtype=np.int64), np.diff(row_ptr[a:b + 1])) * n + col_idx[e0:e1]
            pos = np.searchsorted(xkeys, keys)
            hit = pos < xkeys.size
            hit[hit] = xkeys[pos[hit]] == keys[hit]
            vals = np.zeros(keys.size, dtype=dtype)
            vals[hit] = c.data[pos[hit]]
            out[e0:e1] = vals
        return out
    for a in range(0, m, ROWS):
        b = min(m, a + ROWS)
        e0, e1 = row_ptr[a], row_ptr[b]
        rows = np.repeat(np.arange(0, b - a), np.diff(row_ptr[a:b + 1]))
        out[e0:e1] = x[a:b][rows, col_idx[e0:e1]]
    return out


def check_values(vals):
    """The observed values (a non-empty 1-D array) must be finite and non-negative."""
    if not np.all(np.isfinite(vals)):
        raise ValueError('masked input: an observed value is NaN or infinite')
    if np.min(vals) < 0:
        raise ValueError('masked input: an observed value is negative (MUR needs non-negative data; '
                         'masked input is not lifted by its minimum)')


def observed(x, mask, k=None):
    """Canonical CSR (float32 values if `x` is float32, else float64) of `x` at the positions where `mask` is non-zero.
    `x`: a 2-D numpy array or any scipy.sparse matrix (an observed position it does not store is 0); `mask`: a boolean
    or 0 / 1 array, or a scipy.sparse matrix, of the same shape.  Raises ValueError for a shape mismatch, an observed
    value that is negative or not finite, an empty mask, or k outside [1, 256]; TypeError for complex data."""
    if k is not None:
        check_k(k)
    if not sp.issparse(x):
        x = np.asarray(x)
    if not sp.issparse(mask):
        mask = np.asarray(mask)
    if x.ndim != 2:
        raise ValueError('masked input must be 2-D')
    if tuple(mask.shape) != tuple(x.shape):
        raise ValueError(f'mask has shape {tuple(mask.shape)}, data has shape {tuple(x.shape)}')
    if x.shape[0] >= 2 ** 31 or x.shape[1] >= 2 ** 31:
        raise ValueError('masked input: each dimension must be below 2^31')
    dtype = value_dtype(x)
    if np.issubdtype(mask.dtype, np.complexfloating):
        raise TypeError('mask must be real')
    row_ptr, col_idx = _positions(mask, x.shape)
    if col_idx.size == 0:
        raise ValueError('mask observes no entry')
    vals = _values(x, row_ptr, col_idx, dtype)
    check_values(vals)
    c = sp.csr_matrix((vals, col_idx, row_ptr), shape=x.shape)
    c.has_sorted_indices = True
    return c


def check_positive(c):
    """The Itakura-Saito divergence is undefined at 0: every observed value of the canonical CSR `c` must be > 0."""
    check_positive_values(c.data)


def check_positive_values(vals):
    """check_positive on the observed values themselves (a 1-D array)."""
    if vals.size:
        losses.check_f32_image(vals, 'is', context='observed')


def objective(x, w, h, mask, distance_type='eu', chunk=1 << 20):
    """nmf/utils.py:18-33 restricted to the observed entries, in float64 on the host, `chunk` entries at a time:
        eu  1/2 Sum_M (x - wh)^2
        kl  Sum_M [x log(x / wh) - x + wh]       (inf / nan log terms -> 0)
        is  Sum_M [x / q - log(x / q) - 1],  q = wh + 1e-9       (every observed x must be > 0)
    With the training mask it is the objective `mur(x, k, mask=...)` records; with a held-out mask it scores the fit
    there."""
    losses.check_loss(distance_type, ('eu', 'kl', 'is'))
    c = observed(x, mask)
    if distance_type == 'is':
        check_positive(c)
    w = np.asarray(w, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    rows = np.repeat(np.arange(c.shape[0]), np.diff(c.indptr))
    cols, xv = c.indices, c.data.astype(np.float64)
    s = 0.0
    for a in range(0, c.nnz, chunk):
        b = min(c.nnz, a + chunk)
        wh = np.einsum('ij,ji->i', w[rows[a:b]], h[:, cols[a:b]])
        s += float(np.sum(losses.cells(distance_type, xv[a:b], wh)))
    return s
