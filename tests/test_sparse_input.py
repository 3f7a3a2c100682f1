"""Sparse input on the host: normalisation, validation, the solvers that refuse it, the sparse NNDSVD and the objective
decomposition the device records.  None of this needs a GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import nmf_ref as R


def test_coo_duplicates_and_stored_zeros():
    from nmf_amd import sparse
    rows = np.array([0, 0, 2, 1, 3, 3])
    cols = np.array([1, 1, 0, 2, 3, 0])
    vals = np.array([1.0, 2.0, 0.0, 4.0, 0.0, 5.0])
    x = sp.coo_matrix((vals, (rows, cols)), shape=(4, 5))
    before = (x.row.copy(), x.col.copy(), x.data.copy())
    c = sparse.normalise(x, 3)
    assert c.format == "csr" and c.has_canonical_format and c.nnz == 3
    assert (c.data != 0).all()
    np.testing.assert_array_equal(c.toarray(), x.toarray())
    assert c.toarray()[0, 1] == 3.0                       # duplicates summed
    for a, b in zip(before, (x.row, x.col, x.data)):        # the caller's matrix is untouched
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("fmt", ["csc", "csr_array", "coo_array", "lil", "dok", "bsr"])
def test_formats(fmt):
    from nmf_amd import sparse
    x = sp.random(30, 20, density=0.2, format="csr", random_state=0)
    y = {"csr_array": sp.csr_array, "coo_array": sp.coo_array}.get(fmt, lambda a: a.asformat(fmt))(x)
    c = sparse.normalise(y, 4)
    assert isinstance(c, sp.csr_matrix) and c.has_sorted_indices
    np.testing.assert_array_equal(c.toarray(), x.toarray())


def test_unsorted_indices_and_index_dtypes():
    from nmf_amd import sparse
    data = np.array([3.0, 1.0, 2.0], dtype=np.float32)
    indices = np.array([4, 0, 2], dtype=np.int64)
    indptr = np.array([0, 3, 3], dtype=np.int64)
    x = sp.csr_matrix((data, indices, indptr), shape=(2, 5))
    assert not x.has_sorted_indices
    c = sparse.normalise(x, 2)
    row_ptr, col_idx, values = sparse.arrays(c)
    assert row_ptr.dtype == np.int64 and col_idx.dtype == np.int32 and values.dtype == np.float32
    np.testing.assert_array_equal(col_idx, [0, 2, 4])
    np.testing.assert_array_equal(values, [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(row_ptr, [0, 3, 3])
    assert not x.has_sorted_indices                         # (the copy was sorted, not the caller's matrix)
    xi = sp.csr_matrix(np.array([[0, 2], [3, 0]], dtype=np.int32))
    assert sparse.arrays(sparse.normalise(xi, 1))[2].dtype == np.float64


def test_negative_entries_and_k_limits_raise():
    from nmf_amd import sparse
    from nmf_amd.mur import mur
    x = sp.csr_matrix(np.array([[0.0, -1.0], [2.0, 0.0]]))
    with pytest.raises(ValueError, match="toarray"):
        mur(x, 1)
    y = sp.random(40, 300, density=0.1, format="csr", random_state=0)
    with pytest.raises(ValueError, match="256"):
        mur(y, 257)
    with pytest.raises(ValueError, match="256"):
        sparse.normalise(y, 0)


@pytest.mark.parametrize("method", ["anls", "admm", "ao_admm"])
def test_other_methods_refuse_sparse_before_device_work(method):
    from nmf_amd import NMF
    x = sp.random(20, 10, density=0.3, format="csr", random_state=0)
    with pytest.raises(TypeError, match="method='mur' only"):
        NMF(x, 3).factorize(method=method)


def planted_blocks(seed, k=6, block=(40, 30), noise_blocks=3):
    """Block-diagonal sparse matrix whose leading k singular values are distinct and well separated (one dense positive
    block per component, scaled apart), with a few small noise blocks behind them."""
    rng = np.random.RandomState(seed)
    blocks = [(10.0 * (k - i)) * rng.uniform(0.5, 1.0, block) for i in range(k)]
    blocks += [0.1 * rng.uniform(0.0, 1.0, block) for _ in range(noise_blocks)]
    return sp.block_diag(blocks, format="csr")


@pytest.mark.parametrize("variant", ["zero", "mean", "random"])
def test_sparse_nndsvd_lapack_branch_is_the_dense_one(variant):
    from nmf_amd import utils
    x = planted_blocks(0)
    np.random.seed(3)
    w, h = utils.nndsvd_sparse(x, 6, variant)
    np.random.seed(3)
    w0, h0 = utils.nndsvd(x.toarray(), 6, variant)
    np.testing.assert_array_equal(w, w0)
    np.testing.assert_array_equal(h, h0)


def test_sparse_nndsvd_svds_branch():
    # ('zero' only: 'mean' / 'random' fill the EXACT zeros, and LAPACK leaves exact zeros where ARPACK leaves 1e-17)
    from nmf_amd import utils
    x = planted_blocks(1)
    w, h = utils.nndsvd_sparse(x, 6, "zero", dense_below=0)        # (the svds branch below its size threshold)
    w0, h0 = utils.nndsvd(x.toarray(), 6, "zero")
    assert np.linalg.norm(w - w0) <= 1e-8 * np.linalg.norm(w0)
    assert np.linalg.norm(h - h0) <= 1e-8 * np.linalg.norm(h0)


def test_sparse_nndsvd_svds_branch_at_the_size_threshold():
    from nmf_amd import utils
    x = planted_blocks(2, k=5, block=(420, 400), noise_blocks=0)     # 2100 x 2000 >= 2^22 elements
    assert x.shape[0] * x.shape[1] >= 1 << 22
    w, h = utils.nndsvd_sparse(x, 5, "zero")
    w0, h0 = utils.nndsvd(x.toarray(), 5, "zero")
    assert np.linalg.norm(w - w0) <= 1e-8 * np.linalg.norm(w0)
    assert np.linalg.norm(h - h0) <= 1e-8 * np.linalg.norm(h0)


@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_objective_decomposition(kind):
    from nmf_amd import sparse
    rng = np.random.RandomState(7)
    x = sp.random(60, 45, density=0.15, format="lil", random_state=rng)
    x[4, :] = 0
    x[:, 9] = 0
    x[10, 3] = 0.5
    c = sparse.normalise(x.tocsr(), 5)
    w = np.abs(rng.randn(60, 5))
    h = np.abs(rng.randn(5, 45))
    w[7] = 0                                                 # a zero row of w: wh = 0 at its non-zeros (inf log term -> 0)
    got = sparse.objective(c, w, h, kind, chunk=17)
    want = R.objective(c.toarray(), w @ h, kind)
    assert abs(got - want) <= 1e-12 * abs(want)
