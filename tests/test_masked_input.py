"""Masked input on the host: the float64 restatement of masked MUR pinned to the oracle, the observed-set builder, the
masked objective, validation and the entry points that refuse a mask.  None of this needs a GPU."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import fix_kwargs, load_golden
from masked_ref import masked_h_step, masked_mur, masked_objective, masked_w_step
from oracle import nmf_ref as R

GOLDENS = ["mur_eu_lambda", "mur_eu_ragged", "mur_kl", "mur_kl_lambda"]     # (mur_eu_signed: masked input refuses negatives)


@pytest.mark.parametrize("name", GOLDENS)
def test_all_ones_mask_is_the_reference(name):
    z, meta = load_golden(name)
    v = R.fixture_matrix(meta["vspec"])
    kw = fix_kwargs(meta["kwargs"])
    np.random.seed(meta["seed"])
    want = R.mur(v.copy(), meta["k"], **kw)
    np.random.seed(meta["seed"])
    got = masked_mur(v, np.ones(v.shape, dtype=bool), meta["k"], **kw)
    assert got.i == want.i == int(z["i"])
    np.testing.assert_allclose(got.w, want.w, rtol=1e-12)
    np.testing.assert_allclose(got.h, want.h, rtol=1e-12)
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=1e-12)


@pytest.mark.parametrize("name", GOLDENS)
def test_all_ones_half_steps_are_the_reference_steps(name):
    z, meta = load_golden(name)
    v = R.fixture_matrix(meta["vspec"])
    kind = meta["kwargs"]["distance_type"]
    lw, lh = meta["kwargs"].get("lambda_w", 0.0), meta["kwargs"].get("lambda_h", 0.0)
    ones = np.ones(v.shape, dtype=bool)
    w0, h0 = z["w0"], z["h0"]
    w1 = R.mur_w_step(kind, v, w0, h0, w0 @ h0, lw)
    np.testing.assert_allclose(masked_w_step(kind, v, ones, w0, h0, lw), w1, rtol=1e-12)
    np.testing.assert_allclose(masked_h_step(kind, v, ones, w1, h0, lh), R.mur_h_step(kind, v, w1, h0, w1 @ h0, lh), rtol=1e-12)
    for k2 in ("eu", "kl"):
        assert masked_objective(k2, v, ones, w1 @ h0) == pytest.approx(R.objective(v, w1 @ h0, k2), rel=1e-12)


def planted(m, n, k, seed):
    rng = np.random.RandomState(seed)
    return (rng.rand(m, k) @ rng.rand(k, n)) / k + 0.01 * rng.rand(m, n)


@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_host_objective(kind):
    from nmf_amd import masked
    rng = np.random.RandomState(3)
    x = planted(40, 30, 4, 1)
    w, h = np.abs(rng.randn(40, 4)), np.abs(rng.randn(4, 30))
    w[5] = 0                                                  # wh = 0 on a row: inf / nan log terms -> 0
    ones = np.ones(x.shape, dtype=bool)
    assert masked.objective(x, w, h, ones, kind, chunk=37) == pytest.approx(R.objective(x, w @ h, kind), rel=1e-12)
    m = rng.rand(*x.shape) < 0.3
    m[7] = False
    x[3, 4], m[3, 4] = 0.0, True                             # an observed zero
    xn = np.where(m, x, np.nan)
    wh = w @ h
    if kind == "eu":
        direct = 0.5 * sum((x[i, j] - wh[i, j]) ** 2 for i, j in zip(*np.nonzero(m)))
    else:
        direct = 0.0
        for i, j in zip(*np.nonzero(m)):
            with np.errstate(all="ignore"):
                t = x[i, j] * np.log(x[i, j] / wh[i, j])
            direct += (0.0 if (t == np.inf or np.isnan(t)) else t) - x[i, j] + wh[i, j]
    assert masked.objective(xn, w, h, m, kind, chunk=11) == pytest.approx(direct, rel=1e-12)
    assert masked_objective(kind, xn, m, wh) == pytest.approx(direct, rel=1e-12)


def test_observed_keeps_observed_zeros_and_ignores_unobserved_values():
    from nmf_amd import masked
    x = np.array([[1.0, np.nan, 0.0], [-5.0, 2.0, np.inf], [3.0, 0.0, 4.0]])
    m = np.array([[1, 0, 1], [0, 1, 0], [1, 1, 0]], dtype=np.int8)
    xb, mb = x.copy(), m.copy()
    c = masked.observed(x, m)
    assert c.format == "csr" and c.nnz == 5 and c.data.dtype == np.float64
    np.testing.assert_array_equal(c.indptr, [0, 2, 3, 5])
    np.testing.assert_array_equal(c.indices, [0, 2, 1, 0, 1])
    np.testing.assert_array_equal(c.data, [1.0, 0.0, 2.0, 3.0, 0.0])          # two observed zeros, kept
    np.testing.assert_array_equal(x, xb)
    np.testing.assert_array_equal(m, mb)
    c32 = masked.observed(x.astype(np.float32), m.astype(bool))
    assert c32.data.dtype == np.float32 and c32.nnz == 5


def test_observed_from_sparse_data_and_sparse_mask():
    from nmf_amd import masked
    rng = np.random.RandomState(0)
    x = sp.random(50, 40, density=0.2, format="coo", random_state=rng)
    x = sp.coo_matrix((np.concatenate([x.data, [0.5]]), (np.concatenate([x.row, [x.row[0]]]), np.concatenate([x.col, [x.col[0]]]))),
                      shape=x.shape)                                           # a duplicate: x's value there is the sum
    mask = sp.random(50, 40, density=0.3, format="csc", random_state=rng)
    mask.data[:] = 1
    xb = (x.row.copy(), x.col.copy(), x.data.copy())
    mb = mask.copy()
    c = masked.observed(x, mask)
    dense, md = x.toarray(), mask.toarray() != 0
    assert c.nnz == int(md.sum())
    np.testing.assert_array_equal(c.toarray(), np.where(md, dense, 0))
    np.testing.assert_array_equal(sp.csr_matrix((np.ones(c.nnz), c.indices, c.indptr), shape=c.shape).toarray() != 0, md)
    unstored = md & (dense == 0)
    assert unstored.sum() > 0                                                  # observed but not stored: value 0, still an entry
    for a, b in zip(xb, (x.row, x.col, x.data)):
        np.testing.assert_array_equal(a, b)
    assert (mask != mb).nnz == 0
    # the same from dense data with the same mask (dense mask too)
    c2 = masked.observed(dense, md)
    np.testing.assert_array_equal(c2.indptr, c.indptr)
    np.testing.assert_array_equal(c2.indices, c.indices)
    np.testing.assert_array_equal(c2.data, c.data)


def test_observed_row_blocks_match_a_direct_build(monkeypatch):
    from nmf_amd import masked
    monkeypatch.setattr(masked, "ROWS", 7)
    rng = np.random.RandomState(5)
    x = rng.rand(60, 33)
    m = rng.rand(60, 33) < 0.4
    m[10:20] = False                                                           # empty rows across a block boundary
    c = masked.observed(x, m)
    r, q = np.nonzero(m)
    np.testing.assert_array_equal(c.indices, q)
    np.testing.assert_array_equal(c.data, x[r, q])
    np.testing.assert_array_equal(np.diff(c.indptr), m.sum(axis=1))
    cs = masked.observed(sp.csr_matrix(x), sp.csr_matrix(m))
    np.testing.assert_array_equal(cs.data, x[r, q])


def _mur(*a, **kw):
    from nmf_amd.mur import mur
    return mur(*a, **kw)


@pytest.mark.parametrize("case", ["shape", "negative", "nan", "inf", "empty", "k0", "k257", "engine", "complex", "sparse_negative"])
def test_validation_before_device_work(case):
    x = np.random.RandomState(0).rand(20, 10)
    m = np.ones((20, 10), dtype=bool)
    kw = {}
    k = 3
    err = ValueError
    if case == "shape":
        m = np.ones((10, 20), dtype=bool)
    elif case == "negative":
        x[2, 3] = -1.0
    elif case == "nan":
        x[2, 3] = np.nan
    elif case == "inf":
        x[2, 3] = np.inf
    elif case == "empty":
        m[:] = False
    elif case == "k0":
        k = 0
    elif case == "k257":
        k = 257
    elif case == "engine":
        kw["engine"] = object()
    elif case == "complex":
        x = x.astype(np.complex128)
        err = TypeError
    elif case == "sparse_negative":
        x = sp.csr_matrix(np.where(x > 0.5, x, 0.0))
        x.data[0] = -2.0
    with pytest.raises(err):
        _mur(x, k, mask=m, **kw)


def test_unobserved_bad_values_pass_validation():
    from nmf_amd import masked
    x = np.random.RandomState(0).rand(20, 10)
    m = np.ones((20, 10), dtype=bool)
    x[2, 3], x[4, 5], x[6, 7] = -1.0, np.nan, np.inf
    m[2, 3] = m[4, 5] = m[6, 7] = False
    c = masked.observed(x, m, 3)
    assert c.nnz == 197 and np.isfinite(c.data).all() and (c.data >= 0).all()


def test_factorize_grid_refuses_a_mask():
    from nmf_amd.grid import factorize_grid
    x = np.random.RandomState(0).rand(20, 10)
    with pytest.raises(TypeError, match="mask"):
        factorize_grid(x, "mur", features=(2,), mask=np.ones(x.shape, dtype=bool))


@pytest.mark.parametrize("method", ["anls", "admm", "ao_admm"])
def test_other_methods_refuse_a_mask(method):
    from importlib import import_module

    from nmf_amd import NMF
    x = np.random.RandomState(0).rand(20, 10)
    m = np.ones(x.shape, dtype=bool)
    with pytest.raises(TypeError, match="mask"):
        getattr(import_module("nmf_amd." + method), method)(x, 3, mask=m)
    with pytest.raises(TypeError, match="mask"):
        NMF(x, 3).factorize(method=method, mask=m)


def test_dist_factorize_refuses_a_mask(tmp_path, monkeypatch):
    import torch.distributed as tdist

    from nmf_amd import dist as nd
    for var in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("NMFX_DIST_INIT_METHOD", "file://" + str(tmp_path / "store"))
    x = np.random.RandomState(0).rand(12, 9)
    try:
        with pytest.raises(TypeError, match="mask"):
            nd.factorize(x, 3, method="mur", backend="gloo", mask=np.ones(x.shape, dtype=bool))
    finally:
        if tdist.is_initialized():
            tdist.destroy_process_group()


def test_set_masked_needs_a_handle():
    from nmf_amd import _lib as L
    lib = L.load()
    assert lib.nmfx_version() >= 320
    assert lib.nmfx_set_masked(C.c_void_p(), 1) == L.NMFX_E_ARG
