"""The input rules of nmf_amd.hals.hals_sparse_wide: every refusal is raised before any device work (these tests run without a
GPU: a call that got as far as the device would raise `no HIP device`) and before any draw from the global generator, with its
type and its message, and leaves the caller's matrix as it was.  hals_sparse, hals_wide and NMF.factorize keep their own
refusals: the new function is called by name."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd.hals import hals_sparse, hals_sparse_wide, hals_wide
from nmf_amd.nmf import NMF
from test_hals_sparse_input import data, seeded_draw_after

K_TEXT = "hals_sparse_wide: supports 129 <= k <= 256 components"
REFUSALS = [
    (dict(k=0), ValueError, K_TEXT),
    (dict(k=-3), ValueError, K_TEXT),
    (dict(k=128), ValueError, K_TEXT),
    (dict(k=257), ValueError, K_TEXT),
    (dict(k=1024), ValueError, K_TEXT),
    (dict(k=200.0), ValueError, K_TEXT),
    (dict(k=True), ValueError, K_TEXT),
    (dict(sweeps=0), ValueError, "hals_sparse_wide: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=17), ValueError, "hals_sparse_wide: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=1.5), ValueError, "hals_sparse_wide: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=True), ValueError, "hals_sparse_wide: sweeps must be an integer between 1 and 16"),
    (dict(lambda_w=-0.1), ValueError, "hals_sparse_wide: lambda_w must be non-negative"),
    (dict(lambda_w=True), ValueError, "hals_sparse_wide: lambda_w must be non-negative"),
    (dict(lambda_h=-1e-9), ValueError, "hals_sparse_wide: lambda_h must be non-negative"),
    (dict(lambda_h=float("nan")), ValueError, "hals_sparse_wide: lambda_h must be non-negative"),
    (dict(lambda_h="0"), ValueError, "hals_sparse_wide: lambda_h must be non-negative"),
    (dict(distance_type="eu"), TypeError, "hals_sparse_wide() got an unexpected keyword argument 'distance_type'"),
    (dict(mask=np.ones((12, 9), bool)), TypeError, "hals_sparse_wide() got an unexpected keyword argument 'mask'"),
    (dict(engine=None), TypeError, "hals_sparse_wide() got an unexpected keyword argument 'engine'"),
]


@pytest.mark.parametrize("kw,exc,start", REFUSALS, ids=[f"{i}-{next(iter(r[0]))}" for i, r in enumerate(REFUSALS)])
def test_refusals(kw, exc, start):
    x = data()
    keep = x.copy()
    args = dict(k=200, nndsvd_init=(False, "zero"))
    args.update(kw)
    err, untouched = seeded_draw_after(lambda: hals_sparse_wide(x, **args))
    assert type(err) is exc and str(err).startswith(start), repr(err)
    assert "no HIP device" not in str(err)
    assert untouched
    assert (x != keep).nnz == 0 and np.array_equal(x.data, keep.data)


@pytest.mark.parametrize("k", [1, 64, 128])
def test_a_small_k_is_pointed_to_hals_sparse(k):
    err, untouched = seeded_draw_after(lambda: hals_sparse_wide(data(), k, nndsvd_init=(False, "zero")))
    assert type(err) is ValueError and str(err) == f"{K_TEXT} (got k = {k}); hals_sparse runs 1 <= k <= 128", repr(err)
    assert untouched


@pytest.mark.parametrize("k", [0, 257, 2.5])
def test_no_pointer_where_hals_sparse_would_refuse_too(k):
    err, _ = seeded_draw_after(lambda: hals_sparse_wide(data(), k, nndsvd_init=(False, "zero")))
    assert type(err) is ValueError and str(err) == f"{K_TEXT} (got k = {k!r})", repr(err)


@pytest.mark.parametrize("x", [np.ones((12, 9)), np.ones((12, 9), np.float32), [[1.0, 2.0], [3.0, 4.0]]], ids=["f64", "f32", "list"])
def test_dense_input_is_refused_and_pointed_to_hals_wide(x):
    err, untouched = seeded_draw_after(lambda: hals_sparse_wide(x, 200, nndsvd_init=(False, "zero")))
    assert type(err) is TypeError
    assert str(err) == "hals_sparse_wide: x must be a scipy.sparse matrix; hals_wide runs dense data with 129 <= k <= 1024"
    assert untouched


@pytest.mark.parametrize("fmt", ["csr_matrix", "csc_matrix", "coo_matrix", "csr_array"])
def test_negative_stored_entries_are_refused_with_normalises_message(fmt):
    x = data(fmt)
    x.data[2] = -0.5
    keep = x.copy()
    err, untouched = seeded_draw_after(lambda: hals_sparse_wide(x, 200, nndsvd_init=(False, "zero")))
    assert type(err) is ValueError and str(err).startswith("hals_sparse_wide: sparse input has negative entries"), repr(err)
    assert "no HIP device" not in str(err) and untouched
    assert np.array_equal(x.data, keep.data)


def test_a_valid_call_gets_as_far_as_the_engine(monkeypatch):
    """Every check passed: the next thing is the engine on the canonical CSR copy (stood in for here: no device is touched)."""
    from nmf_amd.engine import Engine
    seen = {}

    def for_sparse(xs, k, device=0, masked=False):
        seen.update(x=xs, k=k, masked=masked)
        raise RuntimeError("reached the engine")

    monkeypatch.setattr(Engine, "for_sparse", staticmethod(for_sparse))
    x = data("coo_matrix")
    for k in (129, 256):
        with pytest.raises(RuntimeError, match="reached the engine"):
            hals_sparse_wide(x, k, nndsvd_init=(False, "zero"))
        assert sp.isspmatrix_csr(seen["x"]) and seen["k"] == k and seen["masked"] is False
        assert (seen["x"] != sp.csr_matrix(x)).nnz == 0


def test_signature_is_that_of_hals_sparse():
    assert inspect.signature(hals_sparse_wide) == inspect.signature(hals_sparse)


def test_the_other_front_ends_keep_their_refusals():
    x = data()
    err, untouched = seeded_draw_after(lambda: hals_sparse(x, 200))
    assert type(err) is ValueError and str(err).startswith("hals_sparse: supports 1 <= k <= 128 components") and untouched
    err, untouched = seeded_draw_after(lambda: hals_wide(x, 200))
    assert type(err) is TypeError and str(err).startswith("hals_wide: takes dense data only; hals_sparse runs scipy.sparse input") and untouched
    err, untouched = seeded_draw_after(lambda: NMF(x, 200).factorize("hals"))
    assert type(err) is ValueError and str(err).startswith("hals_sparse: supports 1 <= k <= 128 components") and untouched


def test_abi_table_and_library():
    assert L.SIGNATURES["nmfx_hals_sparse_wide_run"] == L.SIGNATURES["nmfx_hals_sparse_run"]
    assert L.SIGNATURES["nmfx_hals_sparse_wide_finish"] == L.SIGNATURES["nmfx_hals_sparse_finish"]
    lib = L.load()
    assert lib.nmfx_version() >= 397 and hasattr(lib, "nmfx_hals_sparse_wide_run") and hasattr(lib, "nmfx_hals_sparse_wide_finish")
    from nmf_amd.engine import Engine
    assert callable(Engine.hals_sparse_wide_run) and callable(Engine.hals_sparse_wide_finish)
