"""The input rules of nmf_amd.hals.hals_sparse: every refusal is raised before any device work (these tests run without a
GPU: a call that got as far as the device would raise `no HIP device`) and before any draw from the global generator, with its
type and the start of its message, and leaves the caller's matrix as it was."""
import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd.hals import hals, hals_sparse
from nmf_amd.nmf import NMF


def data(fmt="csr_matrix"):
    return getattr(sp, fmt)(sp.random(12, 9, density=0.4, random_state=np.random.RandomState(3), data_rvs=lambda s: np.random.RandomState(4).uniform(0.1, 1.0, s)))


REFUSALS = [
    (dict(k=0), ValueError, "hals_sparse: supports 1 <= k <= 128 components"),
    (dict(k=-3), ValueError, "hals_sparse: supports 1 <= k <= 128 components"),
    (dict(k=129), ValueError, "hals_sparse: supports 1 <= k <= 128 components"),
    (dict(k=2.5), ValueError, "hals_sparse: supports 1 <= k <= 128 components"),
    (dict(k=True), ValueError, "hals_sparse: supports 1 <= k <= 128 components"),
    (dict(sweeps=0), ValueError, "hals_sparse: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=17), ValueError, "hals_sparse: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=1.5), ValueError, "hals_sparse: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=True), ValueError, "hals_sparse: sweeps must be an integer between 1 and 16"),
    (dict(lambda_w=-0.1), ValueError, "hals_sparse: lambda_w must be non-negative"),
    (dict(lambda_h=-1e-9), ValueError, "hals_sparse: lambda_h must be non-negative"),
    (dict(lambda_h=float("nan")), ValueError, "hals_sparse: lambda_h must be non-negative"),
    (dict(distance_type="eu"), TypeError, "hals_sparse() got an unexpected keyword argument 'distance_type'"),
    (dict(distance_type="kl"), TypeError, "hals_sparse() got an unexpected keyword argument 'distance_type'"),
    (dict(mask=np.ones((12, 9), bool)), TypeError, "hals_sparse() got an unexpected keyword argument 'mask'"),
    (dict(engine=None), TypeError, "hals_sparse() got an unexpected keyword argument 'engine'"),
]


def seeded_draw_after(call):
    """`call` must raise and draw nothing: returns (exception, whether the next seeded draw is the one a fresh seed gives)."""
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(Exception) as e:
        call()
    return e.value, np.array_equal(np.random.rand(4), want)


@pytest.mark.parametrize("kw,exc,start", REFUSALS, ids=[f"{i}-{next(iter(r[0]))}" for i, r in enumerate(REFUSALS)])
def test_refusals(kw, exc, start):
    x = data()
    keep = x.copy()
    args = dict(k=3, nndsvd_init=(False, "zero"))
    args.update(kw)
    err, untouched = seeded_draw_after(lambda: hals_sparse(x, **args))
    assert type(err) is exc and str(err).startswith(start), repr(err)
    assert "no HIP device" not in str(err)
    assert untouched
    assert (x != keep).nnz == 0 and np.array_equal(x.data, keep.data)


@pytest.mark.parametrize("x", [np.ones((12, 9)), np.ones((12, 9), np.float32), [[1.0, 2.0], [3.0, 4.0]]], ids=["f64", "f32", "list"])
def test_dense_input_is_refused(x):
    err, untouched = seeded_draw_after(lambda: hals_sparse(x, 3, nndsvd_init=(False, "zero")))
    assert type(err) is TypeError and str(err) == "hals_sparse: x must be a scipy.sparse matrix; use hals"
    assert untouched


@pytest.mark.parametrize("fmt", ["csr_matrix", "csc_matrix", "coo_matrix", "csr_array"])
def test_negative_stored_entries_are_refused_with_normalises_message(fmt):
    x = data(fmt)
    x.data[2] = -0.5
    keep = x.copy()
    err, untouched = seeded_draw_after(lambda: hals_sparse(x, 3, nndsvd_init=(False, "zero")))
    assert type(err) is ValueError and str(err).startswith("hals_sparse: sparse input has negative entries"), repr(err)
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
    with pytest.raises(RuntimeError, match="reached the engine"):
        hals_sparse(x, 3, nndsvd_init=(False, "zero"))
    assert sp.isspmatrix_csr(seen["x"]) and seen["k"] == 3 and seen["masked"] is False
    assert (seen["x"] != sp.csr_matrix(x)).nnz == 0


def test_nmf_factorize_routes_sparse_data_to_hals_sparse():
    err, untouched = seeded_draw_after(lambda: NMF(data(), 3).factorize("hals", sweeps=0))
    assert type(err) is ValueError and str(err).startswith("hals_sparse: sweeps must be"), repr(err)
    assert untouched
    with pytest.raises(ValueError, match="^hals: sweeps"):               # dense data stays with hals
        NMF(data().toarray(), 3).factorize("hals", sweeps=0)


def test_hals_itself_still_refuses_sparse_input():
    with pytest.raises(TypeError) as e:
        hals(data(), 3)
    assert "hals" in str(e.value) and "no HIP device" not in str(e.value)


def test_abi_table_and_library():
    sig = L.SIGNATURES["nmfx_hals_sparse_run"]
    assert sig == L.SIGNATURES["nmfx_hals_run"]                           # (h, lambda_w, lambda_h, sweeps, min_iter, tol1, tol2, first, count)
    assert L.SIGNATURES["nmfx_hals_sparse_finish"] == L.SIGNATURES["nmfx_aoadmm_finish"]
    lib = L.load()
    assert lib.nmfx_version() >= 391 and hasattr(lib, "nmfx_hals_sparse_run") and hasattr(lib, "nmfx_hals_sparse_finish")
