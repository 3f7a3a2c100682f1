"""The input rules of nmf_amd.hals.hals_masked: every refusal is raised before any device work (these tests run without a GPU:
a call that got as far as the device would raise `no HIP device`) and before any draw from the global generator, with its type
and message, and leaves the caller's data and mask as they were; a valid call hands the engine the canonical CSR of the
observed entries with masked=True."""
import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd import hals as H
from nmf_amd import masked
from nmf_amd.hals import hals, hals_masked, hals_sparse
from nmf_amd.nmf import NMF


def data():
    """(x 12 x 9 float64 with NaN outside the mask and an observed zero, mask bool)."""
    rng = np.random.RandomState(3)
    mask = rng.rand(12, 9) < 0.5
    mask[0, 0] = mask[1, 1] = True
    x = np.where(mask, rng.uniform(0.1, 1.0, (12, 9)), np.nan)
    x[1, 1] = 0.0
    return x, mask


def seeded_draw_after(call):
    """`call` must raise and draw nothing: returns (exception, whether the next seeded draw is the one a fresh seed gives)."""
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(Exception) as e:
        call()
    return e.value, np.array_equal(np.random.rand(4), want)


REFUSALS = [
    (dict(k=0), ValueError, "hals_masked: supports 1 <= k <= 64 components (got k = 0)"),
    (dict(k=-3), ValueError, "hals_masked: supports 1 <= k <= 64 components"),
    (dict(k=65), ValueError, "hals_masked: supports 1 <= k <= 64 components (got k = 65)"),
    (dict(k=128), ValueError, "hals_masked: supports 1 <= k <= 64 components"),
    (dict(k=2.5), ValueError, "hals_masked: supports 1 <= k <= 64 components"),
    (dict(k=True), ValueError, "hals_masked: supports 1 <= k <= 64 components"),
    (dict(sweeps=0), ValueError, "hals_masked: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=17), ValueError, "hals_masked: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=1.5), ValueError, "hals_masked: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=True), ValueError, "hals_masked: sweeps must be an integer between 1 and 16"),
    (dict(lambda_w=-0.1), ValueError, "hals_masked: lambda_w must be non-negative"),
    (dict(lambda_w=True), ValueError, "hals_masked: lambda_w must be non-negative"),
    (dict(lambda_h=-1e-9), ValueError, "hals_masked: lambda_h must be non-negative"),
    (dict(lambda_h=float("nan")), ValueError, "hals_masked: lambda_h must be non-negative"),
    (dict(distance_type="eu"), TypeError, "hals_masked() got an unexpected keyword argument 'distance_type'"),
    (dict(engine=None), TypeError, "hals_masked() got an unexpected keyword argument 'engine'"),
    (dict(weights=np.ones((12, 9))), TypeError, "hals_masked() got an unexpected keyword argument 'weights'"),
]


@pytest.mark.parametrize("kw,exc,start", REFUSALS, ids=[f"{i}-{next(iter(r[0]))}" for i, r in enumerate(REFUSALS)])
def test_refusals(kw, exc, start):
    x, mask = data()
    keep = x.copy(), mask.copy()
    args = dict(k=3, nndsvd_init=(False, "zero"))
    args.update(kw)
    k = args.pop("k")
    err, untouched = seeded_draw_after(lambda: hals_masked(x, k, mask, **args))
    assert type(err) is exc and str(err).startswith(start), repr(err)
    assert "no HIP device" not in str(err)
    assert untouched
    assert np.array_equal(x, keep[0], equal_nan=True) and np.array_equal(mask, keep[1])


def _bad_inputs():
    x, mask = data()
    neg = x.copy(); neg[0, 0] = -0.5
    nan = x.copy(); nan[0, 0] = np.nan
    inf = x.copy(); inf[0, 0] = np.inf
    return [
        ("shape", x, mask[:, :8], ValueError, "hals_masked: mask has shape (12, 8), data has shape (12, 9)"),
        ("negative", neg, mask, ValueError, "hals_masked: masked input: an observed value is negative"),
        ("nan", nan, mask, ValueError, "hals_masked: masked input: an observed value is NaN or infinite"),
        ("inf", inf, mask, ValueError, "hals_masked: masked input: an observed value is NaN or infinite"),
        ("empty", x, np.zeros((12, 9), bool), ValueError, "hals_masked: mask observes no entry"),
        ("1-d", x[0], mask[0], ValueError, "hals_masked: masked input must be 2-D"),
        ("complex x", np.where(mask, 1.0, 0.0).astype(complex), mask, TypeError, "hals_masked: masked input must be real"),
        ("complex mask", x, mask.astype(complex), TypeError, "hals_masked: mask must be real"),
    ]


@pytest.mark.parametrize("what,x,mask,exc,start", _bad_inputs(), ids=[b[0] for b in _bad_inputs()])
def test_masked_observed_errors_carry_the_prefix(what, x, mask, exc, start):
    err, untouched = seeded_draw_after(lambda: hals_masked(x, 3, mask, nndsvd_init=(False, "zero")))
    assert type(err) is exc and str(err).startswith(start), repr(err)
    assert "no HIP device" not in str(err) and untouched


def test_the_mask_is_required():
    x, _ = data()
    with pytest.raises(TypeError, match="mask"):
        hals_masked(x, 3)


def for_sparse_stub(seen):
    def for_sparse(xs, k, device=0, masked=False):
        seen.update(x=xs, k=k, masked=masked)
        raise RuntimeError("reached the engine")
    return staticmethod(for_sparse)


@pytest.mark.parametrize("xkind", ["dense", "dense32", "sparse"])
@pytest.mark.parametrize("mkind", ["bool", "01", "sparse"])
def test_a_valid_call_gets_as_far_as_the_engine(monkeypatch, xkind, mkind):
    """Every check passed: the next thing is the engine, masked, on the canonical CSR of the observed entries -- stored zeros
    kept, values never read outside the mask (stood in for here: no device is touched).  x and mask are not modified."""
    from nmf_amd.engine import Engine
    seen = {}
    monkeypatch.setattr(Engine, "for_sparse", for_sparse_stub(seen))
    x, mask = data()
    want = masked.observed(x, mask, 3)
    xx = {"dense": x, "dense32": x.astype(np.float32), "sparse": sp.coo_matrix(np.where(mask, x, 0.0))}[xkind]
    mm = {"bool": mask, "01": mask.astype(np.int8), "sparse": sp.csc_matrix(mask)}[mkind]
    keep_x = xx.copy()
    keep_m = mm.copy()
    with pytest.raises(RuntimeError, match="reached the engine"):
        hals_masked(xx, 3, mm, nndsvd_init=(False, "zero"))
    got = seen["x"]
    assert sp.isspmatrix_csr(got) and seen["k"] == 3 and seen["masked"] is True
    assert got.nnz == mask.sum() and np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(got.data, want.data.astype(got.data.dtype)) and (got.data == 0).sum() == 1           # the observed zero is stored
    assert got.dtype == (np.float32 if xkind == "dense32" else np.float64)
    if xkind == "sparse":
        assert (xx != keep_x).nnz == 0
    else:
        assert np.array_equal(xx, keep_x, equal_nan=True)
    if mkind == "sparse":
        assert (mm != keep_m).nnz == 0
    else:
        assert np.array_equal(mm, keep_m)


def test_nmf_factorize_routes_a_mask_to_hals_masked(monkeypatch):
    from nmf_amd.engine import Engine
    x, mask = data()
    err, untouched = seeded_draw_after(lambda: NMF(x, 3).factorize("hals", mask=mask, sweeps=0))
    assert type(err) is ValueError and str(err).startswith("hals_masked: sweeps must be"), repr(err)
    assert untouched
    err, _ = seeded_draw_after(lambda: NMF(sp.csr_matrix(np.where(mask, x, 0.0)), 65).factorize("hals", mask=mask))
    assert type(err) is ValueError and str(err).startswith("hals_masked: supports 1 <= k <= 64"), repr(err)
    seen = {}
    monkeypatch.setattr(Engine, "for_sparse", for_sparse_stub(seen))
    with pytest.raises(RuntimeError, match="reached the engine"):
        NMF(x, 3).factorize("hals", mask=mask, nndsvd_init=(False, "zero"), lambda_w=0.1)
    assert seen["masked"] is True and seen["x"].nnz == mask.sum()
    with pytest.raises(ValueError, match="^hals: sweeps"):               # without a mask dense data stays with hals
        NMF(np.where(mask, x, 0.0), 3).factorize("hals", sweeps=0)
    with pytest.raises(ValueError, match="^hals_sparse: sweeps"):        # ... and sparse data with hals_sparse
        NMF(sp.csr_matrix(np.where(mask, x, 0.0)), 3).factorize("hals", sweeps=0)


def test_hals_and_hals_sparse_keep_their_signatures():
    x, mask = data()
    with pytest.raises(TypeError, match="unexpected keyword argument 'mask'"):
        hals(np.where(mask, x, 0.0), 3, mask=mask)
    with pytest.raises(TypeError, match="unexpected keyword argument 'mask'"):
        hals_sparse(sp.csr_matrix(np.where(mask, x, 0.0)), 3, mask=mask)
    with pytest.raises(ValueError, match="^hals: supports 1 <= k <= 128 components"):      # (the bound of 64 is hals_masked's alone)
        hals(np.ones((4, 4)), 129)
    assert H.MAX_K == 128 and H.MAX_K_MASKED == 64


def test_abi_table_and_library():
    assert L.SIGNATURES["nmfx_hals_masked_run"] == L.SIGNATURES["nmfx_hals_sparse_run"] == L.SIGNATURES["nmfx_hals_run"]
    assert L.SIGNATURES["nmfx_hals_masked_finish"] == L.SIGNATURES["nmfx_hals_sparse_finish"]
    lib = L.load()
    assert lib.nmfx_version() >= 392 and hasattr(lib, "nmfx_hals_masked_run") and hasattr(lib, "nmfx_hals_masked_finish")
