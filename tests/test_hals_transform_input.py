"""The input rules of nmf_amd.hals.hals_transform without a GPU: every refusal comes with its class and message before the
library is touched and leaves the global generator and the caller's arrays as they were; NMF.transform routes sparse data and
mask= to it and everything else to transform as before; a valid call reaches the library."""
import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd import hals as H
from nmf_amd.hals import hals_transform
from test_beta_input import no_library  # noqa: F401  (the fixture)


def data():
    """(x 12 x 9 float64 with NaN outside the mask and an observed zero, mask bool, w 12 x 3, h0 3 x 9)."""
    rng = np.random.RandomState(3)
    mask = rng.rand(12, 9) < 0.5
    mask[0, 0] = mask[1, 1] = True
    x = np.where(mask, rng.uniform(0.1, 1.0, (12, 9)), np.nan)
    x[1, 1] = 0.0
    return x, mask, rng.uniform(0.1, 1.0, (12, 3)), rng.uniform(0.1, 1.0, (3, 9))


def sparse_x():
    x, mask, _, _ = data()
    return sp.csr_matrix(np.where(mask, x, 0.0))


def refused(call):
    """`call` must raise, draw nothing and touch no library: (exception)."""
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(Exception) as e:
        call()
    assert np.array_equal(np.random.rand(4), want), "a refusal drew from the global generator"
    assert "library was touched" not in str(e.value) and "no HIP device" not in str(e.value), repr(e.value)
    return e.value


def put(a, value, at=(0, 0)):
    a = np.array(a, dtype=complex if isinstance(value, complex) else np.float64)
    a[at] = value
    return a


REFUSALS = [
    # (which input, keywords, class, start of the message)
    ("both", dict(tol=-1e-9), ValueError, "hals_transform: tol must be a real number with 0 <= tol < 1 (got tol = -1e-09)"),
    ("both", dict(tol=1.0), ValueError, "hals_transform: tol must be a real number with 0 <= tol < 1"),
    ("both", dict(tol=float("nan")), ValueError, "hals_transform: tol must be a real number with 0 <= tol < 1"),
    ("both", dict(tol=float("inf")), ValueError, "hals_transform: tol must be a real number with 0 <= tol < 1"),
    ("both", dict(tol="1e-4"), ValueError, "hals_transform: tol must be a real number with 0 <= tol < 1"),
    ("both", dict(tol=True), ValueError, "hals_transform: tol must be a real number with 0 <= tol < 1"),
    ("both", dict(max_sweeps=0), ValueError, "hals_transform: max_sweeps must be an integer between 1 and 10000 (got max_sweeps = 0)"),
    ("both", dict(max_sweeps=10001), ValueError, "hals_transform: max_sweeps must be an integer between 1 and 10000"),
    ("both", dict(max_sweeps=2.5), ValueError, "hals_transform: max_sweeps must be an integer between 1 and 10000"),
    ("both", dict(max_sweeps=True), ValueError, "hals_transform: max_sweeps must be an integer between 1 and 10000"),
    ("both", dict(lambda_h=-0.1), ValueError, "hals_transform: lambda_h must be non-negative (got lambda_h = -0.1)"),
    ("both", dict(lambda_h=float("nan")), ValueError, "hals_transform: lambda_h must be non-negative"),
    ("both", dict(lambda_h=True), ValueError, "hals_transform: lambda_h must be non-negative"),
    ("both", dict(h0=np.ones((3, 8))), ValueError, "hals_transform: h0 has shape (3, 8), expected (3, 9)"),
    ("both", dict(h0=np.ones(9)), ValueError, "hals_transform: h0 must be 2-D (got 1-D)"),
    ("both", dict(h0=put(np.ones((3, 9)), -0.5)), ValueError, "hals_transform: h0 has a negative entry"),
    ("both", dict(h0=put(np.ones((3, 9)), np.nan)), ValueError, "hals_transform: h0 has an entry that is NaN or infinite"),
    ("both", dict(h0=put(np.ones((3, 9)), 1j)), ValueError, "hals_transform: h0 must be a real array"),
    ("both", dict(w=put(np.ones((12, 3)), -0.5)), ValueError, "hals_transform: w has a negative entry"),
    ("both", dict(w=put(np.ones((12, 3)), np.inf)), ValueError, "hals_transform: w has an entry that is NaN or infinite"),
    ("both", dict(w=put(np.ones((12, 3)), 1j)), ValueError, "hals_transform: w must be a real array"),
    ("both", dict(w=np.ones(12)), ValueError, "hals_transform: w must be 2-D (got 1-D)"),
    ("both", dict(w=np.ones((11, 3))), ValueError, "hals_transform: w has 11 rows, x_new has 12"),
    ("both", dict(w=np.ones((12, 0))), ValueError, "hals_transform: supports 1 <= k <= "),
    ("sparse", dict(w=np.ones((12, 129))), ValueError, "hals_transform: supports 1 <= k <= 128 components (w has 129 columns)"),
    ("masked", dict(w=np.ones((12, 65))), ValueError, "hals_transform: supports 1 <= k <= 64 components with a mask (w has 65 columns)"),
    ("both", dict(sweeps=2), TypeError, "hals_transform() got an unexpected keyword argument 'sweeps'"),
    ("both", dict(distance_type="eu"), TypeError, "hals_transform() got an unexpected keyword argument 'distance_type'"),
]


def _call(kind, kw):
    x, mask, w, h0 = data()
    args = dict(w=w, h0=h0)
    args.update(kw)
    w = args.pop("w")
    if kind == "sparse":
        xs = sparse_x()
        keep = xs.copy()
        err = refused(lambda: hals_transform(xs, w, **args))
        assert (xs != keep).nnz == 0
    else:
        keep = x.copy(), mask.copy()
        err = refused(lambda: hals_transform(x, w, mask, **args))
        assert np.array_equal(x, keep[0], equal_nan=True) and np.array_equal(mask, keep[1])
    return err


@pytest.mark.parametrize("which,kw,exc,start", REFUSALS, ids=[f"{i}-{next(iter(r[1]))}" for i, r in enumerate(REFUSALS)])
def test_refusals(which, kw, exc, start, no_library):  # noqa: F811
    for kind in (("sparse", "masked") if which == "both" else (which,)):
        err = _call(kind, kw)
        assert type(err) is exc and str(err).startswith(start), (kind, repr(err))


def test_dense_data_without_a_mask_points_to_transform(no_library):  # noqa: F811
    x, mask, w, h0 = data()
    err = refused(lambda: hals_transform(np.where(mask, x, 0.0), w))
    assert type(err) is TypeError and str(err).startswith("hals_transform: dense x_new needs mask=")
    assert "transform(x_new, w, distance_type='eu')" in str(err)


def _bad_data():
    x, mask, w, _ = data()
    return [
        ("masked shape", x, mask[:, :8], ValueError, "hals_transform: mask has shape (12, 8), data has shape (12, 9)"),
        ("masked negative", put(x, -0.5), mask, ValueError, "hals_transform: masked input: an observed value is negative"),
        ("masked nan", put(x, np.nan), mask, ValueError, "hals_transform: masked input: an observed value is NaN or infinite"),
        ("masked empty", x, np.zeros((12, 9), bool), ValueError, "hals_transform: mask observes no entry"),
        ("masked 1-d", x[0], mask[0], ValueError, "hals_transform: masked input must be 2-D"),
        ("masked complex", np.where(mask, 1.0, 0.0).astype(complex), mask, TypeError, "hals_transform: masked input must be real"),
        ("masked complex mask", x, mask.astype(complex), TypeError, "hals_transform: mask must be real"),
        ("sparse negative", sp.csr_matrix(put(np.where(mask, x, 0.0), -0.5)), None, ValueError, "hals_transform: sparse input has negative entries"),
        ("sparse complex", sp.csr_matrix(np.where(mask, x, 0.0).astype(complex)), None, TypeError, "hals_transform: sparse input must be real"),
    ]


@pytest.mark.parametrize("what,x,mask,exc,start", _bad_data(), ids=[b[0] for b in _bad_data()])
def test_the_data_rules_carry_the_prefix(what, x, mask, exc, start, no_library):  # noqa: F811
    w = data()[2]
    err = refused(lambda: hals_transform(x, w, mask))
    assert type(err) is exc and str(err).startswith(start), repr(err)


# ---- a valid call reaches the library ----------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def for_sparse_stub(seen):
    def for_sparse(xs, k, device=0, masked=False):
        seen.update(x=xs, k=k, masked=masked, device=device)
        raise _Reached()
    return staticmethod(for_sparse)


@pytest.mark.parametrize("kind", ["sparse", "masked", "masked sparse x"])
def test_the_base_case_reaches_the_library(kind, monkeypatch):
    """Every check passed: the next thing is the engine on the canonical CSR (of the observed entries, masked, with a mask); the
    defaults are scikit-learn's for its cd solver; no draw is made with h0 left out."""
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    seen = {}
    monkeypatch.setattr(Engine, "for_sparse", for_sparse_stub(seen))
    x, mask, w, _ = data()
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(_Reached):
        if kind == "sparse":
            hals_transform(sparse_x().tocoo(), w, device=2)
        elif kind == "masked":
            hals_transform(x, w, mask, device=2)
        else:
            hals_transform(sparse_x().tocsc(), w, sp.coo_matrix(mask), device=2)
    assert np.array_equal(np.random.rand(4), want)
    assert sp.isspmatrix_csr(seen["x"]) and seen["k"] == 3 and seen["device"] == 2 and seen["masked"] is (kind != "sparse")
    if kind == "sparse":
        assert seen["x"].nnz == mask.sum() - 1                       # (the stored zero is no entry of a sparse matrix)
    else:
        obs = masked.observed(x, mask, 3)
        assert seen["x"].nnz == mask.sum() and np.array_equal(seen["x"].indices, obs.indices)        # the observed zero is data
    import inspect
    sig = inspect.signature(hals_transform)
    assert [sig.parameters[n].default for n in ("mask", "h0", "lambda_h", "tol", "max_sweeps", "device")] == [None, None, 0, 1e-4, 200, 0]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("h0", "lambda_h", "tol", "max_sweeps", "device"))


def test_a_valid_call_gets_to_the_library(no_library):  # noqa: F811
    x, mask, w, h0 = data()
    with pytest.raises(AssertionError, match="library was touched"):
        hals_transform(x, w, mask, h0=h0)
    with pytest.raises(AssertionError, match="library was touched"):
        hals_transform(sparse_x(), w, tol=0, max_sweeps=10000, lambda_h=0.5)


# ---- NMF.transform ------------------------------------------------------------------------------------------------------------
def test_nmf_transform_routing(monkeypatch, no_library):  # noqa: F811
    from nmf_amd import NMF
    from nmf_amd import transform as T
    from nmf_amd._driver import Results
    x, mask, w, h0 = data()
    dense = np.where(mask, x, 0.0)
    nmf = NMF(dense, 3)
    with pytest.raises(RuntimeError, match="factorize"):
        nmf.transform(sparse_x())
    calls, tcalls = [], []
    monkeypatch.setattr(H, "hals_transform", lambda data_, w_, **kw: calls.append((data_, w_, kw)) or "folded")
    monkeypatch.setattr(T, "transform", lambda data_, w_, **kw: tcalls.append((data_, w_, kw)) or "transformed")
    nmf.results = Results(w, h0, 9, [1.0], H.Experiment("hals", 3, "eu", (False, "zero"), 10, 1e-3, 1e-3, 0, 0, 1))
    nmf.w, nmf.h = w, h0
    xs = sparse_x()
    assert nmf.transform(xs) == "folded"
    assert calls[-1][0] is xs and calls[-1][1] is w and calls[-1][2] == {}                    # no distance_type injected
    assert nmf.transform(xs, tol=1e-3, h0=h0) == "folded" and calls[-1][2] == dict(tol=1e-3, h0=h0)
    assert nmf.transform(x, mask=mask, max_sweeps=5) == "folded"
    assert calls[-1][0] is x and calls[-1][2] == dict(mask=mask, max_sweeps=5) and calls[-1][2]["mask"] is mask
    assert nmf.transform(xs, mask=mask) == "folded" and calls[-1][2] == dict(mask=mask)
    assert nmf.transform(x, mask=None) == "folded"                                           # mask among the keywords
    assert not tcalls
    assert nmf.transform(dense, max_iter=5) == "transformed"                                  # every other call: as before
    assert tcalls[-1][0] is dense and tcalls[-1][2] == dict(distance_type="eu", max_iter=5) and len(calls) == 5


def test_transform_itself_keeps_refusing(no_library):  # noqa: F811
    from nmf_amd.transform import transform
    x, mask, w, _ = data()
    with pytest.raises(TypeError, match="scipy.sparse input is not supported"):
        transform(sparse_x(), w)
    with pytest.raises(TypeError, match="mask"):
        transform(np.where(mask, x, 0.0), w, mask=mask)


def test_abi_table_and_library():
    assert L.SIGNATURES["nmfx_hals_foldin_run"][1] == [L._vp, L._dbl, L._dbl, L._i32]
    assert L.SIGNATURES["nmfx_hals_foldin_get_sweeps"][1] == [L._vp, L._vp]
    lib = L.load()
    assert lib.nmfx_version() >= 393 and hasattr(lib, "nmfx_hals_foldin_run") and hasattr(lib, "nmfx_hals_foldin_get_sweeps")
