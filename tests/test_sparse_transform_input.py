"""The input rules of nmf_amd.transform.transform_sparse without a GPU: every refusal comes with its class and full message
before the library is touched and leaves the global generator and the caller's arrays as they were; the default start is
sqrt(mean / k) with no draw; NMF.transform_sparse fills distance_type from the last factorize; the ABI table has the two rows."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd import transform as TR
from nmf_amd.transform import transform_sparse
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


IS_TEXT = ("transform_sparse: distance_type='is': the zeros of a sparse matrix have infinite Itakura-Saito divergence; "
           "pass mask= (for instance the matrix's own pattern) to fit the stored entries only")
REFUSALS = [
    # (which input, keywords, class, the full message)
    ("both", dict(distance_type="beta"), ValueError, "transform_sparse: distance_type must be 'eu', 'kl' or 'is' (got 'beta')"),
    ("both", dict(distance_type="l2"), ValueError, "transform_sparse: distance_type must be 'eu', 'kl' or 'is' (got 'l2')"),
    ("both", dict(distance_type=None), ValueError, "transform_sparse: distance_type must be 'eu', 'kl' or 'is' (got None)"),
    ("sparse", dict(distance_type="is"), ValueError, IS_TEXT),
    ("both", dict(tol=-1e-9), ValueError, "transform_sparse: tol must be a real number with 0 <= tol < 1 (got tol = -1e-09)"),
    ("both", dict(tol=1.0), ValueError, "transform_sparse: tol must be a real number with 0 <= tol < 1 (got tol = 1.0)"),
    ("both", dict(tol=float("nan")), ValueError, "transform_sparse: tol must be a real number with 0 <= tol < 1 (got tol = nan)"),
    ("both", dict(tol="1e-4"), ValueError, "transform_sparse: tol must be a real number with 0 <= tol < 1 (got tol = '1e-4')"),
    ("both", dict(tol=True), ValueError, "transform_sparse: tol must be a real number with 0 <= tol < 1 (got tol = True)"),
    ("both", dict(max_iter=0), ValueError, "transform_sparse: max_iter must be an integer between 1 and 10000 (got max_iter = 0)"),
    ("both", dict(max_iter=10001), ValueError, "transform_sparse: max_iter must be an integer between 1 and 10000 (got max_iter = 10001)"),
    ("both", dict(max_iter=2.5), ValueError, "transform_sparse: max_iter must be an integer between 1 and 10000 (got max_iter = 2.5)"),
    ("both", dict(max_iter=True), ValueError, "transform_sparse: max_iter must be an integer between 1 and 10000 (got max_iter = True)"),
    ("both", dict(lambda_h=-0.1), ValueError, "transform_sparse: lambda_h must be a real number >= 0 (got lambda_h = -0.1)"),
    ("both", dict(lambda_h=float("nan")), ValueError, "transform_sparse: lambda_h must be a real number >= 0 (got lambda_h = nan)"),
    ("both", dict(lambda_h=True), ValueError, "transform_sparse: lambda_h must be a real number >= 0 (got lambda_h = True)"),
    ("both", dict(h0=np.ones((3, 8))), ValueError, "transform_sparse: h0 has shape (3, 8), expected (3, 9)"),
    ("both", dict(h0=np.ones(9)), ValueError, "transform_sparse: h0 must be 2-D (got 1-D)"),
    ("both", dict(h0=put(np.ones((3, 9)), -0.5)), ValueError, "transform_sparse: h0 has a negative entry"),
    ("both", dict(h0=put(np.ones((3, 9)), np.nan)), ValueError, "transform_sparse: h0 has an entry that is NaN or infinite"),
    ("both", dict(h0=put(np.ones((3, 9)), 1j)), ValueError, "transform_sparse: h0 must be a real array"),
    ("both", dict(w=put(np.ones((12, 3)), -0.5)), ValueError, "transform_sparse: w has a negative entry"),
    ("both", dict(w=put(np.ones((12, 3)), np.inf)), ValueError, "transform_sparse: w has an entry that is NaN or infinite"),
    ("both", dict(w=put(np.ones((12, 3)), 1j)), ValueError, "transform_sparse: w must be a real array"),
    ("both", dict(w=np.ones(12)), ValueError, "transform_sparse: w must be 2-D (got 1-D)"),
    ("both", dict(w=np.ones((11, 3))), ValueError, "transform_sparse: w has 11 rows, x_new has 12"),
    ("both", dict(w=np.ones((12, 0))), ValueError, "transform_sparse: supports 1 <= k <= 256 components (w has 0 columns)"),
    ("both", dict(w=np.ones((12, 257))), ValueError, "transform_sparse: supports 1 <= k <= 256 components (w has 257 columns)"),
    ("both", dict(max_sweeps=2), TypeError, "transform_sparse() got an unexpected keyword argument 'max_sweeps'"),
    ("both", dict(beta=1.5), TypeError, "transform_sparse() got an unexpected keyword argument 'beta'"),
    ("both", dict(weights=np.ones((12, 9))), TypeError, "transform_sparse() got an unexpected keyword argument 'weights'"),
    # two rules broken: which refusal comes first
    ("both", dict(distance_type="beta", tol=2.0), ValueError, "transform_sparse: distance_type must be 'eu', 'kl' or 'is' (got 'beta')"),
    ("sparse", dict(distance_type="is", w=put(np.ones((12, 3)), -0.5)), ValueError, IS_TEXT),
    ("both", dict(w=put(np.ones((12, 3)), -0.5), tol=2.0), ValueError, "transform_sparse: w has a negative entry"),
    ("both", dict(w=np.ones((12, 257)), tol=2.0), ValueError, "transform_sparse: supports 1 <= k <= 256 components (w has 257 columns)"),
    ("both", dict(tol=2.0, max_iter=0), ValueError, "transform_sparse: tol must be a real number with 0 <= tol < 1 (got tol = 2.0)"),
    ("both", dict(max_iter=0, lambda_h=-1.0), ValueError, "transform_sparse: max_iter must be an integer between 1 and 10000 (got max_iter = 0)"),
    ("both", dict(lambda_h=-1.0, w=np.ones((11, 3))), ValueError, "transform_sparse: lambda_h must be a real number >= 0 (got lambda_h = -1.0)"),
    ("both", dict(w=np.ones((11, 3)), h0=np.ones((3, 8))), ValueError, "transform_sparse: w has 11 rows, x_new has 12"),
]


def _call(kind, kw):
    x, mask, w, h0 = data()
    args = dict(w=w, h0=h0)
    args.update(kw)
    w = args.pop("w")
    if kind == "sparse":
        xs = sparse_x()
        keep = xs.copy()
        err = refused(lambda: transform_sparse(xs, w, **args))
        assert (xs != keep).nnz == 0
    else:
        keep = x.copy(), mask.copy()
        err = refused(lambda: transform_sparse(x, w, mask, **args))
        assert np.array_equal(x, keep[0], equal_nan=True) and np.array_equal(mask, keep[1])
    return err


@pytest.mark.parametrize("which,kw,exc,text", REFUSALS, ids=[f"{i}-{'-'.join(r[1])}" for i, r in enumerate(REFUSALS)])
def test_refusals(which, kw, exc, text, no_library):  # noqa: F811
    for kind in (("sparse", "masked") if which == "both" else (which,)):
        err = _call(kind, kw)
        assert type(err) is exc and str(err) == text, (kind, repr(err))


def test_dense_data_without_a_mask_points_to_transform(no_library):  # noqa: F811
    x, mask, w, h0 = data()
    err = refused(lambda: transform_sparse(np.where(mask, x, 0.0), w))
    assert type(err) is TypeError
    assert str(err) == ("transform_sparse: dense x_new needs mask=; without a mask x_new must be a scipy.sparse matrix "
                        "(dense data without a mask: nmf_amd.transform.transform)")
    err = refused(lambda: transform_sparse(np.where(mask, x, 0.0), w, distance_type="is"))        # ... before the 'is' rule
    assert type(err) is TypeError
    err = refused(lambda: transform_sparse(np.where(mask, x, 0.0), w, distance_type="beta"))      # ... behind the loss name
    assert type(err) is ValueError


def _bad_data():
    x, mask, w, _ = data()
    zero_text = "transform_sparse: "
    return [
        ("masked shape", x, mask[:, :8], "kl", ValueError, "transform_sparse: mask has shape (12, 8), data has shape (12, 9)"),
        ("masked negative", put(x, -0.5), mask, "kl", ValueError, "transform_sparse: masked input: an observed value is negative"),
        ("masked nan", put(x, np.nan), mask, "eu", ValueError, "transform_sparse: masked input: an observed value is NaN or infinite"),
        ("masked empty", x, np.zeros((12, 9), bool), "kl", ValueError, "transform_sparse: mask observes no entry"),
        ("masked 1-d", x[0], mask[0], "kl", ValueError, "transform_sparse: masked input must be 2-D"),
        ("masked complex", np.where(mask, 1.0, 0.0).astype(complex), mask, "kl", TypeError, "transform_sparse: masked input must be real"),
        ("masked complex mask", x, mask.astype(complex), "kl", TypeError, "transform_sparse: mask must be real"),
        ("masked is zero", x, mask, "is", ValueError, zero_text),                  # the observed zero: masked.check_positive
        ("sparse negative", sp.csr_matrix(put(np.where(mask, x, 0.0), -0.5)), None, "kl", ValueError, "transform_sparse: sparse input has negative entries"),
        ("sparse complex", sp.csr_matrix(np.where(mask, x, 0.0).astype(complex)), None, "eu", TypeError, "transform_sparse: sparse input must be real"),
    ]


@pytest.mark.parametrize("what,x,mask,loss,exc,start", _bad_data(), ids=[b[0] for b in _bad_data()])
def test_the_data_rules_carry_the_prefix(what, x, mask, loss, exc, start, no_library):  # noqa: F811
    w = data()[2]
    err = refused(lambda: transform_sparse(x, w, mask, distance_type=loss))
    assert type(err) is exc and str(err).startswith(start), repr(err)
    if what == "masked is zero":
        from nmf_amd import masked
        with pytest.raises(ValueError) as e:
            masked.check_positive(masked.observed(x, mask, 3))
        assert str(err) == f"transform_sparse: {e.value}"


# ---- a valid call reaches the library ----------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


class _Engine:
    """Stands in for the engine of a valid call: records what it is given."""
    seen = {}

    def __init__(self, xs, k, device=0, masked=False):
        _Engine.seen = dict(x=xs, k=k, masked=masked, device=device)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def set_factors(self, w, h):
        _Engine.seen.update(w=w, h=h)

    def sparse_foldin_run(self, *a):
        _Engine.seen.update(run=a)
        raise _Reached()


@pytest.mark.parametrize("kind", ["sparse", "masked", "masked sparse x"])
def test_the_default_start_and_the_call_that_reaches_the_library(kind, monkeypatch):
    """Every check passed: the engine gets the canonical CSR (of the observed entries, masked, with a mask), w, the start
    sqrt(mean / k) -- the float64 mean over all m n cells, or over the observed cells with a mask -- and the loss code, lambda_h,
    tol and max_iter; no draw is made."""
    from nmf_amd import losses, masked
    from nmf_amd.engine import Engine
    monkeypatch.setattr(Engine, "for_sparse", staticmethod(lambda xs, k, device=0, masked=False: _Engine(xs, k, device, masked)))
    x, mask, w, _ = data()
    w_keep = w.copy()
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(_Reached):
        if kind == "sparse":
            transform_sparse(sparse_x().tocoo(), w, device=2, distance_type="eu", lambda_h=0.25, tol=1e-3, max_iter=77)
        elif kind == "masked":
            transform_sparse(x, w, mask, device=2, distance_type="eu", lambda_h=0.25, tol=1e-3, max_iter=77)
        else:
            transform_sparse(sparse_x().tocsc(), w, sp.coo_matrix(mask), device=2, distance_type="eu", lambda_h=0.25, tol=1e-3, max_iter=77)
    assert np.array_equal(np.random.rand(4), want)
    seen = _Engine.seen
    assert sp.isspmatrix_csr(seen["x"]) and seen["k"] == 3 and seen["device"] == 2 and seen["masked"] is (kind != "sparse")
    total = float(np.nansum(np.where(mask, x, 0.0)))
    if kind == "sparse":
        assert seen["x"].nnz == mask.sum() - 1                       # (the stored zero is no entry of a sparse matrix)
        mean = total / (12 * 9)
    else:
        obs = masked.observed(x, mask, 3)
        assert seen["x"].nnz == mask.sum() and np.array_equal(seen["x"].indices, obs.indices)        # the observed zero is data
        mean = total / mask.sum()
    assert seen["h"].shape == (3, 9) and seen["h"].dtype == np.float64
    assert np.allclose(seen["h"], np.sqrt(mean / 3), rtol=1e-14, atol=0) and (seen["h"] == seen["h"][0, 0]).all()
    assert np.array_equal(seen["w"], w) and np.array_equal(w, w_keep) and seen["w"] is not w
    assert seen["run"] == (losses.CODES["eu"], 0.25, 1e-3, 77)


def test_the_signature():
    sig = inspect.signature(transform_sparse)
    assert list(sig.parameters) == ["x_new", "w", "mask", "distance_type", "h0", "lambda_h", "tol", "max_iter", "device"]
    names = ("distance_type", "h0", "lambda_h", "tol", "max_iter", "device")
    assert [sig.parameters[n].default for n in ("mask",) + names] == [None, "kl", None, 0.0, 1e-4, 1000, 0]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names)
    assert sig.parameters["mask"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert TR.SparseTransformResults._fields == ("h", "iters", "obj_history", "experiment")


def test_a_valid_call_gets_to_the_library(no_library):  # noqa: F811
    x, mask, w, h0 = data()
    x[1, 1] = 0.5                                        # (no observed zero: 'is' too is valid)
    for loss in ("eu", "kl", "is"):
        with pytest.raises(AssertionError, match="library was touched"):
            transform_sparse(x, w, mask, h0=h0, distance_type=loss)
    for loss in ("eu", "kl"):
        with pytest.raises(AssertionError, match="library was touched"):
            transform_sparse(sparse_x(), w, tol=0, max_iter=10000, lambda_h=0.5, distance_type=loss)
    with pytest.raises(AssertionError, match="library was touched"):
        transform_sparse(sparse_x(), np.ones((12, 256)))


# ---- NMF.transform_sparse -------------------------------------------------------------------------------------------------------
def test_nmf_transform_sparse(monkeypatch, no_library):  # noqa: F811
    from nmf_amd import NMF
    from nmf_amd import hals as H
    from nmf_amd import mur as MU
    from nmf_amd._driver import Results
    x, mask, w, h0 = data()
    xs = sparse_x()
    nmf = NMF(xs, 3)
    with pytest.raises(RuntimeError) as e:
        nmf.transform_sparse(xs)
    with pytest.raises(RuntimeError) as e2:
        nmf.transform(xs)
    assert str(e.value) == str(e2.value) == "NMF.transform needs a dictionary: call factorize first"
    calls = []
    monkeypatch.setattr(TR, "transform_sparse", lambda data_, w_, mask_=None, **kw: calls.append((data_, w_, mask_, kw)) or "folded")

    def fitted(loss):
        exp = MU.Experiment("mur", 3, loss, (False, "zero"), 10, 1e-3, 1e-3, 0, 0)
        nmf.results = Results(w, h0, 9, [1.0], exp)
        nmf.w, nmf.h = w, h0
    for loss in ("eu", "kl", "is"):
        fitted(loss)
        assert nmf.transform_sparse(xs) == "folded"
        assert calls[-1][0] is xs and calls[-1][1] is w and calls[-1][2] is None and calls[-1][3] == dict(distance_type=loss)
        assert nmf.transform_sparse(x, mask, tol=1e-3) == "folded"
        assert calls[-1][0] is x and calls[-1][2] is mask and calls[-1][3] == dict(distance_type=loss, tol=1e-3)
        assert nmf.transform_sparse(x, mask=mask, distance_type="kl") == "folded" and calls[-1][3] == dict(distance_type="kl")
    fitted("beta")
    assert nmf.transform_sparse(xs, max_iter=5) == "folded" and calls[-1][3] == dict(max_iter=5)       # the function's own default
    nmf.results = Results(w, h0, 9, [1.0], H.Experiment("hals", 3, "eu", (False, "zero"), 10, 1e-3, 1e-3, 0, 0, 1))
    assert nmf.transform_sparse(xs) == "folded" and calls[-1][3] == dict(distance_type="eu")
    # NMF.transform keeps its routes: sparse data and mask= still go to the least-squares fold-in
    hcalls = []
    monkeypatch.setattr(H, "hals_transform", lambda data_, w_, **kw: hcalls.append(kw) or "least squares")
    n = len(calls)
    assert nmf.transform(xs) == "least squares" and nmf.transform(x, mask=mask) == "least squares" and len(calls) == n


def test_transform_itself_keeps_refusing(no_library):  # noqa: F811
    from nmf_amd.transform import transform
    x, mask, w, _ = data()
    with pytest.raises(TypeError, match="scipy.sparse input is not supported"):
        transform(sparse_x(), w)
    with pytest.raises(TypeError, match="mask"):
        transform(np.where(mask, x, 0.0), w, mask=mask)
    with pytest.raises(ValueError, match="^transform: w has a negative entry$"):      # _check_factor keeps transform's own name
        transform(np.where(mask, x, 0.0), put(w, -1.0))


def test_abi_table_and_library():
    assert L.SIGNATURES["nmfx_sparse_foldin_run"] == (L._i32, [L._vp, L._i32, L._dbl, L._dbl, L._i32])
    assert L.SIGNATURES["nmfx_sparse_foldin_get_iters"] == (L._i32, [L._vp, L._vp])
    lib = L.load()
    assert lib.nmfx_version() >= 395 and hasattr(lib, "nmfx_sparse_foldin_run") and hasattr(lib, "nmfx_sparse_foldin_get_iters")
