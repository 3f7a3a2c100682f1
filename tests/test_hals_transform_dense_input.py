"""The input rules of nmf_amd.hals.hals_transform_dense without a GPU: every refusal comes with its class and message before
the library is touched and leaves the global generator and the caller's arrays as they were; a valid call reaches
Engine.for_data; NMF.transform routes solver='hals' on dense data to it and keeps every other route as it was."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd import hals as H
from nmf_amd.hals import hals_transform_dense
from test_beta_input import no_library  # noqa: F401  (the fixture)

WHO = "hals_transform_dense"


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


def data():
    """(x 12 x 9 float64 >= 0 with a zero, w 12 x 3, h0 3 x 9)."""
    rng = np.random.RandomState(3)
    x = rng.uniform(0.1, 1.0, (12, 9))
    x[1, 1] = 0.0
    return x, rng.uniform(0.1, 1.0, (12, 3)), rng.uniform(0.1, 1.0, (3, 9))


REFUSALS = [
    # (keywords, class, start of the message)
    (dict(tol=-1e-9), ValueError, f"{WHO}: tol must be a real number with 0 <= tol < 1 (got tol = -1e-09)"),
    (dict(tol=1.0), ValueError, f"{WHO}: tol must be a real number with 0 <= tol < 1"),
    (dict(tol=float("nan")), ValueError, f"{WHO}: tol must be a real number with 0 <= tol < 1"),
    (dict(tol=float("inf")), ValueError, f"{WHO}: tol must be a real number with 0 <= tol < 1"),
    (dict(tol="1e-4"), ValueError, f"{WHO}: tol must be a real number with 0 <= tol < 1"),
    (dict(tol=True), ValueError, f"{WHO}: tol must be a real number with 0 <= tol < 1"),
    (dict(max_sweeps=0), ValueError, f"{WHO}: max_sweeps must be an integer between 1 and 10000 (got max_sweeps = 0)"),
    (dict(max_sweeps=10001), ValueError, f"{WHO}: max_sweeps must be an integer between 1 and 10000"),
    (dict(max_sweeps=2.5), ValueError, f"{WHO}: max_sweeps must be an integer between 1 and 10000"),
    (dict(max_sweeps=True), ValueError, f"{WHO}: max_sweeps must be an integer between 1 and 10000"),
    (dict(lambda_h=-0.1), ValueError, f"{WHO}: lambda_h must be non-negative (got lambda_h = -0.1)"),
    (dict(lambda_h=float("nan")), ValueError, f"{WHO}: lambda_h must be non-negative"),
    (dict(lambda_h=True), ValueError, f"{WHO}: lambda_h must be non-negative"),
    (dict(h0=np.ones((3, 8))), ValueError, f"{WHO}: h0 has shape (3, 8), expected (3, 9)"),
    (dict(h0=np.ones(9)), ValueError, f"{WHO}: h0 must be 2-D (got 1-D)"),
    (dict(h0=put(np.ones((3, 9)), -0.5)), ValueError, f"{WHO}: h0 has a negative entry"),
    (dict(h0=put(np.ones((3, 9)), np.nan)), ValueError, f"{WHO}: h0 has an entry that is NaN or infinite"),
    (dict(h0=put(np.ones((3, 9)), 1j)), ValueError, f"{WHO}: h0 must be a real array"),
    (dict(w=put(np.ones((12, 3)), -0.5)), ValueError, f"{WHO}: w has a negative entry"),
    (dict(w=put(np.ones((12, 3)), np.inf)), ValueError, f"{WHO}: w has an entry that is NaN or infinite"),
    (dict(w=put(np.ones((12, 3)), 1j)), ValueError, f"{WHO}: w must be a real array"),
    (dict(w=np.ones(12)), ValueError, f"{WHO}: w must be 2-D (got 1-D)"),
    (dict(w=np.ones((11, 3))), ValueError, f"{WHO}: w has 11 rows, x_new has 12"),
    (dict(w=np.ones((12, 0))), ValueError, f"{WHO}: supports 1 <= k <= 128 components (w has 0 columns)"),
    (dict(w=np.ones((12, 129))), ValueError, f"{WHO}: supports 1 <= k <= 128 components (w has 129 columns)"),
    (dict(mask=np.ones((12, 9), bool)), TypeError, f"{WHO}() got an unexpected keyword argument 'mask'"),
    (dict(sweeps=2), TypeError, f"{WHO}() got an unexpected keyword argument 'sweeps'"),
    (dict(distance_type="eu"), TypeError, f"{WHO}() got an unexpected keyword argument 'distance_type'"),
    (dict(x=put(data()[0], -0.5)), ValueError, f"{WHO}: the data must be non-negative (an entry is negative or NaN)"),
    (dict(x=put(data()[0], np.nan)), ValueError, f"{WHO}: the data must be non-negative (an entry is negative or NaN)"),
    (dict(x=put(data()[0], np.inf)), ValueError, f"{WHO}: an entry is infinite or beyond the float32 range"),
    (dict(x=put(data()[0], 1e39)), ValueError, f"{WHO}: an entry is infinite or beyond the float32 range"),
    (dict(x=put(data()[0], 1e-50)), ValueError, f"{WHO}: a positive entry is below the float32 range"),
    (dict(x=put(data()[0], 1j)), ValueError, f"{WHO}: x_new must be a real array"),
    (dict(x=data()[0][0]), ValueError, f"{WHO}: x_new must be 2-D (got 1-D)"),
    (dict(x=np.zeros((12, 0)), h0=None), ValueError, f"{WHO}: x_new is empty"),
    (dict(x=sp.csr_matrix(data()[0])), TypeError, f"{WHO}: x_new must be a dense array; scipy.sparse data"),
]


@pytest.mark.parametrize("kw,exc,start", REFUSALS, ids=[f"{i}-{next(iter(r[0]))}" for i, r in enumerate(REFUSALS)])
def test_refusals(kw, exc, start, no_library):  # noqa: F811
    x, w, h0 = data()
    args = dict(x=x, w=w, h0=h0)
    args.update(kw)
    x, w = args.pop("x"), args.pop("w")
    keep = None if sp.issparse(x) else np.array(x)
    err = refused(lambda: hals_transform_dense(x, w, **args))
    assert type(err) is exc and str(err).startswith(start), repr(err)
    if keep is not None:
        assert np.array_equal(x, keep, equal_nan=True)


def test_the_sparse_refusal_points_to_hals_transform(no_library):  # noqa: F811
    x, w, _ = data()
    err = refused(lambda: hals_transform_dense(sp.coo_matrix(x), w))
    assert type(err) is TypeError and "nmf_amd.hals.hals_transform" in str(err)


def test_hals_transform_keeps_its_refusal(no_library):  # noqa: F811
    x, w, _ = data()
    err = refused(lambda: H.hals_transform(x, w))
    assert type(err) is TypeError and str(err).startswith("hals_transform: dense x_new needs mask=")
    assert "transform(x_new, w, distance_type='eu')" in str(err)


# ---- a valid call reaches the engine -----------------------------------------------------------------------------------------------
class _Reached(Exception):
    pass


def test_the_base_case_reaches_for_data(monkeypatch):
    """Every check passed: the next thing is Engine.for_data on x_new with w's k; no draw is made with h0 left out; the defaults
    are those of hals_transform and keyword-only."""
    from nmf_amd.engine import Engine
    seen = {}

    def for_data(x, k, device=0, engine=None):
        seen.update(x=x, k=k, device=device, engine=engine)
        raise _Reached()
    monkeypatch.setattr(Engine, "for_data", staticmethod(for_data))
    x, w, _ = data()
    keep = x.copy(), w.copy()
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(_Reached):
        hals_transform_dense(x, w, device=2)
    assert np.array_equal(np.random.rand(4), want)
    assert np.array_equal(np.asarray(seen["x"]), keep[0]) and seen["k"] == 3 and seen["device"] == 2 and seen["engine"] is None
    assert np.array_equal(x, keep[0]) and np.array_equal(w, keep[1])
    sig = inspect.signature(hals_transform_dense)
    names = ("h0", "lambda_h", "tol", "max_sweeps", "device")
    assert list(sig.parameters) == ["x_new", "w"] + list(names)
    assert [sig.parameters[n].default for n in names] == [None, 0, 1e-4, 200, 0]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names)


def test_a_valid_call_gets_to_the_library(no_library):  # noqa: F811
    x, w, h0 = data()
    with pytest.raises(AssertionError, match="library was touched"):
        hals_transform_dense(x, w, h0=h0)
    with pytest.raises(AssertionError, match="library was touched"):
        hals_transform_dense(x.astype(np.float32), w, tol=0, max_sweeps=10000, lambda_h=0.5)
    with pytest.raises(AssertionError, match="library was touched"):
        hals_transform_dense((x > 0.5).astype(int), np.ones((12, 128)))          # integer data, the largest k


# ---- NMF.transform ------------------------------------------------------------------------------------------------------------
def _fitted(monkeypatch):
    from nmf_amd import NMF
    from nmf_amd import transform as T
    from nmf_amd._driver import Results
    x, w, h0 = data()
    nmf = NMF(x, 3)
    calls = dict(dense=[], folded=[], mur=[])
    monkeypatch.setattr(H, "hals_transform_dense", lambda data_, w_, **kw: calls["dense"].append((data_, w_, kw)) or "dense")
    monkeypatch.setattr(H, "hals_transform", lambda data_, w_, **kw: calls["folded"].append((data_, w_, kw)) or "folded")
    monkeypatch.setattr(T, "transform", lambda data_, w_, **kw: calls["mur"].append((data_, w_, kw)) or "transformed")
    return nmf, calls, x, w, h0, Results(w, h0, 9, [1.0], H.Experiment("hals", 3, "eu", (False, "zero"), 10, 1e-3, 1e-3, 0, 0, 1))


def test_nmf_transform_routes_solver_hals(monkeypatch, no_library):  # noqa: F811
    nmf, calls, x, w, h0, results = _fitted(monkeypatch)
    with pytest.raises(RuntimeError, match="factorize"):
        nmf.transform(x, solver="hals")
    nmf.results, nmf.w, nmf.h = results, w, h0
    xs, mask = sp.csr_matrix(x), x > 0.3
    assert nmf.transform(x, solver="hals") == "dense"
    assert calls["dense"][-1][0] is x and calls["dense"][-1][1] is w and calls["dense"][-1][2] == {}      # no distance_type, no solver
    assert nmf.transform(x, solver="hals", tol=1e-3, h0=h0, max_sweeps=7) == "dense"
    assert calls["dense"][-1][2] == dict(tol=1e-3, h0=h0, max_sweeps=7)
    assert nmf.transform(xs, solver="hals", tol=1e-3) == "folded" and calls["folded"][-1][0] is xs and calls["folded"][-1][2] == dict(tol=1e-3)
    assert nmf.transform(x, solver="hals", mask=mask) == "folded" and calls["folded"][-1][2] == dict(mask=mask)
    assert nmf.transform(x, solver="hals", mask=None) == "folded" and calls["folded"][-1][2] == dict(mask=None)
    assert len(calls["dense"]) == 2 and len(calls["folded"]) == 3 and not calls["mur"]


def test_nmf_transform_solver_mur_is_the_default_route(monkeypatch, no_library):  # noqa: F811
    nmf, calls, x, w, h0, results = _fitted(monkeypatch)
    nmf.results, nmf.w, nmf.h = results, w, h0
    xs, mask = sp.csr_matrix(x), x > 0.3
    for extra in ({}, dict(solver="mur")):
        assert nmf.transform(x, max_iter=5, **extra) == "transformed"
        assert calls["mur"][-1][0] is x and calls["mur"][-1][1] is w and calls["mur"][-1][2] == dict(distance_type="eu", max_iter=5)
        assert nmf.transform(x, distance_type="kl", **extra) == "transformed" and calls["mur"][-1][2] == dict(distance_type="kl")
        assert nmf.transform(xs, **extra) == "folded" and calls["folded"][-1][0] is xs and calls["folded"][-1][2] == {}
        assert nmf.transform(xs, tol=1e-3, h0=h0, **extra) == "folded" and calls["folded"][-1][2] == dict(tol=1e-3, h0=h0)
        assert nmf.transform(x, mask=mask, max_sweeps=5, **extra) == "folded"
        assert calls["folded"][-1][0] is x and calls["folded"][-1][2] == dict(mask=mask, max_sweeps=5) and calls["folded"][-1][2]["mask"] is mask
        assert nmf.transform(xs, mask=mask, **extra) == "folded" and calls["folded"][-1][2] == dict(mask=mask)
        assert nmf.transform(x, mask=None, **extra) == "folded"
    assert not calls["dense"] and len(calls["mur"]) == 4 and len(calls["folded"]) == 10


@pytest.mark.parametrize("bad", ["cd", "HALS", "", None, 1, ("hals",)])
def test_nmf_transform_refuses_another_solver_before_anything_else(bad, monkeypatch, no_library):  # noqa: F811
    nmf, calls, x, w, h0, results = _fitted(monkeypatch)
    with pytest.raises(ValueError, match="NMF.transform: solver must be 'mur' or 'hals'"):       # even before "factorize first"
        nmf.transform(x, solver=bad)
    nmf.results, nmf.w, nmf.h = results, w, h0
    for args in ((x,), (sp.csr_matrix(x),)):
        err = refused(lambda: nmf.transform(*args, solver=bad))
        assert type(err) is ValueError and repr(bad) in str(err)
    assert not any(calls.values())


def test_abi_table_and_library():
    assert L.SIGNATURES["nmfx_hals_foldin_dense_run"] == (L._i32, [L._vp, L._dbl, L._dbl, L._i32])
    assert L.SIGNATURES["nmfx_hals_foldin_dense_get_sweeps"] == (L._i32, [L._vp, L._vp])
    lib = L.load()
    assert lib.nmfx_version() >= 394
    assert hasattr(lib, "nmfx_hals_foldin_dense_run") and hasattr(lib, "nmfx_hals_foldin_dense_get_sweeps")
