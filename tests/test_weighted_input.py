"""Per-entry weights for MUR, the part that needs no GPU: the float64 yardstick (tests/weighted_ref.py) pinned to the
existing ones, the validation of `mur(x, k, weights=...)` before any device work, the host objective."""
import numpy as np
import pytest
import scipy.sparse as sp

import is_ref
import masked_ref
from oracle import nmf_ref as R
from weighted_cases import STOP, stop_margins, stop_run
from weighted_ref import weighted_h_step, weighted_mur, weighted_objective, weighted_w_step

RTOL = 1e-12            # the bar tests/test_oracle_golden.py holds the oracle to
KINDS = ("eu", "kl", "is")


def case(seed=0):
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.05, 1.0, (40, 30))
    w = rs.uniform(0.1, 1.0, (40, 4))
    h = rs.uniform(0.1, 1.0, (4, 30))
    m = rs.rand(40, 30) < 0.6
    m[5, :] = False                     # a row and a column without weight
    m[:, 7] = False
    return x, w, h, m


def old_steps(kind, x, m, w, h, lw, lh):
    """(W', H', objective of (W', H')) by the existing yardsticks; m = None: no mask."""
    if kind == "is":
        wn = is_ref.is_w_step(x, w, h, lw, m)
        hn = is_ref.is_h_step(x, wn, h, lh, m)
        return wn, hn, is_ref.is_objective(x, wn, hn, m)
    if m is None:
        wn = R.mur_w_step(kind, x, w, h, w @ h, lw)
        hn = R.mur_h_step(kind, x, wn, h, wn @ h, lh)
        return wn, hn, float(R.objective(x, wn @ hn, kind))
    wn = masked_ref.masked_w_step(kind, x, m, w, h, lw)
    hn = masked_ref.masked_h_step(kind, x, m, wn, h, lh)
    return wn, hn, float(masked_ref.masked_objective(kind, x, m, wn @ hn))


def new_steps(kind, x, om, w, h, lw, lh):
    wn = weighted_w_step(kind, x, om, w, h, lw)
    hn = weighted_h_step(kind, x, om, wn, h, lh)
    return wn, hn, weighted_objective(kind, x, om, wn, hn)


# ---- the yardstick pinned ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lw,lh", [(0.0, 0.0), (0.07, 0.0), (0.0, 0.2)])
def test_zero_one_weights_are_the_masked_yardsticks(kind, lw, lh):
    x, w, h, m = case()
    xn = np.where(m, x, np.nan)
    want = old_steps(kind, xn, m, w, h, lw, lh)
    got = new_steps(kind, xn, m.astype(np.float64), w, h, lw, lh)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=0)
    assert (got[0][5] == 0).all() and (got[1][:, 7] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lw,lh", [(0.0, 0.0), (0.07, 0.0), (0.0, 0.2)])
def test_all_ones_weights_are_the_unweighted_yardsticks(kind, lw, lh):
    x, w, h, _ = case(1)
    want = old_steps(kind, x, None, w, h, lw, lh)
    got = new_steps(kind, x, np.ones(x.shape), w, h, lw, lh)
    for a, b in zip(got, want):
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=0)


@pytest.mark.parametrize("kind", KINDS)
def test_scaling_the_weights_at_lambda_zero(kind):
    """The update is invariant under a common factor of the weights at lambda = 0: exactly for IS (a power of two passes
    through every product, sum and the quotient), to rounding for KL; the Euclidean rule sees it through its 1e-9 guard."""
    x, w, h, m = case(2)
    om = np.where(m, np.random.RandomState(3).uniform(0.2, 5.0, x.shape), 0.0)
    a = new_steps(kind, x, om, w, h, 0.0, 0.0)
    b = new_steps(kind, x, 4 * om, w, h, 0.0, 0.0)
    for p, q in zip(a[:2], b[:2]):
        if kind == "is":
            np.testing.assert_array_equal(p, q)
        else:
            np.testing.assert_allclose(p, q, rtol=1e-12 if kind == "kl" else 1e-6, atol=0)
    np.testing.assert_allclose(b[2], 4 * a[2], rtol=1e-6)


def test_the_loop_is_the_masked_loop():
    x, _, _, m = case(4)
    kw = dict(distance_type="kl", min_iter=3, max_iter=40, tol2=0.5, lambda_w=0.01)
    np.random.seed(5)
    want = masked_ref.masked_mur(np.where(m, x, np.nan), m, 4, **kw)
    np.random.seed(5)
    got = weighted_mur(np.where(m, x, np.nan), m.astype(np.float64), 4, **kw)
    assert got.i == want.i and got.trace["stop_rule"] == want.trace["stop_rule"]
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=1e-9)
    np.testing.assert_allclose(got.w @ got.h, want.w @ want.h, rtol=1e-9)


@pytest.mark.parametrize("kind", KINDS)
def test_stop_cases_of_the_gpu_tests_are_not_marginal(kind):
    x, om, seed, kw, want = stop_run(kind)
    margins = stop_margins(want, kw["tol2"])
    print(f"{kind}: float64 run stops at i = {want.i}, margins {margins}")
    assert want.trace["stop_rule"] == 2 and STOP[kind]["min_iter"] < want.i < 399
    assert min(margins) > 10


# ---- validation, before any device work ----------------------------------------------------------------------------------
def _mur(*a, **kw):
    from nmf_amd.mur import mur
    return mur(*a, **kw)


@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to create an engine fails the test: the refusals must come first."""
    from nmf_amd import engine, mur

    class Forbidden:
        def __init__(self, *a, **kw):
            raise AssertionError("an engine was created before the input was refused")
        for_data = for_sparse = __init__

    monkeypatch.setattr(mur, "Engine", Forbidden)
    monkeypatch.setattr(engine, "Engine", Forbidden)


CASES = ["shape", "negative_w", "nan_w", "inf_w", "none_positive", "underflow_w", "overflow_w", "k129", "k0", "mask", "engine",
         "sparse_x", "sparse_w", "complex_w", "complex_x", "negative_x", "nan_x", "inf_x", "is_zero_x", "is_underflow_x"]


@pytest.mark.parametrize("name", CASES)
def test_validation_before_device_work(name, no_engine):
    x = np.random.RandomState(0).rand(20, 10) + 0.1
    om = np.random.RandomState(1).rand(20, 10) + 0.5
    kw, k, err = {}, 3, ValueError
    if name == "shape":
        om = om.T.copy()
    elif name == "negative_w":
        om[2, 3] = -1e-3
    elif name == "nan_w":
        om[2, 3] = np.nan
    elif name == "inf_w":
        om[2, 3] = np.inf
    elif name == "none_positive":
        om[:] = 0
    elif name == "underflow_w":
        om[2, 3] = 1e-60
    elif name == "overflow_w":
        om[2, 3] = 1e60
    elif name == "k129":
        k = 129
    elif name == "k0":
        k = 0
    elif name == "mask":
        kw["mask"] = np.ones(x.shape, dtype=bool)
    elif name == "engine":
        kw["engine"] = object()
    elif name == "sparse_x":
        x, err = sp.csr_matrix(x), TypeError
    elif name == "sparse_w":
        om, err = sp.csr_matrix(om), TypeError
    elif name == "complex_w":
        om, err = om.astype(np.complex128), TypeError
    elif name == "complex_x":
        x, err = x.astype(np.complex128), TypeError
    elif name == "negative_x":
        x[2, 3] = -1.0
    elif name == "nan_x":
        x[2, 3] = np.nan
    elif name == "inf_x":
        x[2, 3] = np.inf
    elif name == "is_zero_x":
        x[2, 3] = 0.0
        kw["distance_type"] = "is"
    elif name == "is_underflow_x":
        x[2, 3] = 1e-60
        kw["distance_type"] = "is"
    x0 = x.copy()
    om0 = om.copy()
    with pytest.raises(err, match="mask=" if name == "sparse_x" else None):
        _mur(x, k, weights=om, **kw)
    for a, b in ((x, x0), (om, om0)):
        a, b = (a.toarray(), b.toarray()) if sp.issparse(a) else (a, b)
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_prepare_ignores_what_lies_under_zero_weight(kind):
    from nmf_amd import weighted
    x = np.random.RandomState(0).rand(20, 10) + 0.1
    om = np.random.RandomState(1).rand(20, 10) + 0.5
    flags = np.ones(x.shape, dtype=bool)
    for (r, c), bad in (((2, 3), -1.0), ((4, 5), np.nan), ((6, 7), np.inf), ((8, 9), 0.0)):
        x[r, c], om[r, c], flags[r, c] = bad, 0.0, False
    x0, om0 = x.copy(), om.copy()
    x32, w32 = weighted.prepare(x, om, 3, kind)
    np.testing.assert_array_equal(x, x0)
    np.testing.assert_array_equal(om, om0)
    assert x32.dtype == w32.dtype == np.float32 and x32.shape == w32.shape == x.shape
    np.testing.assert_array_equal(x32, np.where(flags, x, 0).astype(np.float32))
    np.testing.assert_array_equal(w32, om.astype(np.float32))
    b32, bw = weighted.prepare(x, flags, 3, kind)                  # a boolean array counts as 0 / 1
    np.testing.assert_array_equal(b32, x32)
    np.testing.assert_array_equal(bw, flags.astype(np.float32))


@pytest.mark.parametrize("kind", KINDS)
def test_host_objective_is_the_yardsticks(kind, monkeypatch):
    from nmf_amd import weighted
    monkeypatch.setattr(weighted, "ROWS", 7)                      # several row blocks, one of them without any weight
    x, w, h, m = case(6)
    om = np.where(m, np.random.RandomState(7).uniform(0.01, 50.0, x.shape), 0.0)
    om[7:14] = 0
    xn = np.where(om > 0, x, np.nan)
    got = weighted.objective(xn, w, h, om, kind)
    np.testing.assert_allclose(got, weighted_objective(kind, xn, om, w, h), rtol=RTOL)
    held_out = (om == 0)                                          # scoring on other cells: 0 / 1 weights there
    np.testing.assert_allclose(weighted.objective(x, w, h, held_out, kind),
                               weighted_objective(kind, x, held_out.astype(np.float64), w, h), rtol=RTOL)
    with pytest.raises(ValueError):
        weighted.objective(xn, w, h, np.ones(x.shape), kind)      # a NaN under positive weight


# ---- the entry points that do not take weights -----------------------------------------------------------------------------
def test_factorize_grid_refuses_weights():
    from nmf_amd.grid import factorize_grid
    x = np.random.RandomState(0).rand(20, 10)
    with pytest.raises(TypeError, match="weights"):
        factorize_grid(x, "mur", features=(2,), weights=np.ones(x.shape))


@pytest.mark.parametrize("method", ["anls", "admm", "ao_admm", "mur_pair"])
def test_other_methods_refuse_weights(method):
    from importlib import import_module

    from nmf_amd import NMF
    x = np.random.RandomState(0).rand(20, 10)
    om = np.ones(x.shape)
    if method == "mur_pair":
        from nmf_amd.mur import mur_pair
        with pytest.raises(TypeError, match="weights"):
            mur_pair(x, 3, [{}, {}], weights=om)
        return
    with pytest.raises(TypeError, match="weights"):
        getattr(import_module("nmf_amd." + method), method)(x, 3, weights=om)
    with pytest.raises(TypeError, match="weights"):
        NMF(x, 3).factorize(method=method, weights=om)


def test_dist_factorize_refuses_weights():
    from nmf_amd import dist as nd
    x = np.random.RandomState(0).rand(12, 9)
    with pytest.raises(TypeError, match="weights"):
        nd.factorize(x, 3, method="mur", backend="gloo", weights=np.ones(x.shape))


def test_abi_version_and_null_handle():
    import ctypes as C

    from nmf_amd import _lib as L
    lib = L.load()
    assert lib.nmfx_version() >= 340
    assert lib.nmfx_upload_weights(C.c_void_p(), None, L.F32, 0, 0, 0) == L.NMFX_E_ARG
    assert lib.nmfx_clear_weights(C.c_void_p()) == L.NMFX_E_ARG
