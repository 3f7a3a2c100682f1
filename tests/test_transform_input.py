"""Fold-in without a GPU: the float64 yardstick of tests/transform_ref.py checked on its own, and everything
nmf_amd.transform.transform / NMF.transform decide before the library is touched."""
import numpy as np
import pytest
import scipy.sparse as sp

from transform_ref import h_step, objective, transform_ref
from weighted_cases import log_uniform_weights

EPS = 1e-9


@pytest.fixture
def no_library(monkeypatch):
    """Any use of libnmfx fails the test: validation has to come first."""
    from nmf_amd import _lib

    def touched(*a, **kw):
        raise AssertionError("the library was touched before the input was validated")

    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "require_gpu", touched)


def _transform(*a, **kw):
    from nmf_amd.transform import transform
    return transform(*a, **kw)


# ---- the float64 helper on its own -----------------------------------------------------------------------------------------
def test_helper_on_a_hand_worked_1x1_case():
    x, w, h = np.array([[2.0]]), np.array([[1.0]]), np.array([[1.0]])
    q = 1.0 + EPS
    # eu: h (w x) / (w w h + lam h + 1e-9);  1/2 (2 - 1)^2
    assert h_step("eu", x, w, h)[0, 0] == pytest.approx(2.0 / q, rel=1e-15)
    assert h_step("eu", x, w, h, 0.5)[0, 0] == pytest.approx(2.0 / (1.5 + EPS), rel=1e-15)
    assert objective("eu", x, w, h) == pytest.approx(0.5, rel=1e-15)
    # kl: A = h w (x / (wh + 1e-9)) = 2 / q, B = w = 1;  2 A / (B + sqrt(B^2 + 4 lam A));  2 log 2 - 2 + 1
    a = 2.0 / q
    assert h_step("kl", x, w, h)[0, 0] == pytest.approx(a, rel=1e-15)
    assert h_step("kl", x, w, h, 0.5)[0, 0] == pytest.approx(2 * a / (1 + np.sqrt(1 + 2 * a)), rel=1e-15)
    assert objective("kl", x, w, h) == pytest.approx(2 * np.log(2.0) - 1.0, rel=1e-15)
    # is: sqrt((2 / q^2) / (1 / q + lam));  2 / q - log(2 / q) - 1
    assert h_step("is", x, w, h)[0, 0] == pytest.approx(np.sqrt(2.0 / q), rel=1e-15)
    assert h_step("is", x, w, h, 0.5)[0, 0] == pytest.approx(np.sqrt((2.0 / q ** 2) / (1.0 / q + 0.5)), rel=1e-15)
    assert objective("is", x, w, h) == pytest.approx(2.0 / q - np.log(2.0 / q) - 1.0, rel=1e-15)
    # beta = 1/2: gamma = 2/3, (2 q^-1.5 / q^-.5)^(2/3);  beta = 2.5: gamma = 2/3, (2 q^.5 / q^1.5)^(2/3)
    assert h_step("beta", x, w, h, beta=0.5)[0, 0] == pytest.approx((2.0 / q) ** (2.0 / 3.0), rel=1e-15)
    assert h_step("beta", x, w, h, beta=2.5)[0, 0] == pytest.approx((2.0 / q) ** (2.0 / 3.0), rel=1e-15)
    assert objective("beta", x, w, h, beta=0.5) == pytest.approx((np.sqrt(2.0) - 0.5 * q ** 0.5 - q ** -0.5) / -0.25, rel=1e-14)
    # weights: om = 3 cancels in the eu quotient up to the guard, and scales the objective
    om = np.array([[3.0]])
    assert h_step("eu", x, w, h, om=om)[0, 0] == pytest.approx(6.0 / (3.0 + EPS), rel=1e-15)
    assert objective("eu", x, w, h, om=om) == pytest.approx(1.5, rel=1e-15)
    # no weight: nothing observed, a zero denominator, 0
    none = np.zeros((1, 1))
    for kind, kw in (("kl", {}), ("is", {}), ("beta", dict(beta=0.5))):
        assert h_step(kind, x, w, h, om=none, **kw)[0, 0] == 0.0 and objective(kind, x, w, h, om=none, **kw) == 0.0


def test_loop_matches_its_steps_and_the_stop_rule():
    rng = np.random.RandomState(3)
    x, w = rng.uniform(0.1, 2.0, (30, 20)), rng.uniform(0.1, 1.0, (30, 4))
    keep = w.copy()
    np.random.seed(5)
    out = transform_ref(x, w, "is", min_iter=3, max_iter=3)
    np.random.seed(5)
    h = np.abs(np.random.randn(4, 20))                   # ONE draw, H only
    hist = [objective("is", x, w, h)]
    for _ in range(3):
        h = h_step("is", x, w, h)
        hist.append(objective("is", x, w, h))
    assert out.i == 2 and out.obj_history == hist and np.array_equal(out.h, h)
    assert np.array_equal(out.w, keep) and np.array_equal(w, keep)
    # the stop rule after min_iter: rule 2 with a coarse tol2 fires at the first tested index, min_iter + 1
    h0 = rng.uniform(0.1, 1.0, (4, 20))
    out = transform_ref(x, w, "kl", h0=h0, min_iter=2, max_iter=50, tol2=1e9)
    assert out.i == 3 and out.trace["stop_rule"] == 2 and len(out.obj_history) == 5
    out = transform_ref(x, w, "kl", h0=h0, min_iter=2, max_iter=3, tol2=1e9)
    assert out.i == 2 and out.trace["stop_rule"] == 0 and len(out.obj_history) == 4


def mono_case(kind, beta, variant):
    rng = np.random.RandomState(0)
    x = rng.uniform(0.1, 2.0, (60, 40))
    w, h = rng.uniform(0.1, 1.0, (60, 5)), rng.uniform(0.1, 1.0, (5, 40))
    om = None
    if variant == "zeros":
        x[rng.rand(60, 40) < 0.3] = 0.0
    if variant == "weighted":
        om = log_uniform_weights(x.shape, seed=7).astype(np.float64)
        x = np.where(om > 0, x, np.nan)
    return x, w, h, om


LOSSES = [("eu", None), ("kl", None), ("is", None), ("beta", -1.0), ("beta", 0.5), ("beta", 1.5), ("beta", 2.5)]
MONO = [(kind, beta, variant) for kind, beta in LOSSES for variant in ("plain", "weighted", "zeros")
        if variant != "zeros" or kind in ("eu", "kl") or (kind == "beta" and beta > 0)]


@pytest.mark.parametrize("kind,beta,variant", MONO)
def test_no_step_increases_the_objective(kind, beta, variant):
    """With W fixed the H half-step is the MM step of its loss: at lambda_h = 0 the objective never rises."""
    x, w, h, om = mono_case(kind, beta, variant)
    obj = [objective(kind, x, w, h, om, beta)]
    for _ in range(100):
        h = h_step(kind, x, w, h, 0.0, om, beta)
        obj.append(objective(kind, x, w, h, om, beta))
        assert obj[-1] <= obj[-2] + 1e-12 * abs(obj[-2]), (len(obj) - 2, obj[-2], obj[-1])
    assert np.isfinite(obj).all() and obj[-1] < obj[0]


@pytest.mark.parametrize("kind,beta", LOSSES)
@pytest.mark.parametrize("weighted_form", [False, True])
def test_columns_are_separable(kind, beta, weighted_form):
    """Column j of H depends on column j of x (and of the weights) alone: the H of x[:, a:b] from h0[:, a:b] is columns
    a:b of the full run."""
    x, w, h0, om = mono_case(kind, beta, "weighted" if weighted_form else "plain")
    a, b = 7, 19
    kw = dict(beta=beta, min_iter=12, max_iter=12, lambda_h=0.05)
    full = transform_ref(x, w, kind, om=om, h0=h0, **kw)
    part = transform_ref(x[:, a:b], w, kind, om=None if om is None else om[:, a:b], h0=h0[:, a:b], **kw)
    assert full.i == part.i == 11
    np.testing.assert_allclose(part.h, full.h[:, a:b], rtol=1e-12, atol=0)


# ---- what transform decides before the library is touched -----------------------------------------------------------------
def data(m=12, n=9, k=3, seed=0):
    rng = np.random.RandomState(seed)
    return rng.uniform(0.1, 2.0, (m, n)), rng.uniform(0.1, 1.0, (m, k)), rng.uniform(0.1, 1.0, (k, n))


def test_signature():
    import inspect
    from nmf_amd.transform import TransformResults, transform
    p = inspect.signature(transform).parameters
    assert list(p)[:2] == ["x", "w"]
    want = dict(distance_type="kl", beta=None, weights=None, h0=None, min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5,
                lambda_h=0.0, device=0)
    assert {key: val.default for key, val in p.items() if key not in ("x", "w")} == want
    assert all(p[key].kind is inspect.Parameter.KEYWORD_ONLY for key in want)
    assert TransformResults._fields == ("h", "i", "obj_history", "experiment")


@pytest.mark.parametrize("kind,kw", [("eu", {}), ("kl", {}), ("is", {}), ("beta", dict(beta=0.5)), ("beta", dict(beta=-1.0))])
@pytest.mark.parametrize("weighted_form", [False, True])
def test_valid_requests_reach_the_library_and_nothing_is_modified(kind, kw, weighted_form, no_library):
    x, w, h0 = data()
    if weighted_form:
        kw = dict(kw, weights=log_uniform_weights(x.shape, seed=1))
        x[kw["weights"] == 0] = np.nan
    keep = x.copy(), w.copy(), h0.copy()
    for start in (None, h0):
        with pytest.raises(AssertionError, match="library was touched"):
            _transform(x, w, distance_type=kind, h0=start, max_iter=2, **kw)
    for got, want in zip((x, w, h0), keep):
        np.testing.assert_array_equal(got, want)
    xw, ww, _ = data(k=128)
    with pytest.raises(AssertionError, match="library was touched"):
        _transform(xw, ww, distance_type="eu", max_iter=1)
    with pytest.raises(AssertionError, match="library was touched"):      # zeros are data for eu, kl and beta > 0
        xz = x.copy() if not weighted_form else np.nan_to_num(x)
        xz[0, 0] = 0.0
        _transform(xz, w, distance_type="kl", max_iter=2)


def test_the_start_is_one_draw_of_h(no_library):
    x, w, _ = data()
    np.random.seed(3)
    with pytest.raises(AssertionError, match="library was touched"):
        _transform(x, w, max_iter=2)
    after = np.random.rand()
    np.random.seed(3)
    np.random.randn(3, 9)
    assert np.random.rand() == after
    np.random.seed(3)                                    # with h0 nothing is drawn
    with pytest.raises(AssertionError, match="library was touched"):
        _transform(x, w, h0=np.ones((3, 9)), max_iter=2)
    np.random.seed(3)
    first = np.random.rand()
    np.random.seed(3)
    with pytest.raises(AssertionError, match="library was touched"):
        _transform(x, w, h0=np.ones((3, 9)), max_iter=2)
    assert np.random.rand() == first


def test_type_errors(no_library):
    x, w, _ = data()
    for make in (sp.csr_matrix, sp.csc_matrix, sp.coo_matrix):
        with pytest.raises(TypeError, match="sparse"):
            _transform(make(x), w, max_iter=2)
    with pytest.raises(TypeError, match="mask"):
        _transform(x, w, mask=np.ones(x.shape, dtype=bool), max_iter=2)


def bad_x(case):
    x, w, _ = data()
    x[2, 3] = {"negative": -0.5, "nan": np.nan, "inf": np.inf, "huge": 1e39, "tiny": 1e-50, "zero": 0.0}[case]
    return x, w


@pytest.mark.parametrize("case", ["negative", "nan", "inf", "huge", "tiny"])
@pytest.mark.parametrize("kind,kw", [("eu", {}), ("kl", {}), ("is", {}), ("beta", dict(beta=0.5)), ("beta", dict(beta=0.0))])
def test_unweighted_values(case, kind, kw, no_library):
    """finite and >= 0 in float32, never lifted; a positive value must not underflow to 0."""
    x, w = bad_x(case)
    keep = x.copy()
    with pytest.raises(ValueError):
        _transform(x, w, distance_type=kind, max_iter=2, **kw)
    np.testing.assert_array_equal(x, keep)


@pytest.mark.parametrize("kind,kw", [("is", {}), ("beta", dict(beta=0.0)), ("beta", dict(beta=-1.0))])
def test_a_zero_is_refused_where_the_loss_needs_positive_data(kind, kw, no_library):
    x, w = bad_x("zero")
    with pytest.raises(ValueError, match="positive"):
        _transform(x, w, distance_type=kind, max_iter=2, **kw)
    om = np.ones(x.shape)
    with pytest.raises(ValueError):
        _transform(x, w, distance_type=kind, weights=om, max_iter=2, **kw)
    om[2, 3] = 0                                         # ... unless the cell carries no weight
    with pytest.raises(AssertionError, match="library was touched"):
        _transform(x, w, distance_type=kind, weights=om, max_iter=2, **kw)


def test_weighted_input_goes_through_prepare(no_library):
    x, w, _ = data()
    for bad in (-np.ones(x.shape), np.full(x.shape, np.nan), np.zeros(x.shape), np.ones((3, 3))):
        with pytest.raises(ValueError):
            _transform(x, w, weights=bad, max_iter=2)
    xn = x.copy()
    xn[1, 1] = np.nan                                    # under positive weight
    with pytest.raises(ValueError):
        _transform(xn, w, weights=np.ones(x.shape), max_iter=2)


def test_refusals_of_w_h0_and_the_rest(no_library):
    x, w, h0 = data()

    def refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            _transform(*a, max_iter=kw.pop("max_iter", 2), **kw)

    refused("2-D", x[0], w)
    refused("2-D", x[None], w)
    refused("2-D", x, w[:, 0])
    refused("rows", x, w[:-1])
    refused("128", x, np.ones((12, 129)))
    refused("128", x, np.ones((12, 0)))
    for bad in (-0.5, np.nan, np.inf):
        wb, hb = w.copy(), h0.copy()
        wb[1, 1] = hb[1, 1] = bad
        refused("w ", x, wb)
        refused("h0", x, w, h0=hb)
    refused("h0", x, w, h0=h0[:, :-1])
    refused("h0", x, w, h0=h0.T)
    refused("h0", x, w, h0=h0[0])
    refused("max_iter", x, w, max_iter=0)
    refused("max_iter", x, w, max_iter=-3)
    refused("distance_type", x, w, distance_type="xx")
    refused("beta", x, w, distance_type="beta")
    refused("beta", x, w, distance_type="beta", beta=3.5)
    refused("beta", x, w, distance_type="beta", beta=float("nan"))
    refused("beta", x, w, distance_type="kl", beta=1.0)


# ---- NMF.transform ------------------------------------------------------------------------------------------------------------
def test_nmf_transform(monkeypatch, no_library):
    from nmf_amd import NMF
    from nmf_amd import transform as T
    from nmf_amd.mur import BetaExperiment, Experiment
    from nmf_amd._driver import Results
    x, w, h = data()
    nmf = NMF(x, 3)
    with pytest.raises(RuntimeError, match="factorize"):
        nmf.transform(x)
    calls, real = [], T.transform
    monkeypatch.setattr(T, "transform", lambda data_, w_, **kw: calls.append((data_, w_, kw)) or "result")
    exp = Experiment("mur", 3, "is", (False, "zero"), 10, 1e-5, 1e-5, 0.0, 0.0)
    nmf.results = Results(w, h, 9, [1.0], exp)
    nmf.w, nmf.h = w, h
    new = x[:, :4]
    assert nmf.transform(new, max_iter=5) == "result"
    assert calls[-1][0] is new and calls[-1][1] is w and calls[-1][2] == dict(distance_type="is", max_iter=5)
    nmf.transform(new, distance_type="kl")
    assert calls[-1][2] == dict(distance_type="kl")
    nmf.results = Results(w, h, 9, [1.0], BetaExperiment(*exp._replace(distance_type="beta"), 0.5))
    nmf.transform(new)
    assert calls[-1][2] == dict(distance_type="beta", beta=0.5)
    nmf.transform(new, beta=1.5)
    assert calls[-1][2] == dict(distance_type="beta", beta=1.5)
    nmf.transform(new, distance_type="eu")                # another loss: the stored beta does not follow
    assert calls[-1][2] == dict(distance_type="eu")
    monkeypatch.setattr(T, "transform", real)
    with pytest.raises(AssertionError, match="library was touched"):      # the real function, through the class
        nmf.transform(new, max_iter=2)
