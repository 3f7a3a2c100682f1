"""The beta-divergence of MUR without a GPU: the float64 yardstick of tests/beta_ref.py checked on its own and pinned to the
existing ones at beta = 0, 1, 2, the host objective (nmf_amd.weighted.objective(..., 'beta', beta=)), and everything mur /
NMF / the grid / dist decide before the library is touched."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import is_ref
from beta_ref import EPS, beta_cells, beta_h_step, beta_mur, beta_objective, beta_w_step, gamma
from conftest import ROOT
from oracle import nmf_ref as R
from weighted_cases import log_uniform_weights
from weighted_ref import weighted_h_step, weighted_objective, weighted_w_step

GRID = (-1.0, -0.5, 0.0, 0.5, 0.9, 1.0, 1.5, 2.0, 2.5, 3.0)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of libnmfx fails the test: validation has to come first."""
    from nmf_amd import _lib

    def touched(*a, **kw):
        raise AssertionError("the library was touched before the input was validated")

    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "require_gpu", touched)


def _mur(*a, **kw):
    from nmf_amd.mur import mur
    return mur(*a, **kw)


def case(seed=0):
    rs = np.random.RandomState(seed)
    return rs.uniform(0.05, 1.0, (40, 30)), rs.uniform(0.1, 1.0, (40, 4)), rs.uniform(0.1, 1.0, (4, 30))


# ---- the float64 yardstick on its own --------------------------------------------------------------------------------------
def test_gamma_branches():
    assert gamma(-1.0) == 1.0 / 3.0 and gamma(0.0) == 0.5 and gamma(0.9) == pytest.approx(1 / 1.1, rel=1e-15)
    assert gamma(1.0) == gamma(1.5) == gamma(2.0) == 1.0 and gamma(2.5) == pytest.approx(1 / 1.5, rel=1e-15) and gamma(3.0) == 0.5


def test_hand_worked_1x1_case_at_beta_one_half():
    x, w, h = np.array([[2.0]]), np.array([[1.0]]), np.array([[1.0]])
    q = 1.0 + EPS
    # d = (sqrt 2 - q^.5 / 2 - q^-.5) / (-1/4)
    assert beta_objective(x, w, h, 0.5) == pytest.approx(-4.0 * (np.sqrt(2.0) - 0.5 * np.sqrt(q) - 1.0 / np.sqrt(q)), rel=1e-15)
    # gamma = 2/3: W <- ((2 q^-1.5) / (q^-.5))^(2/3) = (2 / q)^(2/3); with lambda: ((2 q^-1.5) / (q^-.5 + 1/2))^(2/3)
    w1 = beta_w_step(x, w, h, 0.5)
    assert w1[0, 0] == pytest.approx((2.0 / q) ** (2.0 / 3.0), rel=1e-15)
    assert beta_w_step(x, w, h, 0.5, 0.5)[0, 0] == pytest.approx((2.0 * q ** -1.5 / (q ** -0.5 + 0.5)) ** (2.0 / 3.0), rel=1e-15)
    q1 = w1[0, 0] + EPS                                  # H with the new W: (w1 2 q1^-1.5 / (w1 q1^-.5))^(2/3) = (2 / q1)^(2/3)
    assert beta_h_step(x, w1, h, 0.5)[0, 0] == pytest.approx((2.0 / q1) ** (2.0 / 3.0), rel=1e-15)
    none = np.zeros((1, 1))                              # no weight: zero denominator, 0
    assert beta_w_step(x, w, h, 0.5, 0.0, none)[0, 0] == 0.0 and beta_objective(x, w, h, 0.5, none) == 0.0


def test_hand_worked_1x1_case_at_beta_three():
    x, w, h = np.array([[2.0]]), np.array([[1.0]]), np.array([[1.0]])
    q = 1.0 + EPS
    assert beta_objective(x, w, h, 3.0) == pytest.approx((8.0 + 2.0 * q ** 3 - 6.0 * q ** 2) / 6.0, rel=1e-15)
    # gamma = 1/2: W <- sqrt((2 q) / q^2) = sqrt(2 / q); with lambda sqrt(2 q / (q^2 + 1/2))
    w1 = beta_w_step(x, w, h, 3.0)
    assert w1[0, 0] == pytest.approx(np.sqrt(2.0 / q), rel=1e-15)
    assert beta_w_step(x, w, h, 3.0, 0.5)[0, 0] == pytest.approx(np.sqrt(2.0 * q / (q * q + 0.5)), rel=1e-15)
    q1 = w1[0, 0] + EPS
    assert beta_h_step(x, w1, h, 3.0)[0, 0] == pytest.approx(np.sqrt(2.0 / q1), rel=1e-15)


@pytest.mark.parametrize("lw,lh", [(0.0, 0.0), (0.07, 0.2)])
def test_beta_0_is_the_is_yardstick(lw, lh):
    x, w, h = case()
    w1, w2 = beta_w_step(x, w, h, 0.0, lw), is_ref.is_w_step(x, w, h, lw)
    np.testing.assert_allclose(w1, w2, rtol=1e-12, atol=0)
    np.testing.assert_allclose(beta_h_step(x, w1, h, 0.0, lh), is_ref.is_h_step(x, w1, h, lh), rtol=1e-12, atol=0)
    assert beta_objective(x, w, h, 0.0) == pytest.approx(is_ref.is_objective(x, w, h), rel=1e-12)


def test_beta_1_is_the_weighted_kl_yardstick_at_lambda_zero():
    x, w, h = case(1)
    x[3, 4] = 0.0                                        # the log term is 0 there
    ones = np.ones(x.shape)
    w1 = beta_w_step(x, w, h, 1.0)
    np.testing.assert_allclose(w1, weighted_w_step("kl", x, ones, w, h), rtol=1e-12, atol=0)
    np.testing.assert_allclose(beta_h_step(x, w1, h, 1.0), weighted_h_step("kl", x, ones, w1, h), rtol=1e-12, atol=0)
    # (the 'kl' objective has no guard in its q: 1e-9 of q ~ 1 moves the sum by ~1e-9 relative)
    assert beta_objective(x, w, h, 1.0) == pytest.approx(weighted_objective("kl", x, ones, w, h), rel=1e-8)
    om = log_uniform_weights(x.shape, seed=5).astype(np.float64)
    np.testing.assert_allclose(beta_w_step(x, w, h, 1.0, 0.0, om), weighted_w_step("kl", x, om, w, h), rtol=1e-12, atol=0)


def test_beta_2_is_the_oracles_euclidean_step_at_lambda_zero():
    x, w, h = case(2)                                    # (the guards sit in different places: 1e-7)
    w1 = beta_w_step(x, w, h, 2.0)
    np.testing.assert_allclose(w1, R.mur_w_step("eu", x, w, h, w @ h, 0.0), rtol=1e-7, atol=0)
    np.testing.assert_allclose(beta_h_step(x, w1, h, 2.0), R.mur_h_step("eu", x, w1, h, w1 @ h, 0.0), rtol=1e-7, atol=0)
    assert beta_objective(x, w, h, 2.0) == pytest.approx(float(R.objective(x, w @ h, "eu")), rel=1e-7)


@pytest.mark.parametrize("beta", [0.5, 0.9, 1.0, 1.5, 2.0, 2.5, 3.0])
def test_a_zero_is_data_for_positive_beta(beta):
    q = np.array([0.3, 1.0, 7.5])
    np.testing.assert_allclose(beta_cells(np.zeros(3), q, beta), q ** beta / beta, rtol=1e-15, atol=0)


def test_the_limit_forms_are_the_limits():
    rs = np.random.RandomState(3)
    x, q = rs.uniform(0.05, 2.0, 500), rs.uniform(0.05, 2.0, 500)
    for b in (0.0, 1.0):
        lim, near = float(np.sum(beta_cells(x, q, b))), float(np.sum(beta_cells(x, q, b + 1e-6)))
        assert abs(near - lim) / lim < 1e-5


# every beta plain and with log-uniform weights carrying 30 % zeros; every beta > 0 (where a zero is data) with 30 % zeros in x
MONOTONE = [(b, v) for b in GRID for v in ("plain", "weights", "zeros") if v != "zeros" or b > 0]


@pytest.mark.parametrize("beta,variant", MONOTONE)
def test_no_half_step_increases_the_objective(beta, variant):
    """The MM rule at lambda = 0, guard included: each half-step on its own, no slack."""
    rng = np.random.RandomState(0)
    x = rng.uniform(0.1, 2.0, (60, 40))
    w, h = rng.uniform(0.1, 1.0, (60, 5)), rng.uniform(0.1, 1.0, (5, 40))
    om = None
    if variant == "weights":
        om = log_uniform_weights(x.shape, seed=1).astype(np.float64)
    if variant == "zeros":
        x[rng.rand(*x.shape) < 0.3] = 0.0
    obj = [beta_objective(x, w, h, beta, om)]
    for _ in range(50):
        w = beta_w_step(x, w, h, beta, 0.0, om)
        mid = beta_objective(x, w, h, beta, om)
        h = beta_h_step(x, w, h, beta, 0.0, om)
        obj.append(beta_objective(x, w, h, beta, om))
        assert obj[-1] <= mid <= obj[-2], (beta, variant, len(obj))
    assert np.all(np.isfinite(obj)) and obj[-1] < obj[0]


def test_loop_matches_its_steps_and_the_stop_rule():
    rng = np.random.RandomState(3)
    x = rng.uniform(0.1, 2.0, (30, 20))
    np.random.seed(5)
    out = beta_mur(x, 4, 0.5, min_iter=2, max_iter=400, tol1=1e-5, tol2=1e-2)
    assert out.trace["stop_rule"] == 2 and out.i > 3 and len(out.obj_history) == out.i + 2
    assert out.obj_history[-1] >= out.obj_history[-2] - 1e-2 and out.obj_history[-2] < out.obj_history[-3] - 1e-2
    np.random.seed(5)
    w, h = R.start_factors(x, 4, (False, "zero"))
    assert out.obj_history[0] == beta_objective(x, w, h, 0.5)
    w = beta_w_step(x, w, h, 0.5)
    h = beta_h_step(x, w, h, 0.5)
    assert out.obj_history[1] == beta_objective(x, w, h, 0.5)


# ---- the host objective ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", GRID)
def test_weighted_objective_beta(beta):
    from nmf_amd import weighted
    x, w, h = case(4)
    if beta > 0:
        x[2, 3] = 0.0
    om = log_uniform_weights(x.shape, seed=6).astype(np.float64)
    xn = np.where(om > 0, x, np.nan)                     # unscored values are never read
    assert weighted.objective(xn, w, h, om, "beta", beta=beta) == pytest.approx(beta_objective(x, w, h, beta, om), rel=1e-13)
    held = (om == 0).astype(np.float64)                  # scoring held-out cells
    assert weighted.objective(x, w, h, held, "beta", beta=beta) == pytest.approx(beta_objective(x, w, h, beta, held), rel=1e-13)


def test_weighted_objective_beta_refusals():
    from nmf_amd import weighted
    x, w, h = case(4)
    ones = np.ones(x.shape)
    with pytest.raises(ValueError, match="beta"):
        weighted.objective(x, w, h, ones, "beta")
    with pytest.raises(ValueError, match="beta"):
        weighted.objective(x, w, h, ones, "beta", beta=4.0)
    with pytest.raises(ValueError, match="beta"):
        weighted.objective(x, w, h, ones, "kl", beta=1.0)
    x[1, 1] = 0.0
    with pytest.raises(ValueError, match="strictly positive"):
        weighted.objective(x, w, h, ones, "beta", beta=-0.5)
    assert np.isfinite(weighted.objective(x, w, h, ones, "beta", beta=0.5))


# ---- validation before any device work -------------------------------------------------------------------------------------
def data():
    return np.random.RandomState(0).uniform(0.1, 1.0, (20, 10))


@pytest.mark.parametrize("bad", [None, float("nan"), float("inf"), -1.5, 3.5, "x"])
def test_beta_is_required_finite_and_in_range(bad, no_library):
    from nmf_amd import NMF
    x = data()
    with pytest.raises(ValueError, match="beta"):
        _mur(x, 3, distance_type="beta", beta=bad, max_iter=2)
    with pytest.raises(ValueError, match="beta"):
        NMF(x, 3).factorize("mur", distance_type="beta", beta=bad, max_iter=2)
    with pytest.raises(ValueError, match="beta"):
        _mur(x, 3, distance_type="beta", beta=bad, weights=np.ones(x.shape), max_iter=2)


def test_beta_is_keyword_only_and_defaults_to_none():
    import inspect
    from nmf_amd.mur import mur
    p = inspect.signature(mur).parameters["beta"]
    assert p.kind is p.KEYWORD_ONLY and p.default is None


@pytest.mark.parametrize("kind", ["eu", "kl", "is"])
def test_beta_is_refused_with_every_other_distance(kind, no_library):
    x = data()
    with pytest.raises(ValueError, match="beta"):
        _mur(x, 3, distance_type=kind, beta=1.0, max_iter=2)
    with pytest.raises(ValueError, match="beta"):
        _mur(x, 3, distance_type=kind, beta=1.0, weights=np.ones(x.shape), max_iter=2)
    with pytest.raises(KeyError):                        # (an unknown distance still raises the old KeyError first)
        _mur(x, 3, distance_type="xx", beta=1.0)


@pytest.mark.parametrize("beta", [-1.0, 0.0, 0.5, 3.0])
def test_valid_requests_reach_the_library(beta, no_library):
    """Accepted input: the first thing that fails is the missing device."""
    x = data()
    keep = x.copy()
    for kw in (dict(), dict(weights=np.ones(x.shape)), dict(weights=(x > 0.3))):
        with pytest.raises(AssertionError, match="library was touched"):
            _mur(x, 3, distance_type="beta", beta=beta, max_iter=2, **kw)
    with pytest.raises(AssertionError, match="library was touched"):
        _mur(x, 128, distance_type="beta", beta=beta, max_iter=2)
    np.testing.assert_array_equal(x, keep)


@pytest.mark.parametrize("case_", ["zero", "negative", "nan", "tiny", "huge", "inf"])
@pytest.mark.parametrize("beta", [-0.5, 0.0, 0.5, 2.0])
def test_unweighted_values(case_, beta, no_library):
    """_check_is_input's value rules, with "> 0" relaxed to ">= 0" for beta > 0; never lifted."""
    x = data()
    x[2, 3] = {"zero": 0.0, "negative": -0.5, "nan": np.nan, "tiny": 1e-50, "huge": 1e39, "inf": np.inf}[case_]
    keep = x.copy()
    if case_ == "zero" and beta > 0:
        with pytest.raises(AssertionError, match="library was touched"):
            _mur(x, 3, distance_type="beta", beta=beta, max_iter=2)
    else:
        with pytest.raises(ValueError, match="beta"):
            _mur(x, 3, distance_type="beta", beta=beta, max_iter=2)
    np.testing.assert_array_equal(x, keep)               # no in-place lift


def test_a_tiny_value_beside_a_zero_is_still_refused(no_library):
    x = data()
    x[0, 0], x[1, 1] = 0.0, 1e-50
    with pytest.raises(ValueError, match="float32"):
        _mur(x, 3, distance_type="beta", beta=0.5, max_iter=2)


@pytest.mark.parametrize("case_", ["zero", "negative", "nan", "tiny", "huge"])
@pytest.mark.parametrize("beta", [-0.5, 0.5])
def test_weighted_values(case_, beta, no_library):
    """weighted.prepare's rules on the cells under positive weight, with the same beta-dependent positivity rule."""
    x = data()
    x[2, 3] = {"zero": 0.0, "negative": -0.5, "nan": np.nan, "tiny": 1e-50, "huge": 1e39}[case_]
    om = np.ones(x.shape)
    if case_ == "zero" and beta > 0:
        with pytest.raises(AssertionError, match="library was touched"):
            _mur(x, 3, distance_type="beta", beta=beta, weights=om, max_iter=2)
    else:
        with pytest.raises(ValueError):
            _mur(x, 3, distance_type="beta", beta=beta, weights=om, max_iter=2)
    om[2, 3] = 0.0                                       # ... unless the cell carries no weight: only the engine is missing
    with pytest.raises(AssertionError, match="library was touched"):
        _mur(x, 3, distance_type="beta", beta=beta, weights=om, max_iter=2)


def test_weighted_rules_of_today_hold(no_library):
    x = data()
    om = np.ones(x.shape)
    with pytest.raises(ValueError, match="engine="):
        _mur(x, 3, distance_type="beta", beta=0.5, weights=om, engine=object(), max_iter=2)
    with pytest.raises(ValueError, match="128"):
        _mur(np.ones((200, 150)), 129, distance_type="beta", beta=0.5, weights=np.ones((200, 150)), max_iter=2)
    with pytest.raises(ValueError, match="negative"):
        _mur(x, 3, distance_type="beta", beta=0.5, weights=-om, max_iter=2)


def test_mask_sparse_and_large_k_are_refused_naming_beta(no_library):
    x = data()
    m = x > 0.3
    with pytest.raises(ValueError, match=r"beta.*weights="):
        _mur(x, 3, distance_type="beta", beta=0.5, mask=m, max_iter=2)
    with pytest.raises(ValueError, match=r"beta.*weights="):
        _mur(x, 3, distance_type="beta", beta=0.5, mask=m, weights=np.ones(x.shape), max_iter=2)
    xs = sp.random(30, 20, density=0.3, format="csr", random_state=0)
    keep = xs.copy()
    with pytest.raises(ValueError, match=r"beta.*sparse"):
        _mur(xs, 3, distance_type="beta", beta=1.5, max_iter=2)
    assert (xs != keep).nnz == 0
    with pytest.raises(ValueError, match=r"beta.*k <= 128"):
        _mur(np.ones((200, 150)), 129, distance_type="beta", beta=0.5, max_iter=2)


def test_other_entry_points_refuse_beta(no_library, monkeypatch):
    """TypeError, ValueError or the old KeyError: whichever the same call gives for 'is' today."""
    from nmf_amd import dist as nd
    from nmf_amd.admm import admm
    from nmf_amd.anls import anls
    from nmf_amd.ao_admm import ao_admm
    from nmf_amd.grid import factorize_grid
    from nmf_amd.mur import mur_pair
    x = data()
    with pytest.raises(ValueError, match="mur only"):
        anls(x, 3, distance_type="beta")
    with pytest.raises(TypeError):
        anls(x, 3, beta=0.5)
    for solver in (admm, ao_admm):
        with pytest.raises(KeyError):
            solver(x, 3, distance_type="beta")
        with pytest.raises(TypeError):
            solver(x, 3, beta=0.5)
    with pytest.raises(TypeError):                       # mur_pair is Euclidean by construction
        mur_pair(x, 3, [{}, {}], distance_type="beta")
    with pytest.raises(TypeError):
        mur_pair(x, 3, [{}, {}], beta=0.5)
    for method in ("anls", "admm", "ao_admm"):
        with pytest.raises(ValueError, match="mur only"):
            factorize_grid(x, method, features=(2,), distance_type="beta", beta=0.5)

    def joined(*a, **kw):
        raise AssertionError("dist.factorize joined a process group before refusing 'beta'")

    monkeypatch.setattr(nd, "init_process_group", joined)
    with pytest.raises(TypeError, match="beta"):
        nd.factorize(x, 3, method="mur", backend="gloo", distance_type="beta", beta=0.5)
    with pytest.raises(TypeError, match="beta"):
        nd.factorize(x, 3, method="mur", backend="gloo", beta=0.5)


def test_grid_takes_the_sequential_path_validates_once_and_never_lifts(no_library):
    from nmf_amd import grid
    assert not grid._pairable("mur", dict(distance_type="beta", beta=0.5))
    x = data()
    x[1, 1] = -0.25
    keep = x.copy()
    with pytest.raises(ValueError, match="beta"):
        grid.factorize_grid(x, "mur", features=(2,), distance_type="beta", beta=0.5, max_iter=2)
    np.testing.assert_array_equal(x, keep)
    with pytest.raises(ValueError, match="beta"):        # beta= without 'beta': refused before the lift of the 'kl' grid
        grid.factorize_grid(x, "mur", features=(2,), distance_type="kl", beta=0.5, max_iter=2)
    np.testing.assert_array_equal(x, keep)
    with pytest.raises(ValueError, match="beta"):
        grid.factorize_grid(data(), "mur", features=(2,), distance_type="beta", max_iter=2)
    with pytest.raises(ValueError, match="k <= 128"):
        grid.factorize_grid(np.ones((200, 150)), "mur", features=(2, 129), distance_type="beta", beta=0.5, max_iter=2)
    with pytest.raises(AssertionError, match="library was touched"):
        grid.factorize_grid(data(), "mur", features=(2,), distance_type="beta", beta=0.5, max_iter=2)


def test_experiment_carries_beta_only_for_beta_runs():
    """Results.experiment: one extra trailing field for 'beta', exactly today's tuple otherwise."""
    from nmf_amd import mur as M
    assert M.Experiment._fields == ("method", "components", "distance_type", "nndsvd_init", "max_iter", "tol1", "tol2",
                                    "lambda_w", "lambda_h")
    assert M.BetaExperiment._fields == M.Experiment._fields + ("beta",)


def test_save_name_carries_beta(tmp_path):
    from nmf_amd import NMF
    from nmf_amd._driver import Results
    from nmf_amd.mur import BetaExperiment
    holder = NMF(np.ones((4, 3)), 2)
    exp = BetaExperiment("mur", 2, "beta", (False, "zero"), 1, 1e-5, 1e-5, 0.0, 0.5, 1.5)
    holder.results = Results(w=np.ones((4, 2)), h=np.ones((2, 3)), i=0, obj_history=[1.0, 0.5], experiment=exp)
    holder.save_factorization(save_dir=str(tmp_path))
    assert os.listdir(tmp_path) == ["nmf_mur_2_beta_0.0_0.5_random.npz"]
    assert exp[-1] == 1.5 and exp._asdict()["beta"] == 1.5


def test_abi_names_beta():
    from nmf_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "nmfx.h")).read()
    assert re.search(r"NMFX_BETA\s*=\s*3\b", text) and L.BETA == 3 and (L.EU, L.KL, L.IS) == (0, 1, 2)
    assert re.search(r"int\s+nmfx_set_beta\s*\(\s*nmfx_handle_t\s+\w+\s*,\s*double\s+\w+\s*\)", text)
    assert "nmfx_set_beta" in L.SIGNATURES
    lib = L.load()
    assert lib.nmfx_version() >= 350 and hasattr(lib, "nmfx_set_beta")
