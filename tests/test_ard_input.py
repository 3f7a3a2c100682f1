"""Automatic relevance determination without a GPU: the float64 yardstick of tests/ard_ref.py checked on its own (no half-step
and no lambda-step increases C; it recovers a planted rank), the host side of nmf_amd.ard (objective, default b, relevance,
effective rank) and everything mur_ard decides before the library is touched."""
import inspect
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from ard_cases import GAP, RANK, kept_and_gap, rank_reference
from ard_ref import (ard_c, ard_default_b, ard_h_step, ard_k_eff, ard_lambda, ard_mur, ard_objective, ard_relevance,
                     ard_w_step)
from beta_ref import beta_h_step, beta_objective, beta_w_step
from conftest import ROOT
from oracle import nmf_ref as R
from weighted_cases import log_uniform_weights

GRID = (-1.0, -0.5, 0.0, 0.5, 0.9, 1.0, 1.5, 2.0, 2.5, 3.0)


@pytest.fixture
def no_library(monkeypatch):
    """Any use of libnmfx fails the test: validation has to come first."""
    from nmf_amd import _lib

    def touched(*a, **kw):
        raise AssertionError("the library was touched before the input was validated")

    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(_lib, "require_gpu", touched)


def _ard(*a, **kw):
    from nmf_amd.ard import mur_ard
    return mur_ard(*a, **kw)


def data():
    return np.random.RandomState(0).uniform(0.1, 1.0, (20, 10))


# ---- the float64 yardstick on its own --------------------------------------------------------------------------------------
def test_hand_worked_1x1_case():
    x, w, h = np.array([[2.0]]), np.array([[1.0]]), np.array([[1.0]])
    a, b, phi = 3.0, 0.5, 0.25
    c = 1 + 1 + a + 1
    assert ard_c(x.shape, a) == c
    lam = ard_lambda(w, h, a, b)
    assert lam[0] == (1.0 + 1.0 + b) / c
    q = 1.0 + 1e-9
    # beta = 1: gamma = 1, W <- (2 / q) / (1 + phi / lambda)
    w1 = ard_w_step(x, w, h, lam, 1.0, phi)
    assert w1[0, 0] == pytest.approx((2.0 / q) / (1.0 + phi / lam[0]), rel=1e-15)
    q1 = w1[0, 0] + 1e-9
    assert ard_h_step(x, w1, h, lam, 1.0, phi)[0, 0] == pytest.approx((w1[0, 0] * 2.0 / q1) / (w1[0, 0] + phi / lam[0]), rel=1e-15)
    fit = 2.0 * np.log(2.0 / q) - 2.0 + q
    assert ard_objective(x, w, h, lam, 1.0, phi, a, b) == pytest.approx(fit + phi * (c + c * np.log(lam[0])), rel=1e-15)


def test_lambda_is_the_minimiser_and_the_penalty_has_its_closed_form():
    rs = np.random.RandomState(1)
    x, w, h = rs.uniform(0.1, 1.0, (12, 9)), rs.uniform(0.1, 1.0, (12, 4)), rs.uniform(0.1, 1.0, (4, 9))
    a, b, phi = 5.0, 0.3, 0.7
    lam = ard_lambda(w, h, a, b)
    best = ard_objective(x, w, h, lam, 0.5, phi, a, b)
    c = ard_c(x.shape, a)
    assert best == pytest.approx(beta_objective(x, w, h, 0.5) + phi * c * float(np.sum(1.0 + np.log(lam))), rel=1e-14)
    for k in range(4):
        for f in (0.9, 1.1):
            other = lam.copy()
            other[k] *= f
            assert ard_objective(x, w, h, other, 0.5, phi, a, b) > best
    # an infinite lambda switches the penalty of the steps off
    big = np.full(4, np.inf)
    np.testing.assert_array_equal(ard_w_step(x, w, h, big, 0.5, phi), beta_w_step(x, w, h, 0.5))
    np.testing.assert_array_equal(ard_h_step(x, w, h, big, 0.5, phi), beta_h_step(x, w, h, 0.5))
    # ... and a finite one is the per-component lambda_w of the beta step
    col = ard_w_step(x, w, h, lam, 0.5, phi)
    for k in range(4):
        np.testing.assert_allclose(col[:, k], beta_w_step(x, w, h, 0.5, phi / lam[k])[:, k], rtol=1e-14, atol=0)


# every beta plain and with log-uniform weights carrying 30 % zeros; every beta > 0 (where a zero is data) with 30 % zeros in x
MONOTONE = [(b, v) for b in GRID for v in ("plain", "weights", "zeros") if v != "zeros" or b > 0]


@pytest.mark.parametrize("beta,variant", MONOTONE)
def test_no_half_step_and_no_lambda_step_increases_the_objective(beta, variant):
    """60 x 45, K = 8: each W step, each H step and each lambda step on its own, Delta C <= 1e-12 |C|."""
    rng = np.random.RandomState(0)
    x = rng.uniform(0.1, 2.0, (60, 45))
    w, h = rng.uniform(0.1, 1.0, (60, 8)), rng.uniform(0.1, 1.0, (8, 45))
    om = None
    if variant == "weights":
        om = log_uniform_weights(x.shape, seed=1).astype(np.float64)
    if variant == "zeros":
        x[rng.rand(*x.shape) < 0.3] = 0.0
    phi, a = 0.5, 5.0
    b = ard_default_b(x, 8, a, om)
    lam = ard_lambda(w, h, a, b)
    cur = first = ard_objective(x, w, h, lam, beta, phi, a, b, om)
    worst = -np.inf
    for _ in range(100):
        for step in ("w", "h", "lambda"):
            if step == "w":
                w = ard_w_step(x, w, h, lam, beta, phi, om)
            elif step == "h":
                h = ard_h_step(x, w, h, lam, beta, phi, om)
            else:
                lam = ard_lambda(w, h, a, b)
            new = ard_objective(x, w, h, lam, beta, phi, a, b, om)
            worst = max(worst, (new - cur) / abs(cur))
            assert new - cur <= 1e-12 * abs(cur), (beta, variant, step, new - cur, cur)
            cur = new
    assert np.isfinite(cur) and cur < first
    print(f"beta={beta} {variant}: largest relative increase {worst:.2e}")


def test_loop_matches_its_steps_and_the_stop_rule():
    rng = np.random.RandomState(3)
    x = rng.uniform(0.1, 2.0, (30, 20))
    a, b, phi = 5.0, 0.4, 0.2
    np.random.seed(5)
    out = ard_mur(x, 4, 0.5, phi, a, b, min_iter=2, max_iter=400, tol1=-np.inf, tol2=1e-2)
    assert out.trace["stop_rule"] == 2 and out.i > 3 and len(out.obj_history) == out.i + 2
    assert out.obj_history[-1] >= out.obj_history[-2] - 1e-2 and out.obj_history[-2] < out.obj_history[-3] - 1e-2
    np.random.seed(5)
    w, h = R.start_factors(x, 4, (False, "zero"))
    lam = ard_lambda(w, h, a, b)
    assert out.obj_history[0] == ard_objective(x, w, h, lam, 0.5, phi, a, b)
    w = ard_w_step(x, w, h, lam, 0.5, phi)
    h = ard_h_step(x, w, h, lam, 0.5, phi)                 # the same lambda for both half-steps
    assert out.obj_history[1] == ard_objective(x, w, h, ard_lambda(w, h, a, b), 0.5, phi, a, b)
    np.testing.assert_array_equal(out.trace["lam"], ard_lambda(out.w, out.h, a, b))


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("beta", [1.0, 1.5])
def test_the_yardstick_recovers_the_planted_rank(beta, seed):
    x, b, out, rel = rank_reference(beta, seed)
    kept, gap = kept_and_gap(rel)
    print(f"beta={beta} seed={seed}: relevances {np.sort(rel)[::-1]}, gap {gap:.3g}")
    assert ard_k_eff(rel) == RANK["rank"]
    assert gap > GAP                                       # the count cannot hinge on rounding
    assert min(rel[kept]) > 10 and len(out.obj_history) == RANK["iters"] + 1


# ---- the host side of nmf_amd.ard ------------------------------------------------------------------------------------------
def test_default_b():
    from nmf_amd import ard
    x = data()
    assert ard.default_b(x, 4, 5.0) == pytest.approx(np.sqrt(4.0 * 3.0 * x.mean() / 4), rel=1e-15)
    assert ard.default_b(x, 4, 5.0) == pytest.approx(ard_default_b(x, 4, 5.0), rel=1e-15)
    om = log_uniform_weights(x.shape, seed=2).astype(np.float64)
    xn = np.where(om > 0, x, np.nan)                       # never read where the weight is 0
    want = np.sqrt(3.0 * 2.0 * (np.sum(om * x) / np.sum(om)) / 7)
    assert ard.default_b(xn, 7, 4.0, om) == pytest.approx(want, rel=1e-14)
    for a in (2.0, 1.5):
        with pytest.raises(ValueError, match="a > 2"):
            ard.default_b(x, 4, a)


def test_relevance_and_effective_rank_on_hand_made_lambdas():
    from nmf_amd import ard
    shape, a, b = (10, 5), 4.0, 2.0                        # c = 20, floor 0.1
    lam = np.array([0.1, 0.3, 10.1, 0.1 + 1e-3, 5.1])
    rel = ard.relevance(lam, shape, a, b)
    np.testing.assert_allclose(rel, [0.0, 2.0, 100.0, 1e-2, 50.0], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(rel, ard_relevance(lam, shape, a, b), rtol=1e-15, atol=0)
    assert ard.effective_rank(rel) == 3                    # > 1e-3 x 100: 2, 100, 50
    assert ard.effective_rank(rel, 1e-5) == 4 and ard.effective_rank(rel, 0.6) == 1 and ard.effective_rank(rel, 0.4) == 2
    assert ard.effective_rank(rel, 1e-3) == ard_k_eff(rel, 1e-3)
    assert ard.effective_rank(np.zeros(4)) == 0            # everything at the floor
    assert inspect.signature(ard.mur_ard).parameters["prune_tol"].default == 1e-3


@pytest.mark.parametrize("beta", GRID)
def test_host_objective(beta):
    from nmf_amd import ard
    rs = np.random.RandomState(4)
    x, w, h = rs.uniform(0.05, 1.0, (40, 30)), rs.uniform(0.1, 1.0, (40, 4)), rs.uniform(0.1, 1.0, (4, 30))
    if beta > 0:
        x[2, 3] = 0.0
    lam = rs.uniform(0.5, 2.0, 4)                          # any lambda, not only the minimiser
    a, b, phi = 5.0, 0.3, 0.7
    assert ard.objective(x, w, h, lam, beta, phi, a, b) == pytest.approx(ard_objective(x, w, h, lam, beta, phi, a, b), rel=1e-13)
    om = log_uniform_weights(x.shape, seed=6).astype(np.float64)
    xn = np.where(om > 0, x, np.nan)
    assert ard.objective(xn, w, h, lam, beta, phi, a, b, weights=om) == pytest.approx(
        ard_objective(x, w, h, lam, beta, phi, a, b, om), rel=1e-13)


# ---- validation before any device work -------------------------------------------------------------------------------------
def test_signature():
    from nmf_amd import ard
    import nmf_amd
    assert nmf_amd.ard is ard and "ard" in nmf_amd.__all__
    p = inspect.signature(ard.mur_ard).parameters
    assert list(p)[:2] == ["x", "k"] and all(q.kind is q.KEYWORD_ONLY for name, q in p.items() if name not in ("x", "k"))
    assert p["a"].default == 5.0 and p["b"].default is None and p["weights"].default is None
    assert p["min_iter"].default == 100 and p["max_iter"].default == 100000 and p["tol1"].default == p["tol2"].default == 1e-5
    for absent in ("lambda_w", "lambda_h", "mask", "engine"):
        assert absent not in p
    assert ard.ArdResults._fields == ("w", "h", "i", "obj_history", "experiment", "relevance", "k_eff")
    from nmf_amd.mur import BetaExperiment
    assert ard.ArdExperiment._fields == BetaExperiment._fields + ("phi", "a", "b")


@pytest.mark.parametrize("bad", [None, float("nan"), float("inf"), -1.5, 3.5, "x"])
def test_beta_is_required_finite_and_in_range(bad, no_library):
    x = data()
    with pytest.raises(ValueError, match="beta"):
        _ard(x, 3, beta=bad, phi=0.1, max_iter=2)
    with pytest.raises(ValueError, match="beta"):
        _ard(x, 3, beta=bad, phi=0.1, weights=np.ones(x.shape), max_iter=2)


# (b=None is the default, not a refusal)
@pytest.mark.parametrize("name,bad", [(name, bad) for name in ("phi", "a", "b")
                                      for bad in (None, float("nan"), float("inf"), 0.0, -0.1, "x") if (name, bad) != ("b", None)])
def test_phi_a_b_are_finite_and_positive(name, bad, no_library):
    x = data()
    kw = dict(beta=0.5, phi=0.1, a=5.0, b=0.2, max_iter=2)
    kw[name] = bad
    with pytest.raises(ValueError, match=name):
        _ard(x, 3, **kw)


@pytest.mark.parametrize("a", [2.0, 1.0, 0.5])
def test_the_default_b_needs_a_above_two(a, no_library):
    x = data()
    with pytest.raises(ValueError, match="a > 2"):
        _ard(x, 3, beta=0.5, phi=0.1, a=a, max_iter=2)
    with pytest.raises(AssertionError, match="library was touched"):       # ... with a b of its own, a <= 2 is fine
        _ard(x, 3, beta=0.5, phi=0.1, a=a, b=0.3, max_iter=2)


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, float("nan"), "x"])
def test_prune_tol_lies_strictly_between_0_and_1(bad, no_library):
    with pytest.raises(ValueError, match="prune_tol"):
        _ard(data(), 3, beta=0.5, phi=0.1, prune_tol=bad, max_iter=2)


def test_sparse_and_large_k_are_refused(no_library):
    xs = sp.random(30, 20, density=0.3, format="csr", random_state=0)
    keep = xs.copy()
    with pytest.raises(ValueError, match="sparse"):
        _ard(xs, 3, beta=1.5, phi=0.1, max_iter=2)
    assert (xs != keep).nnz == 0
    with pytest.raises(ValueError, match="k <= 128"):
        _ard(np.ones((200, 150)), 129, beta=0.5, phi=0.1, max_iter=2)
    with pytest.raises(ValueError, match="128"):
        _ard(np.ones((200, 150)), 129, beta=0.5, phi=0.1, weights=np.ones((200, 150)), max_iter=2)
    for extra in (dict(lambda_w=0.1), dict(lambda_h=0.1), dict(mask=np.ones((20, 10))), dict(engine=object())):
        with pytest.raises(TypeError):
            _ard(data(), 3, beta=0.5, phi=0.1, **extra)


@pytest.mark.parametrize("case_", ["zero", "negative", "nan", "tiny", "huge", "inf"])
@pytest.mark.parametrize("beta", [-0.5, 0.5])
def test_values_follow_the_beta_rules_and_are_never_lifted(case_, beta, no_library):
    x = data()
    x[2, 3] = {"zero": 0.0, "negative": -0.5, "nan": np.nan, "tiny": 1e-50, "huge": 1e39, "inf": np.inf}[case_]
    keep = x.copy()
    for kw in (dict(), dict(weights=np.ones(x.shape))):
        if case_ == "zero" and beta > 0:
            with pytest.raises(AssertionError, match="library was touched"):
                _ard(x, 3, beta=beta, phi=0.1, max_iter=2, **kw)
        else:
            with pytest.raises(ValueError):
                _ard(x, 3, beta=beta, phi=0.1, max_iter=2, **kw)
        np.testing.assert_array_equal(x, keep)
    om = np.ones(x.shape)
    om[2, 3] = 0.0                                         # the cell carries no weight: only the engine is missing
    if case_ != "inf":
        with pytest.raises(AssertionError, match="library was touched"):
            _ard(x, 3, beta=beta, phi=0.1, weights=om, max_iter=2)


@pytest.mark.parametrize("beta", [-1.0, 0.0, 1.0, 3.0])
def test_valid_requests_reach_the_library(beta, no_library):
    x = data()
    keep = x.copy()
    for kw in (dict(), dict(weights=np.ones(x.shape)), dict(weights=(x > 0.3)), dict(b=0.5, a=1.0), dict(prune_tol=0.5)):
        with pytest.raises(AssertionError, match="library was touched"):
            _ard(x, 3, beta=beta, phi=0.1, max_iter=2, **kw)
    with pytest.raises(AssertionError, match="library was touched"):
        _ard(x, 128, beta=beta, phi=0.1, max_iter=2)
    np.testing.assert_array_equal(x, keep)


def test_abi_names_ard():
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    text = open(os.path.join(ROOT, "include", "nmfx.h")).read()
    assert re.search(r"int\s+nmfx_set_ard\s*\(\s*nmfx_handle_t\s+\w+\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*,\s*double\s+\w+\s*\)", text)
    assert re.search(r"int\s+nmfx_clear_ard\s*\(\s*nmfx_handle_t\s+\w+\s*\)", text)
    assert re.search(r"int\s+nmfx_get_relevance\s*\(\s*nmfx_handle_t\s+\w+\s*,\s*double\s*\*", text)
    for name in ("nmfx_set_ard", "nmfx_clear_ard", "nmfx_get_relevance"):
        assert name in L.SIGNATURES
    lib = L.load()
    assert lib.nmfx_version() >= 360 and hasattr(lib, "nmfx_set_ard")
    for method in ("set_ard", "clear_ard", "relevance"):
        assert callable(getattr(Engine, method))
