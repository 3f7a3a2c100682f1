"""Itakura-Saito MUR without a GPU: the float64 yardstick of tests/is_ref.py checked on its own, the host objective
(nmf_amd.masked.objective(..., 'is')), and everything mur / NMF / the grid / dist decide before the library is touched."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from is_ref import EPS, is_h_step, is_mur, is_objective, is_w_step


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


# ---- the float64 helper on its own -----------------------------------------------------------------------------------------
def test_helper_on_a_hand_worked_1x1_case():
    x, w, h = np.array([[2.0]]), np.array([[1.0]]), np.array([[1.0]])
    q = 1.0 + EPS
    assert is_objective(x, w, h) == pytest.approx(2.0 / q - np.log(2.0 / q) - 1.0, rel=1e-15)
    # W: sqrt((2 / q^2) / (1 / q)) = sqrt(2 / q); then H with q' = w1 + 1e-9: sqrt((w1 2 / q'^2) / (w1 / q')) = sqrt(2 / q')
    w1 = is_w_step(x, w, h)
    assert w1[0, 0] == pytest.approx(np.sqrt(2.0 / q), rel=1e-15)
    h1 = is_h_step(x, w1, h)
    assert h1[0, 0] == pytest.approx(np.sqrt(2.0 / (w1[0, 0] + EPS)), rel=1e-15)
    # lambda enters the denominator: sqrt((2 / q^2) / (1 / q + 1/2))
    assert is_w_step(x, w, h, 0.5)[0, 0] == pytest.approx(np.sqrt((2.0 / q ** 2) / (1.0 / q + 0.5)), rel=1e-15)
    # a cell outside the mask: nothing observed, zero denominator, 0
    none = np.zeros((1, 1), dtype=bool)
    assert is_w_step(x, w, h, 0.0, none)[0, 0] == 0.0 and is_objective(x, w, h, none) == 0.0


def test_helper_never_increases_the_objective():
    rng = np.random.RandomState(0)
    x = rng.uniform(0.1, 2.0, (60, 40))
    w, h = rng.uniform(0.1, 1.0, (60, 5)), rng.uniform(0.1, 1.0, (5, 40))
    obj = [is_objective(x, w, h)]
    for _ in range(50):
        w = is_w_step(x, w, h)
        mid = is_objective(x, w, h)
        h = is_h_step(x, w, h)
        obj.append(is_objective(x, w, h))
        assert obj[-1] <= mid <= obj[-2]                 # each half-step on its own, no slack
    assert obj[-1] < obj[0]                              # (a rank-5 fit of full-rank noise: it moves, it cannot go far)


def test_helper_with_a_mask_never_increases_the_masked_objective():
    rng = np.random.RandomState(1)
    x = rng.uniform(0.1, 2.0, (60, 40))
    m = rng.rand(60, 40) < 0.5
    xn = np.where(m, x, np.nan)
    w, h = rng.uniform(0.1, 1.0, (60, 5)), rng.uniform(0.1, 1.0, (5, 40))
    obj = [is_objective(xn, w, h, m)]
    for _ in range(50):
        w = is_w_step(xn, w, h, 0.0, m)
        h = is_h_step(xn, w, h, 0.0, m)
        obj.append(is_objective(xn, w, h, m))
    assert np.all(np.isfinite(obj)) and np.all(np.diff(obj) <= 0)


def test_helper_keeps_a_fixed_point():
    # V = W H with entries around 1e4: the guard 1e-9 in q moves the fixed point by 5e-10 / q, far below 1e-12
    rng = np.random.RandomState(2)
    w, h = rng.uniform(30, 60, (30, 5)), rng.uniform(30, 60, (5, 20))
    x = w @ h
    w1 = is_w_step(x, w, h)
    h1 = is_h_step(x, w1, h)
    np.testing.assert_allclose(w1, w, rtol=1e-12, atol=0)
    np.testing.assert_allclose(h1, h, rtol=1e-12, atol=0)
    assert abs(is_objective(x, w, h)) < 1e-12


def test_helper_loop_matches_its_steps_and_the_stop_rule():
    rng = np.random.RandomState(3)
    x = rng.uniform(0.1, 2.0, (30, 20))
    np.random.seed(5)
    out = is_mur(x, 4, min_iter=2, max_iter=400, tol1=1e-5, tol2=1e-2)
    assert out.trace["stop_rule"] == 2 and out.i > 3 and len(out.obj_history) == out.i + 2
    assert out.obj_history[-1] >= out.obj_history[-2] - 1e-2 and out.obj_history[-2] < out.obj_history[-3] - 1e-2


# ---- the host objective ----------------------------------------------------------------------------------------------------
def test_masked_objective_is():
    from nmf_amd import masked
    rng = np.random.RandomState(4)
    x = rng.uniform(0.1, 2.0, (50, 30))
    w, h = rng.uniform(0.1, 1.0, (50, 4)), rng.uniform(0.1, 1.0, (4, 30))
    full = np.ones(x.shape, dtype=bool)
    assert masked.objective(x, w, h, full, "is") == pytest.approx(is_objective(x, w, h), rel=1e-13)
    train = rng.rand(*x.shape) < 0.7
    held = ~train
    q = w @ h + EPS
    r = x / q
    cells = r - np.log(r) - 1.0
    assert masked.objective(x, w, h, held, "is") == pytest.approx(float(cells[held].sum()), rel=1e-13)
    assert masked.objective(x, w, h, held, "is", chunk=37) == pytest.approx(float(cells[held].sum()), rel=1e-13)
    assert masked.objective(x, w, h, train, "is") + masked.objective(x, w, h, held, "is") == pytest.approx(float(cells.sum()), rel=1e-13)
    xn = np.where(held, x, -1.0)                        # unobserved values are never read
    assert masked.objective(xn, w, h, held, "is") == pytest.approx(float(cells[held].sum()), rel=1e-13)
    x0 = x.copy()
    x0[3, 4] = 0.0
    with pytest.raises(ValueError, match="strictly positive"):
        masked.objective(x0, w, h, full, "is")
    with pytest.raises(KeyError):
        masked.objective(x, w, h, full, "xx")


# ---- validation before any device work -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["zero", "negative", "nan"])
def test_dense_input_must_be_strictly_positive(case, no_library):
    x = np.random.RandomState(0).uniform(0.1, 1.0, (20, 10))
    x[2, 3] = {"zero": 0.0, "negative": -0.5, "nan": np.nan}[case]
    keep = x.copy()
    with pytest.raises(ValueError, match="strictly positive"):
        _mur(x, 3, distance_type="is", max_iter=2)
    np.testing.assert_array_equal(x, keep)              # no in-place lift
    from nmf_amd import NMF
    with pytest.raises(ValueError, match="strictly positive"):
        NMF(x, 3).factorize("mur", distance_type="is", max_iter=2)
    np.testing.assert_array_equal(x, keep)


@pytest.mark.parametrize("bad,word", [(1e-50, "strictly positive"), (1e39, "float32 range"), (np.inf, "float32 range")])
def test_values_outside_the_float32_range_are_refused(bad, word, no_library):
    """The device holds float32: a positive float64 that underflows to 0 there would drop out of the fit silently."""
    x = np.random.RandomState(0).uniform(0.1, 1.0, (20, 10))
    x[4, 5] = bad
    with pytest.raises(ValueError, match=word):
        _mur(x, 3, distance_type="is", max_iter=2)
    m = np.ones(x.shape, dtype=bool)
    with pytest.raises(ValueError):
        _mur(x, 3, distance_type="is", mask=m, max_iter=2)
    m[4, 5] = False                                     # ... unless it is not observed: then only the engine is missing
    with pytest.raises(AssertionError, match="library was touched"):
        _mur(x, 3, distance_type="is", mask=m, max_iter=2)


def test_dense_k_above_128_is_refused(no_library):
    x = np.random.RandomState(0).uniform(0.1, 1.0, (200, 150))
    with pytest.raises(ValueError, match="k <= 128"):
        _mur(x, 129, distance_type="is", max_iter=2)


def test_sparse_input_without_a_mask_is_refused(no_library):
    x = sp.random(30, 20, density=0.3, format="csr", random_state=0)
    keep = x.copy()
    with pytest.raises(ValueError, match="mask="):
        _mur(x, 3, distance_type="is", max_iter=2)
    assert (x != keep).nnz == 0


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_masked_input_needs_positive_observed_entries(kind, no_library):
    rng = np.random.RandomState(1)
    x = rng.uniform(0.1, 1.0, (20, 10))
    m = rng.rand(20, 10) < 0.6
    m[2, 3] = True
    x[2, 3] = 0.0
    data = x if kind == "dense" else sp.csr_matrix(np.where(m, x, 0.0))
    keep_x, keep_m = x.copy(), m.copy()
    with pytest.raises(ValueError, match="strictly positive"):
        _mur(data, 3, distance_type="is", mask=m, max_iter=2)
    np.testing.assert_array_equal(x, keep_x)
    np.testing.assert_array_equal(m, keep_m)
    x[2, 3] = -1.0                                      # (the masked path's own check)
    with pytest.raises(ValueError):
        _mur(x, 3, distance_type="is", mask=m, max_iter=2)


def test_unobserved_values_are_not_validated(monkeypatch):
    """Zeros, negatives and NaN outside the mask pass: the first thing that fails is the missing device / the engine."""
    from nmf_amd import engine

    class Reached(Exception):
        pass

    def for_sparse(*a, **kw):
        raise Reached

    monkeypatch.setattr(engine.Engine, "for_sparse", classmethod(lambda cls, *a, **kw: for_sparse()))
    rng = np.random.RandomState(2)
    x = rng.uniform(0.1, 1.0, (20, 10))
    m = rng.rand(20, 10) < 0.6
    x[~m] = np.where(rng.rand((~m).sum()) < 0.5, 0.0, np.nan)
    with pytest.raises(Reached):
        _mur(x, 3, distance_type="is", mask=m, max_iter=2)


def test_other_entry_points_refuse_is(no_library, monkeypatch):
    from nmf_amd import dist as nd
    from nmf_amd.anls import anls
    from nmf_amd.grid import factorize_grid
    x = np.random.RandomState(0).uniform(0.1, 1.0, (20, 10))
    with pytest.raises(ValueError, match="mur only"):
        anls(x, 3, distance_type="is")
    with pytest.raises(ValueError, match="mur only"):
        factorize_grid(x, "anls", features=(2,), distance_type="is")
    with pytest.raises(TypeError):                      # mur_pair is Euclidean by construction: it has no distance_type
        from nmf_amd.mur import mur_pair
        mur_pair(x, 3, [{}, {}], distance_type="is")

    def joined(*a, **kw):
        raise AssertionError("dist.factorize joined a process group before refusing 'is'")

    monkeypatch.setattr(nd, "init_process_group", joined)
    with pytest.raises(TypeError, match="'is'"):
        nd.factorize(x, 3, method="mur", backend="gloo", distance_type="is")


def test_grid_takes_the_sequential_path_and_never_lifts(no_library):
    from nmf_amd import grid
    assert not grid._pairable("mur", dict(distance_type="is"))
    x = np.random.RandomState(0).uniform(0.1, 1.0, (20, 10))
    x[1, 1] = -0.25
    keep = x.copy()
    with pytest.raises(ValueError, match="strictly positive"):
        grid.factorize_grid(x, "mur", features=(2,), distance_type="is", max_iter=2)
    np.testing.assert_array_equal(x, keep)


def test_unknown_distance_still_raises_the_old_keyerror(no_library):
    x = np.random.RandomState(0).uniform(0.1, 1.0, (20, 10))
    for name in ("xx", "IS", "itakura"):
        with pytest.raises(KeyError) as info:
            _mur(x, 3, distance_type=name)
        assert info.value.args[0] == 'Distance type unknown: use "kl" or "eu"'


def test_save_name_carries_is(tmp_path):
    from nmf_amd import NMF
    from nmf_amd._driver import Results
    from nmf_amd.mur import Experiment
    holder = NMF(np.ones((4, 3)), 2)
    holder.results = Results(w=np.ones((4, 2)), h=np.ones((2, 3)), i=0, obj_history=[1.0, 0.5],
                             experiment=Experiment("mur", 2, "is", (False, "zero"), 1, 1e-5, 1e-5, 0.0, 0.5))
    holder.save_factorization(save_dir=str(tmp_path))
    assert os.listdir(tmp_path) == ["nmf_mur_2_is_0.0_0.5_random.npz"]


def test_abi_names_is():
    from nmf_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "nmfx.h")).read()
    assert re.search(r"NMFX_IS\s*=\s*2\b", text) and L.IS == 2 and (L.EU, L.KL) == (0, 1)
    assert L.load().nmfx_version() >= 330
