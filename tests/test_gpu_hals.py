"""nmf_amd.hals.hals on the device: the public call against a float64 host loop of the same definition, the monotone objective
of exact coordinate descent, the start scale, what makes the solver worth having (fewer iterations than MUR from MUR's own
start), and the NMF front end.  Single half-steps, problem by problem: tests/test_gpu_hals_step.py."""
import functools
import math
import os

import numpy as np
import pytest

import anls_step as A
import hals_step as HS

pytestmark = pytest.mark.gpu

M, N = 257, 200


@functools.lru_cache(maxsize=None)
def planted(k):
    v = A.planted(M, N, k, seed=1, noise=0.02, jitter=0.05)[0]
    v.setflags(write=False)
    return v


def host_alpha(v, w0, h0):
    """<V, W0 H0> / ||W0 H0||^2 in float64 of the float32 values the device holds."""
    wh = A.f32(w0) @ A.f32(h0)
    return float(np.vdot(np.asarray(v, np.float64), wh) / np.vdot(wh, wh))


def host_hals(v, w, h, lw, lh, sweeps, iters):
    """The float64 loop: (W, H, objective history of iters + 1 entries)."""
    v = np.asarray(v, np.float64)
    vt = np.ascontiguousarray(v.T)
    hist = [0.5 * np.sum((v - w @ h) ** 2)]
    for _ in range(iters):
        g, r = A.gram_rhs(np.ascontiguousarray(h.T), vt, lw)
        w = HS.sweep(g, r, w.T, sweeps)[0].T
        g, r = A.gram_rhs(w, v, lh)
        h = HS.sweep(g, r, h, sweeps)[0]
        hist.append(0.5 * np.sum((v - w @ h) ** 2))
    return w, h, np.array(hist)


def uniform_start(k, seed):
    np.random.seed(seed)
    return np.random.rand(M, k), np.random.rand(k, N)


# ---- the public call against the float64 loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,sweeps", [(8, 1), (40, 1), (40, 2)])
def test_public_call_matches_the_float64_loop(k, sweeps):
    """Same start (the seeded uniform draw, scaled by the float64 alpha), 5 iterations, lambda on both sides: the final product
    within the bar of the trajectory check of tests/test_gpu_anls.py, 1e-4 of ||V||."""
    from nmf_amd.hals import hals
    v = planted(k)
    lw, lh = 0.05, 0.02
    w0, h0 = uniform_start(k, 5)
    a = host_alpha(v, w0, h0)
    wr, hr, hist = host_hals(v, A.f32(w0 * math.sqrt(a)), A.f32(h0 * math.sqrt(a)), lw, lh, sweeps, 5)
    np.random.seed(5)
    keep = v.copy()
    res = hals(v, k, sweeps=sweeps, lambda_w=lw, lambda_h=lh, max_iter=5, nndsvd_init=(False, "zero"))
    assert np.array_equal(v, keep)
    assert res.i == 4 and len(res.obj_history) == res.i + 2
    assert (res.w >= 0).all() and (res.h >= 0).all()
    err = np.linalg.norm(res.w @ res.h - wr @ hr) / np.linalg.norm(v.astype(np.float64))
    print(f"k = {k}, sweeps = {sweeps}: WH error {err:.3e}")
    assert err < 1e-4, err
    np.testing.assert_allclose(res.obj_history, hist, rtol=2e-4)
    exp = res.experiment
    assert (exp.method, exp.components, exp.sweeps, exp.distance_type, exp.lambda_w) == ("hals", k, sweeps, "eu", lw)


def test_kl_only_selects_the_reported_objective():
    from nmf_amd.hals import hals
    v = planted(8)
    out = {}
    for kind in ("eu", "kl"):
        np.random.seed(5)
        out[kind] = hals(v, 8, distance_type=kind, max_iter=4, nndsvd_init=(False, "zero"))
    assert np.array_equal(out["eu"].w, out["kl"].w) and np.array_equal(out["eu"].h, out["kl"].h)
    want = HS.objective("kl", v, out["kl"].w, out["kl"].h)
    assert abs(out["kl"].obj_history[-1] - want) <= HS.OBJ_RTOL * abs(want)


# ---- exact coordinate descent cannot increase the objective ---------------------------------------------------------------------
@pytest.mark.parametrize("k,sweeps", [(8, 1), (40, 1), (100, 1), (40, 3)])
def test_objective_is_monotone(k, sweeps):
    from nmf_amd.hals import hals
    np.random.seed(2)
    res = hals(planted(k), k, sweeps=sweeps, min_iter=40, max_iter=40, nndsvd_init=(False, "zero"))
    obj = np.asarray(res.obj_history)
    assert len(obj) == 41 and res.i == 39
    up = obj[1:] / obj[:-1] - 1
    assert (obj[1:] <= obj[:-1] * (1 + 1e-6)).all(), f"iteration {int(np.argmax(up))}: {up.max():.2e}"


# ---- worth having ----------------------------------------------------------------------------------------------------------------
def test_below_mur_after_30_iterations_from_murs_own_start(monkeypatch):
    """From the same seeded |randn| start on the planted matrix, 30 iterations each.  (In float64 on the host: 0.77 against 7.8.)"""
    from nmf_amd import hals as H
    from nmf_amd.mur import mur
    v = A.planted(M, N, 40, seed=1, noise=0.02, jitter=0.05)[0]
    kw = dict(min_iter=30, max_iter=30, nndsvd_init=(False, "zero"))
    np.random.seed(3)
    slow = mur(v, 40, distance_type="eu", **kw)
    draw = H.utils.initial_factors
    monkeypatch.setattr(H.utils, "initial_factors", lambda x, k, init, uniform=False, defer_device=False: draw(x, k, init, uniform=False, defer_device=defer_device))
    np.random.seed(3)
    fast = H.hals(v, 40, rescale_start=True, **kw)
    print(f"after 30 iterations: hals {fast.obj_history[-1]:.4f}, mur {slow.obj_history[-1]:.4f}")
    assert len(fast.obj_history) == len(slow.obj_history) == 31
    assert fast.obj_history[-1] < slow.obj_history[-1]


# ---- rescale_start ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 40, 100])
def test_alpha_is_the_float64_value(k):
    from nmf_amd.hals import hals
    v = planted(k)
    w0, h0 = uniform_start(k, 9)
    np.random.seed(9)
    hals(v, k, max_iter=1, nndsvd_init=(False, "zero"))
    want = host_alpha(v, w0, h0)
    print(f"k = {k}: alpha {hals.last_alpha!r}, float64 on the host {want!r}")
    assert abs(hals.last_alpha - want) <= 1e-6 * want


def test_a_zero_start_is_not_rescaled():
    from nmf_amd.engine import Engine
    from nmf_amd.hals import start_scale
    v = planted(8)
    with Engine(M, N, 8) as eng:
        eng.upload_v(v)
        assert start_scale(eng, np.zeros((M, 8)), np.ones((8, N))) is None


def test_without_rescale_the_start_is_bit_exact():
    """rescale_start=False: one iteration of the public call is one iteration of the engine from the seeded draw itself."""
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    from nmf_amd.hals import hals
    v = planted(40)
    w0, h0 = uniform_start(40, 4)
    np.random.seed(4)
    res = hals(v, 40, rescale_start=False, max_iter=1, nndsvd_init=(False, "zero"))
    assert hals.last_alpha is None
    with Engine(M, N, 40) as eng:
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        eng.anls_set_distance(L.EU)
        eng.hals_run(0, 0, 1, 10, 1e-3, 1e-3, 0, 1)
        w, h = eng.get_factors()
    assert np.array_equal(res.w, w) and np.array_equal(res.h, h)
    np.random.seed(4)
    scaled = hals(v, 40, rescale_start=True, max_iter=1, nndsvd_init=(False, "zero"))
    assert not np.array_equal(scaled.w, w)


# ---- the NMF front end -----------------------------------------------------------------------------------------------------------
def test_nmf_factorize_hals(tmp_path):
    from nmf_amd.nmf import NMF
    v = planted(8)
    nmf = NMF(v, 8)
    nmf.factorize("hals", max_iter=12, sweeps=2, lambda_h=0.01)
    assert nmf.w.shape == (M, 8) and nmf.h.shape == (8, N) and nmf.results.experiment.method == "hals"
    nmf.save_factorization(save_dir=str(tmp_path))
    files = os.listdir(tmp_path)
    assert len(files) == 1 and files[0].startswith("nmf_hals_8_eu_") and files[0].endswith(".npz")
    out = nmf.transform(v[:, :50].copy(), max_iter=20)
    assert out.h.shape == (8, 50) and (out.h >= 0).all()


def test_abi():
    from nmf_amd import _lib as L
    lib = L.load()
    assert lib.nmfx_version() >= 380 and hasattr(lib, "nmfx_hals_run")
