"""nmf_amd.hals.hals_masked on the device: determinism, the monotone objective of exact coordinate descent, the recorded objective
against nmf_amd.masked.objective, the launch counts, the ABI's refusals, the NMF front end, and what makes the solver worth
having (at or below 200 iterations of masked MUR within 60 of its own, from the same start).  Single half-steps, problem by
problem: tests/test_gpu_hals_masked_step.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import masked_hals_step as MH

pytestmark = pytest.mark.gpu

NO_NNDSVD = (False, "zero")
K = 16


@functools.lru_cache(maxsize=None)
def case():
    """900 x 500, a rank-8 signal with noise, 4 % observed plus a long row (7) and a long column (2); 5 % of the observed values
    are exact zeros; NaN outside the mask.  (x float32, mask bool), read-only."""
    rng = np.random.RandomState(9)
    m, n = 900, 500
    v = rng.uniform(0, 1, (m, 8)) @ rng.uniform(0, 1, (8, n)) * (1 + 0.1 * rng.randn(m, n))
    mask = rng.rand(m, n) < 0.04
    mask[7, :] = True
    mask[:, 2] = True
    v[rng.rand(m, n) < 0.05] = 0.0
    x = np.where(mask, np.abs(v), np.nan).astype(np.float32)
    x.setflags(write=False)
    mask.setflags(write=False)
    assert mask[7].sum() > MH.CHUNK and mask[:, 2].sum() > MH.CHUNK
    return x, mask


def objective(w, h):
    from nmf_amd import masked
    x, mask = case()
    return masked.objective(x, w, h, mask)


def seeded_start(seed=1):
    x, _ = case()
    rng = np.random.RandomState(seed)
    return MH.A.f32(rng.uniform(0.05, 0.5, (x.shape[0], K))), MH.A.f32(rng.uniform(0.05, 0.5, (K, x.shape[1])))      # (what the device holds)


def masked_engine(k=K):
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    x, mask = case()
    return Engine.for_sparse(masked.observed(x, mask, k), k, masked=True)


# ---- the public call -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def public_runs():
    """Two runs of 25 iterations from the same seed, lambda = 0 (shared by the tests below, never modified)."""
    from nmf_amd.hals import hals_masked
    x, mask = case()
    keep = x.copy(), mask.copy()
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(hals_masked(x, K, mask, min_iter=25, max_iter=25, nndsvd_init=NO_NNDSVD))
    assert np.array_equal(x, keep[0], equal_nan=True) and np.array_equal(mask, keep[1])
    return out


def test_two_runs_bit_identical():
    a, b = public_runs()
    assert np.array_equal(a.w, b.w) and np.array_equal(a.h, b.h)
    assert np.array_equal(np.asarray(a.obj_history), np.asarray(b.obj_history))


def test_history_is_non_increasing_and_its_end_is_the_objective_of_the_result():
    """Exact coordinate descent cannot increase the objective; the float32 rounding of an iterate moves 1/2 Sum (x - wh)^2 by a
    few 1e-7 of itself at most, hence the 1e-6 (the allowance of tests/test_gpu_hals_sparse.py)."""
    res = public_runs()[0]
    obj = np.asarray(res.obj_history)
    assert len(obj) == 26 and res.i == 24
    up = obj[1:] / obj[:-1] - 1
    print(f"history {obj[0]:.4f} -> {obj[-1]:.4f}; largest step up {up.max():.2e}")
    assert (obj[1:] <= obj[:-1] * (1 + 1e-6)).all(), f"iteration {int(np.argmax(up))}: {up.max():.2e}"
    assert obj[-1] < 0.5 * obj[0]
    want = objective(res.w, res.h)
    assert abs(obj[-1] - want) <= 1e-9 * want, (obj[-1], want)
    assert (res.w >= 0).all() and (res.h >= 0).all()
    exp = res.experiment
    assert (exp.method, exp.components, exp.sweeps, exp.distance_type, exp.lambda_w, exp.lambda_h) == ("hals", K, 1, "eu", 0, 0)


def test_rescale_start_is_the_masked_alpha():
    from nmf_amd.hals import hals_masked
    x, mask = case()
    np.random.seed(1)
    hals_masked(x, K, mask, max_iter=1, nndsvd_init=NO_NNDSVD)
    np.random.seed(1)
    w0, h0 = np.random.rand(x.shape[0], K), np.random.rand(K, x.shape[1])
    q = (MH.A.f32(w0) @ MH.A.f32(h0))[mask]
    want = float(x[mask].astype(np.float64) @ q) / float(q @ q)
    print(f"alpha {hals_masked.last_alpha!r}, float64 on the host {want!r}")
    assert abs(hals_masked.last_alpha - want) <= 1e-6 * want
    np.random.seed(1)
    hals_masked(x, K, mask, max_iter=1, rescale_start=False, nndsvd_init=NO_NNDSVD)
    assert hals_masked.last_alpha is None


# ---- worth having ----------------------------------------------------------------------------------------------------------------
def test_at_or_below_200_masked_mur_iterations_within_60(monkeypatch):
    """From the same seeded |randn| start (rescaled for HALS), lambda = 0."""
    from nmf_amd import hals as H
    from nmf_amd.mur import mur
    x, mask = case()
    np.random.seed(3)
    slow = mur(x, K, mask=mask, distance_type="eu", min_iter=200, max_iter=200, nndsvd_init=NO_NNDSVD)
    draw = H.utils.initial_factors
    monkeypatch.setattr(H.utils, "initial_factors", lambda xs, k, init, uniform=False, defer_device=False: draw(xs, k, init, uniform=False))
    np.random.seed(3)
    fast = H.hals_masked(x, K, mask, min_iter=60, max_iter=60, nndsvd_init=NO_NNDSVD)
    target = slow.obj_history[-1]
    assert len(slow.obj_history) == 201 and len(fast.obj_history) == 61
    reached = np.nonzero(np.asarray(fast.obj_history) <= target)[0]
    print(f"masked mur after 200 iterations {target:.4f}; hals_masked after 60 {fast.obj_history[-1]:.4f}, first at or below after "
          f"{int(reached[0]) if len(reached) else None} iterations")
    assert len(reached), (target, fast.obj_history[-1])


# ---- launches --------------------------------------------------------------------------------------------------------------------
def profile(eng, name):
    ms, n = C.c_double(), C.c_int64()
    rc = eng.lib.nmfx_profile_get(eng.h, name.encode(), C.byref(ms), C.byref(n))
    return n.value if rc == 0 else 0


def test_launch_sites_per_iteration():
    """nmfx_profile_get: one W phase and one H phase scope per iteration; no stats pass, no unmasked HALS phase and no MUR phase."""
    iters = 7
    names = ("sp_mhals_wphase", "sp_mhals_hphase", "sp_stats", "sp_hals_wphase", "sp_hals_hphase", "sp_wphase", "sp_hphase")
    with masked_engine() as eng:
        eng.set_factors(*seeded_start())
        eng._ck(eng.lib.nmfx_profile_enable(eng.h, 1))
        eng.hals_masked_run(0, 0, 1, MH.NEVER, 0, 0, 0, 3)
        eng.hals_masked_run(0, 0, 1, MH.NEVER, 0, 0, 3, iters - 3)
        eng.hals_masked_finish(MH.NEVER, 0, 0, iters)
        eng.synchronize()
        counts = {name: profile(eng, name) for name in names}
        assert eng.state()[2] == iters + 1
    assert counts == {"sp_mhals_wphase": iters, "sp_mhals_hphase": iters, "sp_stats": 0, "sp_hals_wphase": 0, "sp_hals_hphase": 0,
                      "sp_wphase": 0, "sp_hphase": 0}, counts


def test_finish_records_nothing_twice_and_a_stopped_handle_stays():
    w0, h0 = seeded_start()
    with masked_engine() as eng:
        eng.set_factors(w0, h0)
        eng.hals_masked_finish(10, 1e-3, 1e-3, 0)        # nothing has run: obj[0] of the start
        assert eng.state() == (0, -1, 1)
        assert abs(eng.objectives(0, 1)[0] - objective(w0, h0)) <= 1e-9 * objective(w0, h0)
        eng.set_factors(w0, h0)
        eng.hals_masked_run(0, 0, 1, 2, 0.0, 1e30, 0, 8)         # tol2 = 1e30: rule 2 fires at the first tested index, 3
        assert eng.state() == (2, 3, 5)
        pair = eng.get_factors()
        eng.hals_masked_finish(2, 0.0, 1e30, 8)
        eng.hals_masked_run(0, 0, 1, 2, 0.0, 1e30, 8, 2)         # the flag is up: every launch returns at once
        assert eng.state() == (2, 3, 5)
        again = eng.get_factors()
        assert np.array_equal(pair[0], again[0]) and np.array_equal(pair[1], again[1])
        want = objective(*pair)
        assert abs(eng.objectives(4, 1)[0] - want) <= 1e-9 * want


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_refusals():
    from nmf_amd import _lib as L
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    lib = L.load()
    assert lib.nmfx_version() >= 392
    x, mask = case()
    T = (10, 1e-3, 1e-3)

    def refused(eng, word, *args, finish=True):
        before = eng.state()
        assert lib.nmfx_hals_masked_run(eng.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h), (args, lib.nmfx_last_error(eng.h))
        if finish:
            assert lib.nmfx_hals_masked_finish(eng.h, *T, 0) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h)
        assert eng.state() == before                    # nothing recorded

    w0, h0 = seeded_start()
    with Engine.for_sparse(masked.observed(x, mask, K), K) as eng:          # the same entries on an unmasked handle
        eng.set_factors(w0, h0)
        refused(eng, b"masked handle", 0.0, 0.0, 1, *T, 0, 1)
    with Engine(64, 48, 8) as eng:
        eng.upload_v(np.random.RandomState(0).rand(64, 48))
        eng.set_factors(np.random.RandomState(1).rand(64, 8), np.random.RandomState(2).rand(8, 48))
        refused(eng, b"sparse handle", 0.0, 0.0, 1, *T, 0, 1)
    with masked_engine(65) as eng:                      # kp = 128
        eng.set_factors(np.random.RandomState(1).rand(900, 65), np.random.RandomState(2).rand(65, 500))
        refused(eng, b"64", 0.0, 0.0, 1, *T, 0, 1)
    with masked_engine() as eng:
        eng.set_factors(w0, h0)
        for args, word in (((0.0, 0.0, 0, *T, 0, 1), b"sweeps"), ((0.0, 0.0, 17, *T, 0, 1), b"sweeps"), ((0.0, 0.0, 1, *T, -1, 1), b"range"),
                           ((0.0, 0.0, 1, *T, 0, -1), b"range"), ((-1.0, 0.0, 1, *T, 0, 1), b"lambda"), ((0.0, float("nan"), 1, *T, 0, 1), b"lambda")):
            refused(eng, word, *args, finish=False)
        assert lib.nmfx_hals_masked_finish(eng.h, *T, -1) == L.NMFX_E_ARG and b"range" in lib.nmfx_last_error(eng.h)
        # the family rule: neither solver continues the other's run without nmfx_set_factors
        eng.hals_masked_run(0, 0, 1, *T, 0, 1)
        assert lib.nmfx_mur_run(eng.h, L.EU, 0.0, 0.0, *T, 1, 1) == L.NMFX_E_STATE and b"another solver" in lib.nmfx_last_error(eng.h)
        eng.set_factors(w0, h0)
        eng.mur_run(L.EU, 0.0, 0.0, *T, 0, 1)
        assert lib.nmfx_hals_masked_run(eng.h, 0.0, 0.0, 1, *T, 1, 1) == L.NMFX_E_STATE and b"another solver" in lib.nmfx_last_error(eng.h)
        # the unmasked entry points go on refusing a masked handle
        assert lib.nmfx_hals_sparse_run(eng.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"masked" in lib.nmfx_last_error(eng.h)
        assert lib.nmfx_hals_run(eng.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(eng.h)


# ---- the NMF front end -----------------------------------------------------------------------------------------------------------
def test_nmf_factorize_hals_with_a_mask():
    from nmf_amd.nmf import NMF
    x, mask = case()
    nmf = NMF(x, 8)
    nmf.factorize("hals", mask=mask, max_iter=12, sweeps=2, lambda_h=0.01)
    exp = nmf.results.experiment
    assert nmf.w.shape == (900, 8) and nmf.h.shape == (8, 500) and (exp.method, exp.distance_type, exp.sweeps) == ("hals", "eu", 2)
    assert len(nmf.results.obj_history) == nmf.results.i + 2
    want = objective(nmf.w, nmf.h)
    assert abs(nmf.results.obj_history[-1] - want) <= 1e-9 * want
