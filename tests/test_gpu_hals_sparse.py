"""nmf_amd.hals.hals_sparse on the device: the public call against the float64 host loop of the same definition and against
dense `hals` on x.toarray(), the monotone objective of exact coordinate descent, what makes the solver worth having (below
sparse MUR after 30 iterations from MUR's own start), the stop rule, determinism, the start scale, the launch counts, the ABI's
refusals and the NMF front end.  Single half-steps, problem by problem: tests/test_gpu_hals_sparse_step.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_hals_step as SH

pytestmark = pytest.mark.gpu

NO_NNDSVD = (False, "zero")


@functools.lru_cache(maxsize=None)
def case(k, density):
    """The 700 x 600 matrices of tests/test_gpu_sparse.py (dense row 3, dense column 11, two empty rows and columns), float32."""
    x = SH.sparse_case(700, 600, density, seed=k, dense_row=3, dense_col=11, empty_rows=(0, 350), empty_cols=(1, 599))
    return sp.csr_matrix(x, dtype=np.float32)


def uniform_start(x, k, seed):
    np.random.seed(seed)
    return np.random.rand(x.shape[0], k), np.random.rand(k, x.shape[1])


def host_alpha(x, w0, h0):
    """<X, W0 H0> / ||W0 H0||^2 in float64 of the float32 values the device holds."""
    w, h = SH.A.f32(w0), SH.A.f32(h0)
    return float(np.sum(sp.csr_matrix(x, dtype=np.float64).multiply(w @ h))) / float(np.sum((w.T @ w) * (h @ h.T)))


def scaled_start(x, k, seed):
    w0, h0 = uniform_start(x, k, seed)
    a = host_alpha(x, w0, h0)
    return SH.A.f32(w0 * math.sqrt(a)), SH.A.f32(h0 * math.sqrt(a))


# ---- the public call against the float64 loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,sweeps", [(8, 1), (40, 1), (40, 2)])
def test_public_call_matches_the_float64_loop(k, sweeps):
    """Same start (the seeded uniform draw, scaled by the float64 alpha), 5 iterations, lambda on both sides: the bars of
    tests/test_gpu_hals.py::test_public_call_matches_the_float64_loop.  The caller's matrix is left as it was."""
    from nmf_amd.hals import hals_sparse
    x = case(k, 0.03)
    lw, lh = 0.05, 0.02
    wr, hr, hist = SH.host_hals(x, *scaled_start(x, k, 5), lw, lh, sweeps, 5)
    keep = x.copy()
    np.random.seed(5)
    res = hals_sparse(x, k, sweeps=sweeps, lambda_w=lw, lambda_h=lh, max_iter=5, nndsvd_init=NO_NNDSVD)
    assert (x != keep).nnz == 0 and np.array_equal(x.data, keep.data) and np.array_equal(x.indices, keep.indices)
    assert res.i == 4 and len(res.obj_history) == res.i + 2
    assert (res.w >= 0).all() and (res.h >= 0).all()
    err = np.linalg.norm(res.w @ res.h - wr @ hr) / np.linalg.norm(x.data.astype(np.float64))
    print(f"k = {k}, sweeps = {sweeps}: WH error {err:.3e}, history rel {np.max(np.abs(np.asarray(res.obj_history) / hist - 1)):.3e}")
    assert err < 1e-4, err
    np.testing.assert_allclose(res.obj_history, hist, rtol=2e-4)
    exp = res.experiment
    assert (exp.method, exp.components, exp.sweeps, exp.distance_type, exp.lambda_w, exp.lambda_h) == ("hals", k, sweeps, "eu", lw, lh)


@pytest.mark.parametrize("fmt", ["csc_matrix", "coo_matrix", "csr_array"])
def test_any_sparse_format_gives_the_same_bits(fmt):
    from nmf_amd.hals import hals_sparse
    x = case(8, 0.03)
    out = []
    for xx in (x, getattr(sp, fmt)(x)):
        np.random.seed(5)
        out.append(hals_sparse(xx, 8, max_iter=3, nndsvd_init=NO_NNDSVD))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)


# ---- the same class as dense hals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rescale", [True, False])
def test_equal_in_class_with_dense_hals(rescale, monkeypatch):
    """hals(x.toarray()) on the exact-f32 kernels from the same seeded start: the same stop index, history length and history."""
    from nmf_amd.hals import hals, hals_sparse
    monkeypatch.setenv("NMFX_PRECISION", "f32")
    x = case(16, 0.02)
    kw = dict(min_iter=10, max_iter=25, lambda_w=0.01, lambda_h=0.01, rescale_start=rescale, nndsvd_init=NO_NNDSVD)
    np.random.seed(7)
    dense = hals(x.toarray().astype(np.float64), 16, **kw)
    np.random.seed(7)
    got = hals_sparse(x, 16, **kw)
    assert got.i == dense.i and len(got.obj_history) == len(dense.obj_history) == got.i + 2
    np.testing.assert_allclose(got.obj_history, dense.obj_history, rtol=2e-4)
    if rescale:
        assert abs(hals_sparse.last_alpha - hals.last_alpha) <= 1e-6 * abs(hals.last_alpha)


def test_nndsvd_start_is_the_default():
    """The default start is the sparse NNDSVD that mur uses; no draw from the global generator."""
    from nmf_amd.hals import hals_sparse
    x = case(8, 0.03)
    np.random.seed(3)
    want = np.random.rand(3)
    np.random.seed(3)
    res = hals_sparse(x, 8, max_iter=3)
    assert np.array_equal(np.random.rand(3), want)
    assert res.experiment.nndsvd_init == (True, "zero") and len(res.obj_history) == 4
    assert res.obj_history[-1] < res.obj_history[0]


# ---- exact coordinate descent cannot increase the objective ---------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 40, 100])
def test_objective_is_monotone(k):
    from nmf_amd.hals import hals_sparse
    np.random.seed(2)
    res = hals_sparse(case(k, 0.03), k, min_iter=40, max_iter=40, nndsvd_init=NO_NNDSVD)
    obj = np.asarray(res.obj_history)
    assert len(obj) == 41 and res.i == 39
    up = obj[1:] / obj[:-1] - 1
    assert (obj[1:] <= obj[:-1] * (1 + 1e-6)).all(), f"iteration {int(np.argmax(up))}: {up.max():.2e}"


# ---- worth having ----------------------------------------------------------------------------------------------------------------
def test_below_sparse_mur_after_30_iterations_from_murs_own_start(monkeypatch):
    """From the same seeded |randn| start (rescaled for HALS) on the k = 16 / 2 % matrix, 30 iterations each.  (In float64 on
    the host: 1422.4 against 1441.3.)"""
    from nmf_amd import hals as H
    from nmf_amd.mur import mur
    x = case(16, 0.02)
    kw = dict(min_iter=30, max_iter=30, nndsvd_init=NO_NNDSVD)
    np.random.seed(3)
    slow = mur(x, 16, distance_type="eu", **kw)
    draw = H.utils.initial_factors
    monkeypatch.setattr(H.utils, "initial_factors", lambda xs, k, init, uniform=False, defer_device=False: draw(xs, k, init, uniform=False))
    np.random.seed(3)
    fast = H.hals_sparse(x, 16, rescale_start=True, **kw)
    print(f"after 30 iterations: hals_sparse {fast.obj_history[-1]:.4f}, sparse mur {slow.obj_history[-1]:.4f}")
    assert len(fast.obj_history) == len(slow.obj_history) == 31
    assert fast.obj_history[-1] < slow.obj_history[-1]


# ---- the stop rule ---------------------------------------------------------------------------------------------------------------
def test_stop_rule_stops_where_the_float64_loop_stops():
    """tol2 sits between the float64 loop's decreases at two consecutive indices, a factor 2 from each (asserted), so float32
    iterates cannot move the stop: the device stops at the same i, the history has i + 2 entries and the returned pair is the
    one its last entry belongs to."""
    from nmf_amd.hals import hals_sparse
    k, min_iter, stop = 8, 0, 2
    x = case(k, 0.03)
    _, _, hist = SH.host_hals(x, *scaled_start(x, k, 6), 0.0, 0.0, 1, 12)
    dec = hist[:-1] - hist[1:]                          # dec[i]: the decrease iteration i brings (float64: 187, 86, 14, 6.0, ...)
    tol2 = math.sqrt(dec[stop - 1] * dec[stop])         # the rule is tested at i = 1, 2, ...: it must hold at 2 and not at 1
    assert dec[stop] * 2 <= tol2 and (dec[min_iter + 1:stop] >= 2 * tol2).all(), dec[:4]      # the precondition
    np.random.seed(6)
    res = hals_sparse(x, k, min_iter=min_iter, max_iter=12, tol1=1e-3, tol2=float(tol2), nndsvd_init=NO_NNDSVD)
    assert res.i == stop and len(res.obj_history) == res.i + 2, (res.i, stop, len(res.obj_history))
    want = SH.objective(x, res.w, res.h)
    assert abs(res.obj_history[-1] - want) <= 1e-9 * abs(want), (res.obj_history[-1], want)
    np.testing.assert_allclose(res.obj_history, hist[:stop + 2], rtol=2e-4)


def test_finish_records_nothing_twice_and_a_stopped_handle_stays():
    from nmf_amd.engine import Engine
    x = case(8, 0.03)
    w0, h0 = scaled_start(x, 8, 6)
    with Engine.for_sparse(x, 8) as eng:
        eng.set_factors(w0, h0)
        eng.hals_sparse_finish(10, 1e-3, 1e-3, 0)       # nothing has run: obj[0] of the start
        assert eng.state() == (0, -1, 1)
        assert abs(eng.objectives(0, 1)[0] - SH.objective(x, w0, h0)) <= 1e-9 * SH.objective(x, w0, h0)
        eng.set_factors(w0, h0)
        eng.hals_sparse_run(0, 0, 1, 2, 0.0, 1e30, 0, 8)        # tol2 = 1e30: rule 2 fires at the first tested index, 3
        rule, stop_i, n_obj = eng.state()
        assert (rule, stop_i, n_obj) == (2, 3, 5)
        pair = eng.get_factors()
        eng.hals_sparse_finish(2, 0.0, 1e30, 8)
        eng.hals_sparse_run(0, 0, 1, 2, 0.0, 1e30, 8, 2)
        assert eng.state() == (2, 3, 5)
        again = eng.get_factors()
        assert np.array_equal(pair[0], again[0]) and np.array_equal(pair[1], again[1])
        want = SH.objective(x, *pair)
        assert abs(eng.objectives(4, 1)[0] - want) <= 1e-9 * want


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_two_runs_bit_identical():
    from nmf_amd.hals import hals_sparse
    x = SH.sparse_case(900, 500, 0.03, seed=9, dense_row=7, dense_col=2)
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(hals_sparse(x, 24, min_iter=20, max_iter=20, nndsvd_init=NO_NNDSVD))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))


# ---- rescale_start ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 40, 100])
def test_alpha_is_the_float64_value(k):
    from nmf_amd.hals import hals_sparse
    x = case(k, 0.03)
    w0, h0 = uniform_start(x, k, 9)
    np.random.seed(9)
    hals_sparse(x, k, max_iter=1, nndsvd_init=NO_NNDSVD)
    want = host_alpha(x, w0, h0)
    print(f"k = {k}: alpha {hals_sparse.last_alpha!r}, float64 on the host {want!r}")
    assert abs(hals_sparse.last_alpha - want) <= 1e-6 * want
    np.random.seed(9)
    hals_sparse(x, k, max_iter=1, rescale_start=False, nndsvd_init=NO_NNDSVD)
    assert hals_sparse.last_alpha is None


# ---- launches --------------------------------------------------------------------------------------------------------------------
def profile(eng, name):
    ms, n = C.c_double(), C.c_int64()
    rc = eng.lib.nmfx_profile_get(eng.h, name.encode(), C.byref(ms), C.byref(n))
    return n.value if rc == 0 else 0


def test_two_passes_over_the_non_zeros_per_iteration():
    """nmfx_profile_get: one W phase and one H phase scope per iteration, two stats scopes, and no MUR phase scope at all (the
    objective of the start is the one objective-only pass)."""
    from nmf_amd.engine import Engine
    x = case(8, 0.03)
    w0, h0 = scaled_start(x, 8, 6)
    iters = 7
    with Engine.for_sparse(x, 8) as eng:
        eng.set_factors(w0, h0)
        eng._ck(eng.lib.nmfx_profile_enable(eng.h, 1))
        eng.hals_sparse_run(0, 0, 1, SH.NEVER, 0, 0, 0, 3)
        eng.hals_sparse_run(0, 0, 1, SH.NEVER, 0, 0, 3, iters - 3)
        eng.hals_sparse_finish(SH.NEVER, 0, 0, iters)
        eng.synchronize()
        counts = {name: profile(eng, name) for name in ("sp_hals_wphase", "sp_hals_hphase", "sp_stats", "sp_wphase", "sp_hphase")}
        assert eng.state()[2] == iters + 1
    assert counts == {"sp_hals_wphase": iters, "sp_hals_hphase": iters, "sp_stats": 2 * iters, "sp_wphase": 0, "sp_hphase": 0}, counts


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_refusals():
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    lib = L.load()
    assert lib.nmfx_version() >= 391
    x = case(8, 0.03)
    T = (10, 1e-3, 1e-3)

    def refused(eng, word, *args, finish=True):
        before = eng.state() if word != b"first" else None
        assert lib.nmfx_hals_sparse_run(eng.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h), (args, lib.nmfx_last_error(eng.h))
        if finish:
            assert lib.nmfx_hals_sparse_finish(eng.h, *T, 0) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h)
        if before is not None:
            assert eng.state() == before                # nothing recorded

    with Engine.for_sparse(x, 8, masked=True) as eng:
        eng.set_factors(*scaled_start(x, 8, 1))
        refused(eng, b"masked", 0.0, 0.0, 1, *T, 0, 1)
    with Engine(64, 48, 8) as eng:
        eng.upload_v(np.random.RandomState(0).rand(64, 48))
        eng.set_factors(np.random.RandomState(1).rand(64, 8), np.random.RandomState(2).rand(8, 48))
        refused(eng, b"sparse handle", 0.0, 0.0, 1, *T, 0, 1)
    with Engine.for_sparse(x, 129) as eng:              # kp = 256
        eng.set_factors(np.random.RandomState(1).rand(700, 129), np.random.RandomState(2).rand(129, 600))
        refused(eng, b"128", 0.0, 0.0, 1, *T, 0, 1)
    with Engine.for_sparse(x, 8) as eng:
        w0, h0 = scaled_start(x, 8, 1)
        eng.set_factors(w0, h0)
        for args, word in (((0.0, 0.0, 0, *T, 0, 1), b"sweeps"), ((0.0, 0.0, 17, *T, 0, 1), b"sweeps"), ((0.0, 0.0, 1, *T, -1, 1), b"range"),
                           ((0.0, 0.0, 1, *T, 0, -1), b"range"), ((-1.0, 0.0, 1, *T, 0, 1), b"lambda"), ((0.0, float("nan"), 1, *T, 0, 1), b"lambda")):
            refused(eng, word, *args, finish=False)
        assert lib.nmfx_hals_sparse_finish(eng.h, *T, -1) == L.NMFX_E_ARG and b"range" in lib.nmfx_last_error(eng.h)
        # the family rule of DESIGN.md 4.10: neither solver continues the other's run without nmfx_set_factors
        eng.hals_sparse_run(0, 0, 1, *T, 0, 1)
        assert lib.nmfx_mur_run(eng.h, L.EU, 0.0, 0.0, *T, 1, 1) == L.NMFX_E_STATE and b"another solver" in lib.nmfx_last_error(eng.h)
        eng.set_factors(w0, h0)
        eng.mur_run(L.EU, 0.0, 0.0, *T, 0, 1)
        assert lib.nmfx_hals_sparse_run(eng.h, 0.0, 0.0, 1, *T, 1, 1) == L.NMFX_E_STATE and b"another solver" in lib.nmfx_last_error(eng.h)
        assert lib.nmfx_hals_run(eng.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(eng.h)


# ---- the NMF front end -----------------------------------------------------------------------------------------------------------
def test_nmf_factorize_hals_on_sparse_data():
    from nmf_amd.nmf import NMF
    x = case(8, 0.03)
    keep = x.copy()
    nmf = NMF(sp.csc_matrix(x), 8)
    nmf.factorize("hals", max_iter=12, sweeps=2, lambda_h=0.01)
    exp = nmf.results.experiment
    assert nmf.w.shape == (700, 8) and nmf.h.shape == (8, 600) and (exp.method, exp.distance_type, exp.sweeps) == ("hals", "eu", 2)
    assert len(nmf.results.obj_history) == nmf.results.i + 2
    want = SH.objective(x, nmf.w, nmf.h)
    assert abs(nmf.results.obj_history[-1] - want) <= 1e-9 * want
    assert (x != keep).nnz == 0
