"""The sparse MUR fold-in on the device (nmfx_sparse_foldin_run, nmf_amd.transform.transform_sparse), column by
column against the float64 definition of tests/sparse_transform_step.py at the bars and the slack proven in
tests/test_sparse_transform_bars.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_transform_step as T

pytestmark = pytest.mark.gpu

STOP = T.STOP


def _fail(fails):
    if fails:
        raise AssertionError("\n".join(fails))


@functools.lru_cache(maxsize=None)
def reference(c):
    return T.solve(c, **STOP)


def engine_for(c):
    """A fresh sparse handle on the case's x_new (masked on a masked case)."""
    from nmf_amd import masked, sparse
    from nmf_amd.engine import Engine
    p = T.problem(c)
    if c.handle == "sparse":
        return Engine.for_sparse(sparse.normalise(p.x, c.k), c.k)
    return Engine.for_sparse(masked.observed(p.x, p.mask, c.k), c.k, masked=True)


def case(handle, loss, k):
    return next(c for c in T.CASES if (c.handle, c.loss, c.k) == (handle, loss, k))


# ---- values and counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_fixed_step_counts_against_float64(c):
    """tol = 0 with max_iter = 1, 3, 25: every column against the float64 run of as many steps (a column that stopped earlier has
    reached an exact fixed point in f32 and would move nothing in the later steps)."""
    bar = T.bar_of(c, "fixed")
    fails, worst = [], 0.0
    for steps in T.FIXED_STEPS:
        res = T.run_device(c, 0.0, steps)
        assert res.h.dtype == np.float64 and res.h.shape == (c.k, T.N)
        assert res.iters.dtype == np.int32 and res.iters.shape == (T.N,) and (res.iters >= 1).all() and (res.iters <= steps).all()
        assert tuple(res.experiment) == ("transform_sparse", c.k, c.loss, 0.0, steps, c.lam)
        ref = T.solve(c, 0.0, steps, counts=np.full(T.N, steps))
        w, msgs = T.value_failures(c, res.h, ref.h, bar, f"{steps} steps")
        worst = max(worst, w)
        fails += msgs
    print(f"{T.case_id(c)}: fixed counts, worst deviation {worst:.3e} (bar {bar:.1e})")
    _fail(fails)


@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_stop_rule(c):
    """tol = 1e-3, max_iter = 400: every column's count is one the float64 trajectory accepts (within the slack), at most
    LIMIT(n) columns have another count than the float64 run, and the values are those of the float64 run at the device's counts."""
    res = T.run_device(c, **STOP)
    fails, at = T.count_failures(c, res.iters, STOP["tol"], STOP["max_iter"], T.SLACK, ref=reference(c))
    off = int((res.iters != reference(c).counts).sum())
    print(f"{T.case_id(c)}: steps min {res.iters.min()} mean {res.iters.mean():.0f} max {res.iters.max()}; {off} columns off the float64 count")
    if at is not None:
        bar = T.bar_of(c, "stop")
        worst, msgs = T.value_failures(c, res.h, at.h, bar, "stop")
        print(f"{T.case_id(c)}: stop run, worst deviation {worst:.3e} (bar {bar:.1e})")
        fails += msgs
    _fail(fails)


# ---- the recorded objectives ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_recorded_objectives_are_f64_grade(c):
    p = T.problem(c)
    res = T.run_device(c, **STOP)
    assert len(res.obj_history) == 2 and all(isinstance(v, np.float64) for v in res.obj_history)
    fails = []
    for i, h in enumerate((p.h0, res.h)):
        want, got = T.host_objective(c, h), float(res.obj_history[i])
        rel = abs(got - want) / max(abs(want), 1.0)
        print(f"{T.case_id(c)}: obj[{i}] = {got:.9e}, rel {rel:.3e}")
        if not rel <= T.OBJ_RTOL:
            fails.append(f"{T.case_id(c)} obj[{i}]: recorded {got!r}, float64 of the pair {want!r}: rel {rel:.3e} > {T.OBJ_RTOL:.0e}")
    _fail(fails)


# ---- determinism, the empty column ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", T.PAIRS, ids="-".join)
def test_two_runs_give_the_same_bits(pair):
    from nmf_amd.transform import transform_sparse
    for k in (5, 130):
        c = case(*pair, k)
        p = T.problem(c)
        first = T.run_device(c, **STOP)
        again = transform_sparse(p.x, p.w, p.mask, distance_type=c.loss, h0=p.h0, lambda_h=c.lam, **STOP)
        assert np.array_equal(first.h, again.h) and np.array_equal(first.iters, again.iters)
        assert np.array_equal(np.asarray(first.obj_history), np.asarray(again.obj_history))


@pytest.mark.parametrize("pair", T.PAIRS, ids="-".join)
def test_a_column_without_entries(pair):
    """a = 0: step 1 takes the column to exact zeros, step 2 moves nothing and stops it; under a cap of 1 the count is 1."""
    for k in (3, 40):
        c = case(*pair, k)
        assert T.problem(c).lens[0] == 0
        res = T.run_device(c, **STOP)
        assert res.iters[0] == 2 and not res.h[:, 0].any()
        one = T.run_device(c, 0.0, 1)
        assert one.iters[0] == 1 and not one.h[:, 0].any()


def test_the_default_start():
    """h0 left out: the constant sqrt(mean / k), no draw; the handle-level run from that start gives the same bits."""
    from nmf_amd import losses
    from nmf_amd.transform import transform_sparse
    for c in (case("sparse", "kl", 5), case("masked", "eu", 17)):
        p = T.problem(c)
        np.random.seed(5)
        want = np.random.rand(3)
        np.random.seed(5)
        res = transform_sparse(p.x, p.w, p.mask, distance_type=c.loss, lambda_h=c.lam, tol=1e-3, max_iter=50)
        assert np.array_equal(np.random.rand(3), want)
        total = float(p.xv.sum())
        mean = total / (T.M * T.N) if c.handle == "sparse" else total / int(p.lens.sum())
        with engine_for(c) as eng:
            eng.set_factors(p.w, np.full((c.k, T.N), np.sqrt(mean / c.k)))
            eng.sparse_foldin_run(losses.CODES[c.loss], c.lam, 1e-3, 50)
            assert np.array_equal(eng.get_factors()[1], res.h) and np.array_equal(eng.sparse_foldin_iters(), res.iters)


# ---- state and the C refusals -----------------------------------------------------------------------------------------------------
def test_state_of_the_counts():
    from nmf_amd import _lib as L
    from nmf_amd import losses
    lib = L.load()
    assert lib.nmfx_version() >= 395
    out = np.zeros(T.N, dtype=np.int32)
    ptr = out.ctypes.data_as(C.c_void_p)
    for c in (case("sparse", "eu", 16), case("masked", "kl", 5)):
        p = T.problem(c)
        with engine_for(c) as eng:
            eng.set_factors(p.w, p.h0)
            assert lib.nmfx_sparse_foldin_get_iters(eng.h, ptr) == L.NMFX_E_STATE             # before a run
            assert b"nmfx_sparse_foldin_get_iters" in lib.nmfx_last_error(eng.h)
            eng.sparse_foldin_run(losses.CODES[c.loss], c.lam, 1e-3, 10)
            w, _ = eng.get_factors()
            assert np.array_equal(w, p.w), "W was touched"
            iters = eng.sparse_foldin_iters()
            assert iters.dtype == np.int32 and iters.shape == (T.N,) and (iters >= 1).all() and (iters <= 10).all()
            assert eng.state()[2] == 2                                                          # two objectives recorded
            assert lib.nmfx_hals_foldin_get_sweeps(eng.h, ptr) == L.NMFX_E_STATE              # the HALS getter knows nothing of it
            eng.set_factors(p.w, p.h0)                                                          # new factors: the counts are gone
            assert lib.nmfx_sparse_foldin_get_iters(eng.h, ptr) == L.NMFX_E_STATE
            eng.sparse_foldin_run(losses.CODES[c.loss], c.lam, 1e-3, 10)
            assert np.array_equal(eng.sparse_foldin_iters(), iters)
    c = case("sparse", "eu", 16)                                                               # ... and the other way round
    p = T.problem(c)
    with engine_for(c) as eng:
        eng.set_factors(p.w, p.h0)
        eng.hals_foldin_run(0.0, 1e-3, 5)
        assert lib.nmfx_hals_foldin_get_sweeps(eng.h, ptr) == L.NMFX_OK
        assert lib.nmfx_sparse_foldin_get_iters(eng.h, ptr) == L.NMFX_E_STATE


def test_abi_refusals_launch_nothing():
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    lib = L.load()
    out = np.zeros(T.N, dtype=np.int32)
    ptr = out.ctypes.data_as(C.c_void_p)

    def refused(eng, word, *args):
        before = eng.state()
        assert lib.nmfx_sparse_foldin_run(eng.h, *args) == L.NMFX_E_ARG, (args, lib.nmfx_last_error(eng.h))
        text = lib.nmfx_last_error(eng.h)
        assert b"nmfx_sparse_foldin_run" in text and word in text, (args, text)
        assert eng.state() == before
        assert lib.nmfx_sparse_foldin_get_iters(eng.h, ptr) == L.NMFX_E_STATE

    with Engine(64, 48, 8) as eng:
        eng.upload_v(np.random.RandomState(0).rand(64, 48))
        eng.set_factors(np.random.RandomState(1).rand(64, 8), np.random.RandomState(2).rand(8, 48))
        refused(eng, b"sparse handle", L.KL, 0.0, 1e-4, 10)
    for c in (case("sparse", "kl", 16), case("masked", "is", 16)):
        p = T.problem(c)
        with engine_for(c) as eng:
            eng.set_factors(p.w, p.h0)
            if c.handle == "sparse":
                refused(eng, b"Itakura-Saito", L.IS, 0.0, 1e-4, 10)
            refused(eng, b"distance", L.BETA, 0.0, 1e-4, 10)
            refused(eng, b"distance", 77, 0.0, 1e-4, 10)
            for tol in (float("nan"), -1e-9, 1.0, float("inf")):
                refused(eng, b"tol", L.KL, 0.0, tol, 10)
            for cap in (0, -1, 10001):
                refused(eng, b"max_iter", L.KL, 0.0, 1e-4, cap)
            for lam in (-0.5, float("nan")):
                refused(eng, b"lambda", L.KL, lam, 1e-4, 10)
            assert np.array_equal(eng.get_factors()[1], p.h0)                                   # nothing moved
            assert lib.nmfx_foldin_run(eng.h, L.KL, 0.0, 0, 0.0, 0.0, 0, 1) == L.NMFX_E_ARG     # the dense fold-in keeps refusing sparse handles
            eng.sparse_foldin_run(L.KL, 0.0, 1e-4, 10)
            assert lib.nmfx_sparse_foldin_get_iters(eng.h, ptr) == L.NMFX_OK and (out >= 1).all() and (out <= 10).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _one_float64_step(x, mask, w, h, loss):
    """One step of the definition from h, in float64 from the f32 images (dense x; mask None: every cell is data)."""
    w, h = w.astype(np.float32).astype(np.float64), h.astype(np.float32).astype(np.float64)
    x = np.where(np.ones_like(x, bool) if mask is None else mask, x, 0.0).astype(np.float32).astype(np.float64)
    m = np.ones_like(x) if mask is None else mask.astype(np.float64)
    q = w @ h
    if loss == "kl":
        a = w.T @ (m * x / (q + 1e-9))
        d = w.T @ m
        return 2 * h * a / (d + np.sqrt(d * d))
    iq = 1.0 / (q + 1e-9)
    return h * np.sqrt((w.T @ (m * x * iq * iq)) / (w.T @ (m * iq)))


def test_fit_then_fold_in_end_to_end():
    """mur on sparse data under KL for 30 iterations, then NMF.transform_sparse of the same data from the fit's H, one step:
    one float64 step from the fit's H.  The same for a masked Itakura-Saito fit."""
    from nmf_amd import NMF
    rng = np.random.RandomState(12)
    dense = rng.uniform(0.2, 1.0, (60, 40)) * (rng.rand(60, 40) < 0.3)
    xs = sp.csr_matrix(dense)
    np.random.seed(3)
    nmf = NMF(xs, 6)
    nmf.factorize(method="mur", distance_type="kl", min_iter=30, max_iter=30)
    res = nmf.transform_sparse(xs, h0=nmf.h, tol=0, max_iter=1)
    assert res.experiment.distance_type == "kl" and (res.iters == 1).all()
    want = _one_float64_step(dense, None, nmf.w, nmf.h, "kl")
    dev = T.deviation(res.h, want)
    print(f"sparse kl end to end: worst deviation {dev.max():.3e}")
    # one f32 step: a column sums at most 60 terms (60 x 2^-24 = 3.6e-6 of the sum at the very worst) and the epilogue adds a
    # handful of roundings: 1e-5 is about twice that bound
    assert dev.max() <= 1e-5

    mask = rng.rand(60, 40) < 0.4
    pos = np.where(mask, rng.uniform(0.2, 1.0, (60, 40)), np.nan)
    np.random.seed(4)
    nmf = NMF(pos, 6)
    nmf.factorize(method="mur", distance_type="is", mask=mask, min_iter=30, max_iter=30)
    res = nmf.transform_sparse(pos, mask, h0=nmf.h, tol=0, max_iter=1)
    assert res.experiment.distance_type == "is" and (res.iters == 1).all()
    want = _one_float64_step(np.nan_to_num(pos), mask, nmf.w, nmf.h, "is")
    dev = T.deviation(res.h, want)
    print(f"masked is end to end: worst deviation {dev.max():.3e}")
    assert dev.max() <= 1e-5
