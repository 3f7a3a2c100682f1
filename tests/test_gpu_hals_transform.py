"""The HALS fold-in on the device (nmfx_hals_foldin_run, nmf_amd.hals.hals_transform), problem by problem
against the float64 definition of tests/hals_transform_step.py at the bars and the slack proven in
tests/test_hals_transform_bars.py."""
import numpy as np
import pytest
import scipy.sparse as sp

import hals_transform_step as T
from mur_step import NEVER

pytestmark = pytest.mark.gpu

LONG, STOP = T.LONG, T.STOP


def _fail(fails):
    if fails:
        raise AssertionError("\n".join(fails))


# ---- 1: the solve at a fixed count is the H half-step, bit for bit --------------------------------------------------------------
STEP_CASES = [T.Case(kind, matrix, k, "scaled") for kind in ("sparse", "masked") for matrix in ("base", "rowsT")
              for k in (3, 40, 64) + ((128,) if kind == "sparse" else ())]


@pytest.mark.parametrize("c", STEP_CASES, ids=T.case_id)
def test_solve_at_a_fixed_count_is_the_h_half_step(c):
    """One iteration of hals_sparse_run / hals_masked_run with sweeps = s from (w0, h0) gives (w1, h1); the fold-in of (w1, h0)
    with tol = 0 and max_sweeps = s is h1, bit for bit (whole columns, pieces with their fix-up, and the long kernel)."""
    p = T.problem(c)
    assert p.nobs.max() > 2 * 256 and p.nobs.min() <= 1              # long columns and (nearly) empty ones
    lw = 0.05
    with T.engine_for(c) as eng:
        run = eng.hals_sparse_run if c.kind == "sparse" else eng.hals_masked_run
        for s in (1, 3, 16):
            eng.set_factors(p.w, p.h0)
            run(lw, p.lam, s, NEVER, 0, 0, 0, 1)
            w1, h1 = eng.get_factors()
            eng.set_factors(w1, p.h0)
            eng.hals_foldin_run(p.lam, 0.0, s)
            w, h = eng.get_factors()
            counts = eng.hals_foldin_sweeps()
            assert np.array_equal(w, w1), f"s = {s}: W was touched"
            assert np.array_equal(h, h1), f"s = {s}: {int((h != h1).any(axis=0).sum())} of {h.shape[1]} columns differ from the H half-step"
            assert counts.dtype == np.int32 and counts.shape == (h.shape[1],) and (counts >= 1).all() and (counts <= s).all()


# ---- 2: beyond the refresh ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_forty_sweeps_against_float64(c):
    """tol = 0, max_sweeps = 40: every problem against the float64 sweep of 40 (a problem that stopped earlier moved nothing in
    its last sweep, and would move nothing in the later ones)."""
    p = T.problem(c)
    run = T.run_foldin(c, **LONG)
    ref = T.solve(p.g, p.r, p.h0, 0.0, LONG["max_sweeps"], counts=np.full(p.r.shape[1], LONG["max_sweeps"]))
    bar = T.bar_of(c, "long")
    worst, msg = T.deviation(c, run.h, ref, bar, f"{T.case_id(c)} long", record=True)
    print(f"{T.case_id(c)}: worst deviation {worst:.3e} (bar {bar:.1e}); sweeps min {run.sweeps.min()} max {run.sweeps.max()}")
    assert (run.sweeps >= 1).all() and (run.sweeps <= LONG["max_sweeps"]).all()
    _fail([msg] if msg else [])


# ---- 3: the stop rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_stop_rule(c):
    """tol = 1e-3, max_sweeps = 8: on the float64 sweep run for the device's own counts every problem stopped where the rule
    says (within the slack) and not before; the values are compared as in test 2."""
    run = T.run_foldin(c, **STOP)
    fails, ref = T.stop_failures(c, run.sweeps, STOP["tol"], STOP["max_sweeps"], T.SLACK)
    print(f"{T.case_id(c)}: sweeps 1..8 -> {np.bincount(run.sweeps, minlength=9)[1:].tolist()}")
    if ref is not None:
        bar = T.bar_of(c, "stop")
        worst, msg = T.deviation(c, run.h, ref, bar, f"{T.case_id(c)} stop", record=True)
        print(f"{T.case_id(c)}: worst deviation {worst:.3e} (bar {bar:.1e})")
        if msg:
            fails.append(msg)
    _fail(fails)


# ---- 4: the recorded objectives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_recorded_objectives_are_f64_grade(c):
    p = T.problem(c)
    run = T.run_foldin(c, **STOP)
    scale = 1e-2 * 0.5 * float(np.sum(p.vv)) if c.kind == "sparse" else 0.0     # (sparse_hals_step.check_steps: OBJ_FLOOR of 1/2 ||X||^2)
    fails = []
    for i, h in enumerate((p.h0, run.h)):
        want, got = T.host_objective(c, h), float(run.objectives[i])
        rel = abs(got - want) / max(abs(want), scale) if max(abs(want), scale) > 0 else abs(got)
        print(f"{T.case_id(c)}: obj[{i}] rel {rel:.3e}")
        if not rel <= T.OBJ_RTOL:
            fails.append(f"obj[{i}]: recorded {got!r}, float64 of the pair {want!r}: rel {rel:.3e} > {T.OBJ_RTOL:.0e}")
    _fail(fails)


# ---- 5: padding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "masked"])
@pytest.mark.parametrize("k", [3, 40])
def test_padded_components_are_exact_zeros(kind, k):
    """A run with k components equals, bit for bit, the run of the padded width whose extra components start at zero (and,
    with lambda = 0 dead, stay exact zeros): values, sweep counts and objectives."""
    c = T.Case(kind, "base", k, "scaled")
    p = T.problem(c)
    kp = 4 if k <= 4 else 64
    out = []
    for kk in (k, kp):
        wp, hp = np.zeros((p.w.shape[0], kk)), np.zeros((kk, p.h0.shape[1]))
        wp[:, :k], hp[:k] = p.w, p.h0
        with T.engine_for(c, kk) as eng:
            eng.set_factors(wp, hp)
            eng.hals_foldin_run(0.0, **STOP)
            out.append((eng.get_factors()[1], eng.hals_foldin_sweeps(), eng.objectives(0, 2)))
    (h, s, obj), (hp, sp_, objp) = out
    assert (hp[k:] == 0).all()
    assert np.array_equal(h, hp[:k]) and np.array_equal(s, sp_) and np.array_equal(obj, objp)


# ---- 6, 8: the front end --------------------------------------------------------------------------------------------------------
FRONT = [T.Case(kind, matrix, k, "scaled") for kind in ("sparse", "masked") for matrix, k in (("5x4", 4), ("base", 8))]


@pytest.mark.parametrize("c", FRONT, ids=T.case_id)
def test_front_end_is_the_handle_level_run_twice_over(c):
    """hals_transform and NMF.transform return what the handle gives (values, counts, objectives), two calls give the same bits,
    and the caller's arrays are as they were."""
    from nmf_amd import NMF
    from nmf_amd._driver import Results
    from nmf_amd.hals import Experiment, hals_transform
    p = T.problem(c)
    want = T.run_foldin(c, **STOP)
    x = p.x.copy()
    w, h0 = p.w.copy(), p.h0.copy()
    mask = None if p.mask is None else p.mask.copy()
    kw = dict(h0=h0, lambda_h=p.lam, **STOP)
    first = hals_transform(x, w, mask, **kw)
    second = hals_transform(x, w, mask, **kw)
    nmf = NMF(None, c.k)
    nmf.results = Results(w, h0, 0, [1.0], Experiment("hals", c.k, "eu", (False, "zero"), 1, 1e-3, 1e-3, 0, 0, 1))
    nmf.w = w
    third = nmf.transform(x, **kw) if mask is None else nmf.transform(x, mask=mask, **kw)
    for res in (first, second, third):
        assert res.h.dtype == np.float64 and res.h.shape == (c.k, p.h0.shape[1]) and res.sweeps.dtype == np.int32
        assert np.array_equal(res.h, want.h) and np.array_equal(res.sweeps, want.sweeps)
        assert np.array_equal(np.asarray(res.obj_history), want.objectives) and len(res.obj_history) == 2
        assert tuple(res.experiment) == ("hals_transform", c.k, STOP["tol"], STOP["max_sweeps"], p.lam)
    assert np.array_equal(w, p.w) and np.array_equal(h0, p.h0)
    if mask is None:
        assert (x != p.x).nnz == 0
    else:
        assert np.array_equal(x, p.x, equal_nan=True) and np.array_equal(mask, p.mask)
    zero = hals_transform(x, w, mask, lambda_h=p.lam, **STOP)            # the default start: all zeros
    with T.engine_for(c) as eng:
        eng.set_factors(p.w, np.zeros_like(p.h0))
        eng.hals_foldin_run(p.lam, **STOP)
        assert np.array_equal(zero.h, eng.get_factors()[1]) and np.array_equal(zero.sweeps, eng.hals_foldin_sweeps())


def test_a_column_without_an_observed_entry_keeps_its_start():
    c = T.Case("masked", "base", 16, "scaled")
    p = T.problem(c)
    assert p.lam == 0 and (p.nobs == 0).sum() == 2
    run = T.run_foldin(c, **LONG)
    empty = p.nobs == 0
    assert np.array_equal(run.h[:, empty], p.h0[:, empty]) and (run.sweeps[empty] == 1).all()


# ---- 7: the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_refusals_launch_nothing():
    import ctypes as C
    from nmf_amd import _lib as L
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    lib = L.load()
    assert lib.nmfx_version() >= 393
    c = T.Case("masked", "base", 8, "scaled")
    p = T.problem(c)
    n = p.h0.shape[1]
    out = np.zeros(n, dtype=np.int32)
    ptr = out.ctypes.data_as(C.c_void_p)

    def refused(eng, word, *args):
        before = eng.state()
        assert lib.nmfx_hals_foldin_run(eng.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h), (args, lib.nmfx_last_error(eng.h))
        assert eng.state() == before
        assert lib.nmfx_hals_foldin_get_sweeps(eng.h, ptr) == L.NMFX_E_STATE

    with Engine(64, 48, 8) as eng:
        eng.upload_v(np.random.RandomState(0).rand(64, 48))
        eng.set_factors(np.random.RandomState(1).rand(64, 8), np.random.RandomState(2).rand(8, 48))
        refused(eng, b"sparse handle", 0.0, 1e-4, 10)
    rng = np.random.RandomState(5)
    with Engine.for_sparse(masked.observed(p.x, p.mask, 65), 65, masked=True) as eng:
        eng.set_factors(rng.rand(700, 65), rng.rand(65, 600))
        refused(eng, b"more than 64 components", 0.0, 1e-4, 10)
    xs = sp.csr_matrix(T.problem(T.Case("sparse", "base", 8, "scaled")).x, dtype=np.float64)
    with Engine.for_sparse(xs, 129) as eng:
        eng.set_factors(rng.rand(700, 129), rng.rand(129, 600))
        refused(eng, b"more than 128 components", 0.0, 1e-4, 10)
    for cc in (c, T.Case("sparse", "base", 8, "scaled")):
        q = T.problem(cc)
        with T.engine_for(cc) as eng:
            eng.set_factors(q.w, q.h0)
            for tol in (float("nan"), -1e-9, 1.0, float("inf")):
                refused(eng, b"tol", 0.0, tol, 10)
            for cap in (0, -1, 10001):
                refused(eng, b"max_sweeps", 0.0, 1e-4, cap)
            for lam in (-0.5, float("nan")):
                refused(eng, b"lambda", lam, 1e-4, 10)
            h_before = eng.get_factors()[1]
            assert np.array_equal(h_before, q.h0)
            eng.hals_foldin_run(0.0, 1e-4, 10)
            assert lib.nmfx_hals_foldin_get_sweeps(eng.h, ptr) == L.NMFX_OK and (out >= 1).all() and (out <= 10).all()
            assert eng.state()[2] == 2
            eng.set_factors(q.w, q.h0)                       # new factors: the counts are gone with the solve
            assert lib.nmfx_hals_foldin_get_sweeps(eng.h, ptr) == L.NMFX_E_STATE
