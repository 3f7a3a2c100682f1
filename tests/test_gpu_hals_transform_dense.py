"""The dense HALS fold-in on the device (nmfx_hals_foldin_dense_run, nmf_amd.hals.hals_transform_dense), column
by column against the float64 definition of tests/hals_transform_dense_step.py at the bars and the slack proven in
tests/test_hals_transform_dense_bars.py."""
import numpy as np
import pytest

import anls_step as A
import hals_step as HS
import hals_transform_dense_step as D
from mur_step import NEVER

pytestmark = pytest.mark.gpu

LONG, STOP = D.LONG, D.STOP


def _fail(fails):
    if fails:
        raise AssertionError("\n".join(fails))


# ---- 1: the solve at a fixed count is the H half-step, bit for bit --------------------------------------------------------------
# The cold regime: after 16 sweeps every column still moves by more than 1e-4 of its largest component (emulated: 1.1e-4 at k = 16,
# 2.7e-4 at 40, 3.7e-4 at 128; float32 rounding is 6e-8), so no column meets d_s = 0 <= tol xmax_s at tol = 0 and every count is s.
STEP_CASES = [D.Case("cold", 257, 200, k, a) for k, ariths in ((16, ("f32",)), (40, ("f32", "bf16")), (128, ("f32", "bf16")))
              for a in ariths]


def _half_step_and_foldin(c, s):
    """One iteration of hals_run with sweeps = s from (w0, h0) -> (W1, H1); on a fresh handle the fold-in of (W1, h0) with tol = 0
    and max_sweeps = s.  Returns (W1, H1, W, H, counts)."""
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = D.lams_of(c)
    with D.engine_for(c) as eng:
        assert c.k <= 32 or eng.precision() == c.arith
        eng.set_factors(w0, h0)
        eng.hals_run(lw, lh, s, NEVER, 0, 0, 0, 1)
        w1, h1 = eng.get_factors()
    with D.engine_for(c) as eng:
        eng.set_factors(w1, h0)
        eng.hals_foldin_dense_run(lh, 0.0, s)
        w, h = eng.get_factors()
        return w1, h1, w, h, eng.hals_foldin_dense_sweeps()


@pytest.mark.parametrize("c", STEP_CASES, ids=D.case_id)
def test_solve_at_a_fixed_count_is_the_h_half_step(c):
    """The fold-in of (W1, h0) with tol = 0 and max_sweeps = s is the H1 of the half-step with sweeps = s, bit for bit, W is
    untouched and every column counts s sweeps."""
    for s in (1, 3, 16):
        w1, h1, w, h, counts = _half_step_and_foldin(c, s)
        assert np.array_equal(w, w1), f"s = {s}: W was touched"
        assert np.array_equal(h, h1), f"s = {s}: {int((h != h1).any(axis=0).sum())} of {h.shape[1]} columns differ from the H half-step"
        assert counts.dtype == np.int32 and counts.shape == (c.n,) and (counts == s).all(), f"s = {s}: counts {np.unique(counts)}"


def test_a_column_that_stops_moving_stops_with_the_bits_of_the_half_step():
    """The mixed regime at k = 16: columns with a few free components reach a float32 fixed point within 16 sweeps, d_s = 0, and
    stop there at tol = 0 (d_s <= tol xmax_s).  Further sweeps would move nothing: H is still the half-step's, bit for bit."""
    c = D.Case("mixed", 257, 200, 16, "f32")
    w1, h1, w, h, counts = _half_step_and_foldin(c, 16)
    assert np.array_equal(w, w1) and np.array_equal(h, h1)
    assert (counts >= 1).all() and (counts <= 16).all() and (counts < 16).any() and (counts == 16).any(), np.unique(counts)


# ---- 2: beyond the refresh ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", D.CASES, ids=D.IDS)
def test_forty_sweeps_against_float64(c):
    """tol = 0, max_sweeps = 40: every column against the float64 sweep of 40, across both refreshes of the kept residual (a
    column that stopped earlier moved nothing in its last sweep, and would move nothing in the later ones)."""
    run = D.run_foldin(c, **LONG)
    assert c.k <= 32 or run.arith == c.arith
    ref = D.reference(c, "long")
    bar = D.bar_of(c, "long")
    worst, msg = D.deviation(c, run.h, ref, bar, f"{D.case_id(c)} long", record=True)
    print(f"{D.case_id(c)}: worst deviation {worst:.3e} (bar {bar:.1e}); sweeps min {run.sweeps.min()} max {run.sweeps.max()}")
    assert (run.sweeps >= 1).all() and (run.sweeps <= LONG["max_sweeps"]).all()
    _fail([msg] if msg else [])


# ---- 3: the stop rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", D.CASES, ids=D.IDS)
def test_stop_rule(c):
    """tol = 1e-3, max_sweeps = 8: counts in 1 .. 8; on the float64 sweep run for the device's own counts every column stopped
    where the rule says (within the slack) and not before; the values are compared as in test 2, at the STOP bar."""
    run = D.run_foldin(c, **STOP)
    assert run.sweeps.dtype == np.int32 and (run.sweeps >= 1).all() and (run.sweeps <= STOP["max_sweeps"]).all()
    fails, ref = D.stop_failures(c, run.sweeps, STOP["tol"], STOP["max_sweeps"], D.SLACK)
    print(f"{D.case_id(c)}: sweeps 1..8 -> {np.bincount(run.sweeps, minlength=9)[1:].tolist()}")
    if ref is not None:
        bar = D.bar_of(c, "stop")
        worst, msg = D.deviation(c, run.h, ref, bar, f"{D.case_id(c)} stop", record=True)
        print(f"{D.case_id(c)}: worst deviation {worst:.3e} (bar {bar:.1e})")
        if msg:
            fails.append(msg)
    _fail(fails)


# ---- 4: the recorded objectives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", D.CASES, ids=D.IDS)
def test_recorded_objectives_are_the_f64_objective(c):
    """obj[i] is Engine.objective_f64 of the same pair, bit for bit, and the float64 host 1/2 ||x - w h||^2 within OBJ_RTOL."""
    p = D.problem(c)
    run = D.run_foldin(c, **STOP)
    fails = []
    assert run.objectives.shape == (2,)
    for i, h in enumerate((p.h0, run.h)):
        got, want = float(run.objectives[i]), D.host_objective(c, h)
        if got != run.f64[i]:
            fails.append(f"obj[{i}]: recorded {got!r}, objective_f64 of the pair {run.f64[i]!r}")
        rel = abs(got - want) / abs(want)
        print(f"{D.case_id(c)}: obj[{i}] rel {rel:.3e}")
        if not rel <= D.OBJ_RTOL:
            fails.append(f"obj[{i}]: recorded {got!r}, float64 of the pair {want!r}: rel {rel:.3e} > {D.OBJ_RTOL:.0e}")
    _fail(fails)


# ---- 5: determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [D.Case("mixed", 70, 4200, 33, "bf16"), D.Case("mixed", 257, 200, 128, "f32")], ids=D.case_id)
def test_two_runs_give_the_same_bits(c):
    p = D.problem(c)
    first = D.run_foldin(c, **STOP)
    with D.engine_for(c) as eng:
        second = D.foldin(eng, p.w, p.h0, p.lam, **STOP)
        third = D.foldin(eng, p.w, p.h0, p.lam, **STOP)           # the same handle again, after set_factors
    for other in (second, third):
        assert np.array_equal(first.h, other.h) and np.array_equal(first.sweeps, other.sweeps)
        assert np.array_equal(first.objectives, other.objectives)


# ---- 6: padding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,kk", [(D.Case("cold", 257, 200, 15, "f32"), 16), (D.Case("cold", 257, 200, 17, "f32"), 32),
                                  (D.Case("mixed", 257, 200, 33, "bf16"), 64), (D.Case("mixed", 257, 200, 65, "bf16"), 128)],
                         ids=lambda a: D.case_id(a) if isinstance(a, tuple) else f"in{a}")
def test_padded_components_are_exact_zeros(c, kk):
    """The run with k components equals, bit for bit, the run on a handle of the padded width whose extra components start at
    zero: leading rows, sweep counts and objectives; the extra rows stay exact zeros (lambda_h = 0: they are dead)."""
    p = D.problem(c)
    want = D.run_foldin(c, **STOP) if p.lam == 0 else None       # (the runs below are at lambda_h = 0)
    out = []
    for k in (c.k, kk):
        wp, hp = np.zeros((c.m, k)), np.zeros((k, c.n))
        wp[:, :c.k], hp[:c.k] = p.w, p.h0
        with D.engine_for(c, k) as eng:
            out.append(D.foldin(eng, wp, hp, 0.0, **STOP))
    a, b = out
    assert (b.h[c.k:] == 0).all()
    assert np.array_equal(a.h, b.h[:c.k]) and np.array_equal(a.sweeps, b.sweeps) and np.array_equal(a.objectives, b.objectives)
    if want is not None:
        assert np.array_equal(a.h, want.h) and np.array_equal(a.sweeps, want.sweeps)


# ---- 7: dead components and exact zeros -----------------------------------------------------------------------------------------
def test_a_dead_component_keeps_its_start():
    """G_33 = 0 at lambda = 0: row 3 of H is written back as it was read, whatever it holds, and counts towards xmax."""
    c = D.Case("dead", 257, 200, 40, "bf16")
    p = D.problem(c)
    assert p.lam == 0 and np.diag(p.g)[3] == 0 and (p.w[:, 3] == 0).all()
    h0 = p.h0.copy()
    h0[3] = A.f32(np.linspace(0.25, 2.0, c.n))
    with D.engine_for(c) as eng:
        run = D.foldin(eng, p.w, h0, 0.0, **LONG)
    assert np.array_equal(run.h[3], h0[3])
    base = D.run_foldin(c, **LONG)
    assert np.array_equal(base.h[3], p.h0[3]) and (base.h[3] == 0).all()
    live = np.arange(c.k) != 3
    assert np.array_equal(run.h[live], base.h[live])                 # (column 3 of W is zero: the other components never see it)


@pytest.mark.parametrize("c", [D.Case("mixed", 257, 200, 64, "bf16"), D.Case("cold", 257, 200, 40, "bf16"),
                               D.Case("mixed", 257, 200, 128, "f32")], ids=D.case_id)
def test_strictly_clamped_zeros_are_exact_zeros(c):
    """The STRICT rule, counted: every reference zero with a dual beyond STRICT max|r_c| (and beyond the bar's reach) is an exact
    zero of the device, in both runs."""
    p = D.problem(c)
    for name, cfg in (("long", LONG), ("stop", STOP)):
        run = D.run_foldin(c, **cfg)
        ref = D.reference(c, "long") if name == "long" else D.reference(c, "stop", counts=run.sweeps)
        bar = D.bar_of(c, name)
        top = ref.x.max(axis=0)
        strict = (ref.x == 0) & (ref.numer < -HS.STRICT * np.abs(p.r).max(axis=0)[None, :]) \
            & (-ref.numer > bar * np.where(top > 0, top, 1.0)[None, :] * np.diag(p.g)[:, None])
        assert strict.sum() > 50, int(strict.sum())
        assert (run.h[strict] == 0).all(), f"{name}: {int((run.h[strict] != 0).sum())} of {int(strict.sum())} strictly clamped entries are not 0"
        assert not np.signbit(run.h).any()


# ---- 8: one product pass --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [D.Case("mixed", 257, 200, 64, "bf16"), D.Case("mixed", 257, 200, 64, "f32"),
                               D.Case("cold", 257, 200, 17, "f32")], ids=D.case_id)
def test_one_product_pass_and_one_solve_launch(c):
    p = D.problem(c)
    with D.engine_for(c) as eng:
        eng.set_factors(p.w, p.h0)
        eng.profile_enable(True)
        eng.profile_reset()
        eng.hals_foldin_dense_run(p.lam, **LONG)
        eng.state()                                       # (synchronises)
        assert eng.profile_get("hphase")[1] == 1
        assert eng.profile_get("hals_solve")[1] == 1
        for name in ("wphase", "wphase_noobj", "hals_sweep", "nnls", "objective"):
            assert eng.profile_get(name)[1] == 0, name
        assert eng.profile_get("objective_f64")[1] == 2
        assert eng.hals_foldin_dense_sweeps().max() > 16


# ---- 9: the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_refusals_launch_nothing():
    import ctypes as C
    import scipy.sparse as sp
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    lib = L.load()
    assert lib.nmfx_version() >= 394
    rng = np.random.RandomState(5)
    v = rng.rand(64, 48)

    def refused(eng, word, *args):
        out = np.zeros(eng.n, dtype=np.int32)
        ptr = out.ctypes.data_as(C.c_void_p)
        before = eng.state()
        assert lib.nmfx_hals_foldin_dense_run(eng.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h), (args, lib.nmfx_last_error(eng.h))
        assert eng.state() == before
        assert lib.nmfx_hals_foldin_dense_get_sweeps(eng.h, ptr) == L.NMFX_E_STATE

    with Engine.for_sparse(sp.csr_matrix(v), 8) as eng:
        eng.set_factors(rng.rand(64, 8), rng.rand(8, 48))
        refused(eng, b"dense handle", 0.0, 1e-4, 10)
    with Engine(64, 48, 8) as eng:
        eng.upload_v(v)
        eng.upload_weights((v > 0.3).astype(np.float32))
        eng.set_factors(rng.rand(64, 8), rng.rand(8, 48))
        refused(eng, b"weights", 0.0, 1e-4, 10)
    with Engine(64, 48, 129) as eng:
        eng.upload_v(v)
        eng.set_factors(rng.rand(64, 129), rng.rand(129, 48))
        refused(eng, b"more than 128 components", 0.0, 1e-4, 10)
    w, h0 = rng.rand(64, 8), rng.rand(8, 48)
    with Engine(64, 48, 8) as eng:
        out = np.zeros(48, dtype=np.int32)
        ptr = out.ctypes.data_as(C.c_void_p)
        eng.upload_v(v)
        eng.set_factors(w, h0)
        for tol in (float("nan"), -1e-9, 1.0, float("inf")):
            refused(eng, b"tol", 0.0, tol, 10)
        for cap in (0, -1, 10001):
            refused(eng, b"max_sweeps", 0.0, 1e-4, cap)
        for lam in (-0.5, float("nan")):
            refused(eng, b"lambda", lam, 1e-4, 10)
        before = eng.state()
        assert lib.nmfx_hals_foldin_run(eng.h, 0.0, 1e-4, 10) == L.NMFX_E_ARG and b"sparse handle" in lib.nmfx_last_error(eng.h)
        assert lib.nmfx_hals_foldin_get_sweeps(eng.h, ptr) == L.NMFX_E_STATE
        assert eng.state() == before
        wd, hd = eng.get_factors()
        assert np.array_equal(wd, A.f32(w)) and np.array_equal(hd, A.f32(h0))
        eng.hals_foldin_dense_run(0.0, 1e-4, 10)
        assert lib.nmfx_hals_foldin_dense_get_sweeps(eng.h, ptr) == L.NMFX_OK and (out >= 1).all() and (out <= 10).all()
        assert eng.state()[0] == 0 and eng.state()[2] == 2                        # no stop, two objectives
        assert np.array_equal(eng.get_factors()[0], A.f32(w))
        assert lib.nmfx_hals_foldin_get_sweeps(eng.h, ptr) == L.NMFX_E_STATE      # the sparse entry point knows nothing of it
        eng.set_factors(w, h0)                            # new factors: the counts are gone with the solve
        assert lib.nmfx_hals_foldin_dense_get_sweeps(eng.h, ptr) == L.NMFX_E_STATE
        eng.anls_run(0.0, 0.0, NEVER, 0, 0, 0, 1)         # another family has run: the fold-in does not continue it
        assert lib.nmfx_hals_foldin_dense_run(eng.h, 0.0, 1e-4, 10) == L.NMFX_E_STATE


# ---- 10: the front ends ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [D.Case("mixed", 5, 4, 4, "f32"), D.Case("cold", 257, 200, 17, "f32")], ids=D.case_id)
def test_front_ends_return_what_the_handle_gives(c):
    """hals_transform_dense and NMF.transform(x, solver='hals') return what the handle gives (values, counts, objectives), and
    the caller's arrays are as they were; the default start is all zeros."""
    from nmf_amd import NMF
    from nmf_amd._driver import Results
    from nmf_amd.engine import Engine
    from nmf_amd.hals import Experiment, hals_transform_dense
    p = D.problem(c)
    x, w, h0 = p.v.copy(), p.w.copy(), p.h0.copy()
    with Engine.for_data(x, c.k) as eng:                  # (the front end's engine: the default arithmetic mode)
        want = D.foldin(eng, p.w, p.h0, p.lam, **STOP)
        zero = D.foldin(eng, p.w, np.zeros_like(p.h0), p.lam, **STOP)
    kw = dict(h0=h0, lambda_h=p.lam, **STOP)
    first = hals_transform_dense(x, w, **kw)
    nmf = NMF(None, c.k)
    nmf.results = Results(w, h0, 0, [1.0], Experiment("hals", c.k, "eu", (False, "zero"), 1, 1e-3, 1e-3, 0, 0, 1))
    nmf.w = w
    second = nmf.transform(x, solver="hals", **kw)
    for res in (first, second):
        assert res.h.dtype == np.float64 and res.h.shape == (c.k, c.n) and res.sweeps.dtype == np.int32
        assert np.array_equal(res.h, want.h) and np.array_equal(res.sweeps, want.sweeps)
        assert np.array_equal(np.asarray(res.obj_history), want.objectives) and len(res.obj_history) == 2
        assert tuple(res.experiment) == ("hals_transform", c.k, STOP["tol"], STOP["max_sweeps"], p.lam)
    assert np.array_equal(x, p.v) and np.array_equal(w, p.w) and np.array_equal(h0, p.h0)
    res = hals_transform_dense(x, w, lambda_h=p.lam, **STOP)
    assert np.array_equal(res.h, zero.h) and np.array_equal(res.sweeps, zero.sweeps)
