"""MUR with the beta-divergence on the device (kernels_phase.hip) against the float64 statement of tests/beta_ref.py.
Runs only on a real MI355X (`-m gpu`).

Bars.  Half-steps: mur_step.BARS[("f32", "kl")] = 2e-5, the project's bar for exact-f32 kernels: gamma <= 1 never amplifies
the error of the ratio of sums, and the power's share has to fit inside it (the kernels use full-precision powf).  Recorded
objective: mur_step.OBJ_RTOL (1e-5), relative to max(|objective|, OBJ_FLOOR x the data scale) -- the convention of
tests/test_gpu_weighted.py; the data scale of d_beta is its x-only term, Sum om x^beta / |beta (beta - 1)| (1/2 Sum om x^2
at beta = 2), Sum om x at beta = 1 and 0 at beta = 0 (scale-invariant, as for 'is').  Whole runs: the project's WH_TOL.
Every comparison prints its figure before it asserts.

The measured maxima belong in DESIGN.md 4.5 (not measured yet)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from beta_ref import beta_h_step, beta_mur, beta_objective, beta_w_step
from gpu_common import WH_TOL, wh_error
from mur_step import BARS, NEVER, OBJ_FLOOR, OBJ_RTOL, compare, make_inputs
from oracle import nmf_ref as R
from weighted_cases import log_uniform_weights, stop_margins

pytestmark = pytest.mark.gpu

BAR = BARS[("f32", "kl")]


def _mur(*a, **kw):
    from nmf_amd.mur import mur
    return mur(*a, **kw)


def drive(eng, code, w0, h0, lw, lh, steps=(1, 2)):
    """The calls nmf_amd.mur.mur makes, with the stop rule off: {s: (W_s, H_s, recorded objectives 0 .. s)}."""
    out = {}
    for s in steps:
        eng.set_factors(w0, h0)
        eng.mur_run(code, lw, lh, NEVER, 0, 0, 0, s)
        eng.mur_finish(code, NEVER, 0, 0, s)
        w, h = eng.get_factors()
        out[s] = (w, h, eng.objectives(0, s + 1))
    return out


def data_scale(x, om, beta):
    xo = np.where(om > 0, x, 0.0)
    if beta == 0:
        return 0.0
    if beta == 1:
        return float(np.sum(om * xo))
    live = (om > 0) & (xo > 0) if beta < 0 else om > 0
    return float(np.sum(om[live] * xo[live] ** beta)) / abs(beta * (beta - 1.0))


def beta_inputs(m, n, k, beta, seed):
    """make_inputs; for beta > 0 about 30 % of V are exact zeros, plus (m, n >= 8) an all-zero row and column: zeros are
    data there.  For beta <= 0 V stays strictly positive (uniform in [0.05, 1))."""
    v, w0, h0 = make_inputs(m, n, k, seed=seed)
    if beta > 0:
        rng = np.random.default_rng(seed + 1)
        v[rng.random(v.shape) < 0.3] = 0
        if m >= 8 and n >= 8:
            v[1, :] = 0
            v[:, 2] = 0
    return v, w0, h0


def check(tag, x, om, beta, w0, h0, lw, lh, runs):
    """Every half-step against the yardstick fed the device's previous iterate, every recorded objective against the
    float64 objective of the device's iterates.  Returns the worst figures; raises naming every failure."""
    fails, worst, iterate = [], {}, {0: (w0, h0)}
    for s in sorted(runs):
        ws, hs, _ = runs[s]
        wp, hp = iterate[s - 1]
        for label, dev, ref in ((f"W{s}", ws, beta_w_step(x, wp, hp, beta, lw, om)),
                                (f"H{s}", hs, beta_h_step(x, ws, hp, beta, lh, om))):
            err, msg = compare(f"{tag} {label}", dev, ref, BAR)
            worst[label] = err
            if msg:
                fails.append(msg)
        iterate[s] = (ws, hs)
    omd = np.ones(x.shape) if om is None else om
    scale = OBJ_FLOOR * data_scale(x, omd, beta)
    for s, (_, _, hist) in sorted(runs.items()):
        for i in range(s + 1):
            want = beta_objective(x, *iterate[i], beta, om)
            rel = abs(float(hist[i]) - want) / max(abs(want), scale)
            worst[f"obj[{i}]/{s}"] = rel
            if not rel <= OBJ_RTOL:
                fails.append(f"{tag} obj[{i}] of the {s}-step run: recorded {hist[i]!r}, float64 {want!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    print(f"{tag}: worst relative errors", {key: f"{val:.2e}" for key, val in worst.items()})
    assert not fails, "\n".join(fails)
    return worst


# ---- 1. half-steps element by element ------------------------------------------------------------------------------------
# (m, n, k, lambda_w, lambda_h, betas): the shapes of tests/test_gpu_is.py / test_gpu_weighted.py -- padded ranks 16, 64, 128,
# ragged edges, n = 1, splits -- plus two that pad to 32; every padded rank sees a beta of each gamma branch
# (beta < 1, 1 <= beta <= 2, beta > 2) and every beta of the grid appears.
SHAPES = [(127, 1, 3, 0.0, 0.0, (-1.0, 1.0, 2.5)), (700, 600, 16, 0.05, 0.0, (0.5, 1.5, 3.0)),
          (130, 70, 20, 0.0, 0.02, (0.9, 2.0, 2.5)), (300, 200, 20, 0.0, 0.1, (0.5,)), (300, 200, 33, 0.0, 0.1, (-0.5, 2.0, 2.5)),
          (257, 130, 64, 0.1, 0.05, (0.9, 1.0, 3.0)), (700, 600, 100, 0.0, 0.0, (0.0, 1.5, 2.5)),
          (640, 384, 128, 0.02, 0.3, (0.5, 2.0, 3.0))]
CASES = [(m, n, k, lw, lh, b) for m, n, k, lw, lh, bs in SHAPES for b in bs]


def test_the_cases_cover_the_grid():
    assert {c[5] for c in CASES} == {-1.0, -0.5, 0.0, 0.5, 0.9, 1.0, 1.5, 2.0, 2.5, 3.0}


@pytest.mark.parametrize("m,n,k,lw,lh,beta", CASES)
def test_half_steps_element_by_element(m, n, k, lw, lh, beta):
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    v, w0, h0 = beta_inputs(m, n, k, beta, seed=4000 + k)
    x = v.astype(np.float64)
    with Engine(m, n, k) as eng:
        eng.upload_v(v)
        eng.set_beta(beta)
        assert "exact-f32" in eng.note() and "beta" in eng.note(), eng.note()
        runs = drive(eng, L.BETA, w0, h0, lw, lh)
    check(f"beta={beta} {m}x{n} k={k}", x, None, beta, w0, h0, lw, lh, runs)
    if beta > 0 and m >= 8 and n >= 8:                             # an all-zero row / column of V: exactly 0
        for s in runs:
            assert (runs[s][0][1] == 0).all() and (runs[s][1][:, 2] == 0).all()


# ---- 2. the same with weights= ---------------------------------------------------------------------------------------------
WEIGHTED_CASES = [(m, n, k, lw, lh, b) for b in (0.5, 1.5, -1.0)
                  for m, n, k, lw, lh in [(300, 200, 33, 0.0, 0.1), (257, 130, 64, 0.1, 0.05), (640, 384, 128, 0.02, 0.3)]]
WEIGHTED_CASES.append((300, 200, 20, 0.0, 0.1, 0.5))              # padded rank 32


@pytest.mark.parametrize("m,n,k,lw,lh,beta", WEIGHTED_CASES)
def test_weighted_half_steps_element_by_element(m, n, k, lw, lh, beta):
    from nmf_amd import _lib as L
    from nmf_amd import weighted
    from nmf_amd.engine import Engine
    v, w0, h0 = beta_inputs(m, n, k, beta, seed=5000 + k)
    om = log_uniform_weights((m, n), seed=6000 + k, edges=True)
    x = v.astype(np.float64)
    x[om == 0] = np.nan                                            # never read: the device receives 0 there
    x32, w32 = weighted.prepare(x, om, k, "beta", beta=beta)
    with Engine(m, n, k) as eng:
        eng.upload_v(x32)
        eng.upload_weights(w32)
        eng.set_beta(beta)
        runs = drive(eng, L.BETA, w0, h0, lw, lh)
    check(f"weighted beta={beta} {m}x{n} k={k}", x, om.astype(np.float64), beta, w0, h0, lw, lh, runs)
    for s in runs:                                                 # no weight at all: exactly 0, no NaN
        assert np.isfinite(runs[s][0]).all() and np.isfinite(runs[s][1]).all()
        assert (runs[s][0][1:3] == 0).all() and (runs[s][1][:, 3] == 0).all()


# ---- 3. whole runs ---------------------------------------------------------------------------------------------------------
def run_data(seed=3):
    return R.planted_matrix(300, 200, 12, seed=seed, dtype=np.float64) + 0.01


@pytest.mark.parametrize("beta", [0.5, 1.5])
def test_run_against_the_float64_run(beta):
    x = run_data()
    x[np.random.RandomState(8).rand(*x.shape) < 0.05] = 0.0        # zeros are data for beta > 0
    kw = dict(min_iter=30, max_iter=30, lambda_w=0.01)
    np.random.seed(4)
    got = _mur(x.copy(), 12, distance_type="beta", beta=beta, **kw)
    np.random.seed(4)
    want = beta_mur(x, 12, beta, **kw)
    assert got.i == want.i == 29 and len(got.obj_history) == len(want.obj_history) == 31
    err = wh_error(got.w, got.h, want.w, want.h, x)
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    print(f"beta run (beta={beta}): wh_error {err:.2e}, history rel {rel:.2e}")
    assert err < WH_TOL
    assert got.experiment.distance_type == "beta" and got.experiment.beta == beta and got.experiment[-1] == beta
    assert (got.w >= 0).all() and (got.h >= 0).all()


def test_weighted_run_against_the_float64_run():
    from nmf_amd import weighted
    x = run_data()
    om = (np.random.RandomState(7).rand(*x.shape) < 0.7).astype(np.float64)      # a 0 / 1 hold-out pattern
    xn = np.where(om > 0, x, np.nan)
    kw = dict(min_iter=30, max_iter=30)
    np.random.seed(4)
    got = _mur(xn, 12, distance_type="beta", beta=0.5, weights=om, **kw)
    np.random.seed(4)
    want = beta_mur(xn, 12, 0.5, om, **kw)
    err = wh_error(got.w, got.h, want.w, want.h, np.where(om > 0, x, 0.0))
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    held = weighted.objective(x, got.w, got.h, 1.0 - om, "beta", beta=0.5)
    print(f"weighted beta run (0/1, beta=0.5): wh_error {err:.2e}, history rel {rel:.2e}, held-out objective {held:.4g}")
    assert got.i == want.i == 29
    assert err < WH_TOL
    h = np.asarray(got.obj_history)
    assert np.all(h[1:] <= h[:-1] * (1 + OBJ_RTOL)), np.diff(h).max()           # lambda = 0: the MM rule never increases it


def test_beta_0_agrees_with_the_is_run():
    x = run_data()
    kw = dict(min_iter=30, max_iter=30, lambda_h=0.01)
    np.random.seed(5)
    got = _mur(x.copy(), 12, distance_type="beta", beta=0.0, **kw)
    np.random.seed(5)
    want = _mur(x.copy(), 12, distance_type="is", **kw)
    err = wh_error(got.w, got.h, want.w, want.h, x)
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    print(f"beta = 0 vs 'is': wh_error {err:.2e}, history rel {rel:.2e}")
    assert err < WH_TOL and got.i == want.i


def test_beta_1_agrees_with_the_exact_f32_kl_run(monkeypatch):
    monkeypatch.setenv("NMFX_PRECISION", "f32")
    x = run_data()
    kw = dict(min_iter=30, max_iter=30)                            # lambda = 0: the two closed forms coincide
    np.random.seed(5)
    got = _mur(x.copy(), 12, distance_type="beta", beta=1.0, **kw)
    np.random.seed(5)
    want = _mur(x.copy(), 12, distance_type="kl", **kw)
    err = wh_error(got.w, got.h, want.w, want.h, x)
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    print(f"beta = 1 vs exact-f32 'kl': wh_error {err:.2e}, history rel {rel:.2e}")
    assert err < WH_TOL and got.i == want.i


# chosen on the CPU (float64 run of beta_mur): with these the run stops at i = 5 and its last two decisions sit about 250 x
# OBJ_RTOL x objective from the threshold
STOP = dict(seed=3, min_iter=3, max_iter=400, tol1=1e-5, tol2=20.4)


def test_stop_rule_fires_where_the_float64_run_stops():
    x = run_data()
    kw = {key: val for key, val in STOP.items() if key != "seed"}
    np.random.seed(STOP["seed"])
    want = beta_mur(x, 12, 0.5, **kw)
    margins = stop_margins(want, kw["tol2"])
    print(f"beta stop: float64 run stops at i = {want.i}, margins of its last two decisions {margins} (x OBJ_RTOL x objective)")
    assert want.trace["stop_rule"] == 2 and kw["min_iter"] < want.i < 399 and min(margins) > 150      # the yardstick alone
    np.random.seed(STOP["seed"])
    got = _mur(x.copy(), 12, distance_type="beta", beta=0.5, **kw)
    err = wh_error(got.w, got.h, want.w, want.h, x)
    print(f"beta stop: device i = {got.i}, factors at the stop vs the float64 run {err:.2e}")
    assert got.i == want.i and len(got.obj_history) == len(want.obj_history) == got.i + 2
    assert err < WH_TOL


@pytest.mark.parametrize("weighted_run", [False, True])
def test_two_runs_bit_identical(weighted_run):
    x = run_data(5)
    kw = dict(weights=log_uniform_weights(x.shape, seed=11).astype(np.float64)) if weighted_run else {}
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(_mur(x.copy(), 24, distance_type="beta", beta=0.5, min_iter=15, max_iter=15, **kw))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))


# ---- 4. ABI ----------------------------------------------------------------------------------------------------------------
def _eu_still_runs(eng, v, w0, h0):
    """After a refusal the handle runs 'eu' as a fresh one does."""
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    got = drive(eng, L.EU, w0, h0, 0.0, 0.0, steps=(2,))[2]
    with Engine(*v.shape, w0.shape[1]) as fresh:
        fresh.upload_v(v)
        want = drive(fresh, L.EU, w0, h0, 0.0, 0.0, steps=(2,))[2]
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_refusals_at_the_abi():
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    lib = L.require_gpu()
    assert lib.nmfx_version() >= 350 and L.BETA == 3
    v, w0, h0 = make_inputs(200, 160, 8, seed=9)
    with Engine(200, 160, 8) as eng:
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        h = eng.h
        rc = lib.nmfx_mur_run(h, L.BETA, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1)                # beta never set
        assert rc == L.NMFX_E_STATE and b"beta" in lib.nmfx_last_error(h)
        rc = lib.nmfx_mur_finish(h, L.BETA, NEVER, 0.0, 0.0, 0)
        assert rc == L.NMFX_E_STATE and b"beta" in lib.nmfx_last_error(h)
        assert eng.state()[2] == 0
        _eu_still_runs(eng, v, w0, h0)
        for bad in (3.5, -1.5, float("nan"), float("inf")):
            rc = lib.nmfx_set_beta(h, bad)
            assert rc == L.NMFX_E_ARG and b"beta" in lib.nmfx_last_error(h), bad
        eng.set_factors(w0, h0)
        rc = lib.nmfx_mur_run(h, L.BETA, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1)                # ... which stored nothing
        assert rc == L.NMFX_E_STATE
        _eu_still_runs(eng, v, w0, h0)
        eng.set_beta(0.5)
        eng.set_factors(w0, h0)
        i64, dbl = C.c_int64(), C.c_double()
        calls = {
            "mur_phase_a": lambda: lib.nmfx_mur_phase_a(h, L.BETA, 0.0, 0),
            "mur_phase_b": lambda: lib.nmfx_mur_phase_b(h, L.BETA, 0.0, NEVER, 0.0, 0.0, 0),
            "mur_finish_a": lambda: lib.nmfx_mur_finish_a(h, L.BETA, 0),
            "mur_chunk_info": lambda: lib.nmfx_mur_chunk_info(h, L.BETA, C.byref(i64), C.byref(i64), C.byref(i64)),
            "mur_phase_a_head": lambda: lib.nmfx_mur_phase_a_head(h, L.BETA, 0.0, 0),
            "mur_phase_a_cols": lambda: lib.nmfx_mur_phase_a_cols(h, L.BETA, 0, 128),
            "mur_slice_info": lambda: lib.nmfx_mur_slice_info(h, L.BETA, 1, C.byref(i64), C.byref(i64)),
            "mur_phase_b_slice": lambda: lib.nmfx_mur_phase_b_slice(h, L.BETA, 0.0, NEVER, 0.0, 0.0, 0, 0, 64),
            "mur_phase_b_rest": lambda: lib.nmfx_mur_phase_b_rest(h, L.BETA, 0, 64),
            "mur_run_sharded": lambda: lib.nmfx_mur_run_sharded(h, L.BETA, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1),
            "mur_finish_sharded": lambda: lib.nmfx_mur_finish_sharded(h, L.BETA, NEVER, 0.0, 0.0, 0),
            "profile_repeat": lambda: lib.nmfx_profile_repeat(h, b"wphase", L.BETA, 1, C.byref(dbl)),
        }
        for name, call in calls.items():
            rc = call()
            msg = lib.nmfx_last_error(h)
            assert rc == L.NMFX_E_ARG and b"beta" in msg, (name, rc, msg)
            st = eng.state()
            assert st[0] == 0 and st[2] == 0, (name, st)          # nothing was recorded, nothing stopped
        _eu_still_runs(eng, v, w0, h0)
        eng.set_factors(w0, h0)
        eng.mur_run(L.BETA, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1)      # a beta run: the Euclidean f64 referee does not apply
        rc = lib.nmfx_objective_f64(h, C.byref(dbl))
        assert rc == L.NMFX_E_ARG and b"beta" in lib.nmfx_last_error(h)
        _eu_still_runs(eng, v, w0, h0)

    xs = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 4)
    with Engine.for_sparse(xs, 4) as eng:                         # a sparse handle
        rc = lib.nmfx_set_beta(eng.h, 0.5)
        assert rc == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(eng.h)
        rs = np.random.RandomState(0)
        eng.set_factors(np.abs(rs.randn(64, 4)), np.abs(rs.randn(4, 48)))
        rc = lib.nmfx_mur_run(eng.h, L.BETA, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1)
        assert rc == L.NMFX_E_ARG and b"beta" in lib.nmfx_last_error(eng.h)
        eng.mur_run(L.EU, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1)        # ... and still runs 'eu'
        eng.mur_finish(L.EU, NEVER, 0.0, 0.0, 1)
        assert eng.state()[2] == 2 and np.isfinite(eng.get_factors()[0]).all()
    v2, w2, h2 = make_inputs(200, 160, 200, seed=10)
    with Engine(200, 160, 200) as eng:                            # k > 128
        eng.upload_v(v2)
        rc = lib.nmfx_set_beta(eng.h, 0.5)
        assert rc == L.NMFX_E_ARG and b"128" in lib.nmfx_last_error(eng.h)
        _eu_still_runs(eng, v2, w2, h2)
