"""MUR with the beta-divergence and automatic relevance determination on the device (kernels_phase.hip, nmfx_set_ard) against
the float64 statement of tests/ard_ref.py.  Runs only on a real MI355X (`-m gpu`).

Bars.  Half-steps: mur_step.BARS[("f32", "kl")] = 2e-5, the beta path's bar: the penalty only adds a positive f32 constant to
a denominator and gamma <= 1 does not amplify.  Relevance: rtol 1e-10 (an f64 sum over exact f32 values; only the order of
the additions differs).  Recorded objective: mur_step.OBJ_RTOL relative to |Sum om d_beta| + |penalty| + the beta tests'
data-scale floor (the two parts can cancel, so the error is not measured against their sum alone).  Whole runs: WH_TOL.
Every comparison prints its figure before it asserts; the measured maxima belong in DESIGN.md 4.6."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from ard_cases import GAP, RANK, kept_and_gap, rank_reference
from ard_ref import ard_default_b, ard_h_step, ard_lambda, ard_mur, ard_penalty, ard_relevance, ard_w_step
from beta_ref import beta_objective
from gpu_common import WH_TOL, wh_error
from mur_step import BARS, NEVER, OBJ_FLOOR, OBJ_RTOL, compare, make_inputs
from oracle import nmf_ref as R
from weighted_cases import log_uniform_weights

pytestmark = pytest.mark.gpu

BAR = BARS[("f32", "kl")]
LAM_RTOL = 1e-10
PHI, A = 5.0, 5.0            # half-step cases: phi / lambda_k is a few per cent of the denominators


def _ard(*a, **kw):
    from nmf_amd.ard import mur_ard
    return mur_ard(*a, **kw)


def drive(eng, w0, h0, steps=(1, 2)):
    """The calls nmf_amd.ard.mur_ard makes, with the stop rule off:
    {0: lambda_0, s: (W_s, H_s, recorded objectives 0 .. s, lambda_s)}."""
    from nmf_amd import _lib as L
    out = {}
    for s in steps:
        eng.set_factors(w0, h0)
        if 0 not in out:
            out[0] = eng.relevance()                               # lambda_0, before any run
        eng.mur_run(L.BETA, 0.0, 0.0, NEVER, 0, 0, 0, s)
        eng.mur_finish(L.BETA, NEVER, 0, 0, s)
        w, h = eng.get_factors()
        out[s] = (w, h, eng.objectives(0, s + 1), eng.relevance())
    return out


def data_scale(x, om, beta):
    """The x-only term of d_beta (tests/test_gpu_beta.py)."""
    xo = np.where(om > 0, x, 0.0)
    if beta == 0:
        return 0.0
    if beta == 1:
        return float(np.sum(om * xo))
    live = (om > 0) & (xo > 0) if beta < 0 else om > 0
    return float(np.sum(om[live] * xo[live] ** beta)) / abs(beta * (beta - 1.0))


def ard_inputs(m, n, k, beta, seed):
    """make_inputs; for beta > 0 about 30 % of V are exact zeros, plus (m, n >= 8) an all-zero row and column.  For
    beta <= 0 V stays strictly positive."""
    v, w0, h0 = make_inputs(m, n, k, seed=seed)
    if beta > 0:
        rng = np.random.default_rng(seed + 1)
        v[rng.random(v.shape) < 0.3] = 0
        if m >= 8 and n >= 8:
            v[1, :] = 0
            v[:, 2] = 0
    return v, w0, h0


def check(tag, x, om, beta, b, w0, h0, runs):
    """Every half-step against the yardstick fed the device's previous iterate and the lambda recomputed from it in float64;
    every lambda against the float64 lambda of the factors read back; every recorded objective against nmf_amd.ard.objective
    of the device's iterate and lambda.  Raises naming every failure."""
    from nmf_amd import ard
    fails, worst, iterate, lam_dev = [], {}, {0: (w0, h0)}, {0: runs[0]}
    steps = sorted(s for s in runs if s)
    for s in steps:
        ws, hs, _, lam_s = runs[s]
        wp, hp = iterate[s - 1]
        lam = ard_lambda(wp, hp, A, b)
        for label, dev, ref in ((f"W{s}", ws, ard_w_step(x, wp, hp, lam, beta, PHI, om)),
                                (f"H{s}", hs, ard_h_step(x, ws, hp, lam, beta, PHI, om))):
            err, msg = compare(f"{tag} {label}", dev, ref, BAR)
            worst[label] = err
            if msg:
                fails.append(msg)
        iterate[s], lam_dev[s] = (ws, hs), lam_s
    for s in sorted(lam_dev):
        want = ard_lambda(*iterate[s], A, b)
        rel = float(np.max(np.abs(lam_dev[s] - want) / want))
        worst[f"lambda{s}"] = rel
        if not (lam_dev[s].shape == want.shape and rel <= LAM_RTOL):
            fails.append(f"{tag} lambda_{s}: rel {rel:.3e} > {LAM_RTOL:.0e}")
    omd = np.ones(x.shape) if om is None else om
    xs = np.where(omd > 0, x, 0.0)
    scale = OBJ_FLOOR * data_scale(x, omd, beta)
    for s in steps:
        hist = runs[s][2]
        for i in range(s + 1):
            want = ard.objective(xs, *iterate[i], lam_dev[i], beta, PHI, A, b, weights=om)
            size = abs(beta_objective(x, *iterate[i], beta, om)) + abs(ard_penalty(*iterate[i], lam_dev[i], PHI, A, b)) + scale
            rel = abs(float(hist[i]) - want) / size
            worst[f"obj[{i}]/{s}"] = rel
            if not rel <= OBJ_RTOL:
                fails.append(f"{tag} obj[{i}] of the {s}-step run: recorded {hist[i]!r}, float64 {want!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    print(f"{tag}: worst relative errors", {key: f"{val:.2e}" for key, val in worst.items()})
    assert not fails, "\n".join(fails)
    return worst


# ---- 1 - 3. half-steps, relevance, recorded objective ----------------------------------------------------------------------
# padded ranks 16 / 32 / 64 (k = 33: 31 padded components) / 64 / 128, ragged edges, n = 1; three betas per shape, so that every
# gamma branch (beta < 1, 1 <= beta <= 2, beta > 2) meets every padded rank
SHAPES = [(127, 1, 3, (-1.0, 1.0, 2.5)), (130, 70, 20, (0.5, 1.5, 2.5)), (300, 200, 33, (0.0, 1.0, 2.5)),
          (257, 130, 64, (-1.0, 1.5, 2.5)), (640, 384, 128, (0.5, 1.0, 2.5))]
CASES = [(m, n, k, b) for m, n, k, bs in SHAPES for b in bs]


def test_the_cases_cover_the_betas():
    assert {c[3] for c in CASES} == {-1.0, 0.0, 0.5, 1.0, 1.5, 2.5}


@pytest.mark.parametrize("m,n,k,beta", CASES)
def test_half_steps_relevance_and_objective(m, n, k, beta):
    from nmf_amd.engine import Engine
    v, w0, h0 = ard_inputs(m, n, k, beta, seed=7000 + k)
    x = v.astype(np.float64)
    b = ard_default_b(x, k, A)
    with Engine(m, n, k) as eng:
        eng.upload_v(v)
        eng.set_beta(beta)
        eng.set_ard(PHI, A, b)
        runs = drive(eng, w0, h0)
    check(f"ard beta={beta} {m}x{n} k={k}", x, None, beta, b, w0, h0, runs)
    assert runs[1][3].shape == (k,)
    if beta > 0 and m >= 8 and n >= 8:                             # an all-zero row / column of V: exactly 0
        for s in (1, 2):
            assert (runs[s][0][1] == 0).all() and (runs[s][1][:, 2] == 0).all()


@pytest.mark.parametrize("m,n,k,beta", [(m, n, k, b) for m, n, k in [(300, 200, 33), (640, 384, 128)] for b in (-1.0, 0.5, 1.5)])
def test_weighted_half_steps_relevance_and_objective(m, n, k, beta):
    from nmf_amd import weighted
    from nmf_amd.engine import Engine
    v, w0, h0 = ard_inputs(m, n, k, beta, seed=8000 + k)
    om = log_uniform_weights((m, n), seed=9000 + k, edges=True)
    x = v.astype(np.float64)
    x[om == 0] = np.nan                                            # never read: the device receives 0 there
    x32, w32 = weighted.prepare(x, om, k, "beta", beta=beta)
    omd = om.astype(np.float64)
    b = ard_default_b(np.where(omd > 0, x, 0.0), k, A, omd)
    with Engine(m, n, k) as eng:
        eng.upload_v(x32)
        eng.upload_weights(w32)
        eng.set_beta(beta)
        eng.set_ard(PHI, A, b)
        runs = drive(eng, w0, h0)
    check(f"weighted ard beta={beta} {m}x{n} k={k}", x, omd, beta, b, w0, h0, runs)
    for s in (1, 2):                                               # no weight at all: exactly 0, no NaN
        assert np.isfinite(runs[s][0]).all() and np.isfinite(runs[s][1]).all()
        assert (runs[s][0][1:3] == 0).all() and (runs[s][1][:, 3] == 0).all()


def objective_error(recorded, x, w, h, lam, beta, phi, a, b):
    """|recorded - C| relative to |Sum d_beta| + |penalty| (unweighted data)."""
    fit, pen = beta_objective(x, w, h, beta), ard_penalty(w, h, lam, phi, a, b)
    return abs(float(recorded) - (fit + pen)) / (abs(fit) + abs(pen))


# ---- 4. whole runs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [1.0, 1.5])
def test_rank_recovery(beta):
    x, b, want, rel_want = rank_reference(beta, 0)
    np.random.seed(0)
    got = _ard(x.copy(), RANK["k"], beta=beta, phi=RANK["phi"], a=RANK["a"], min_iter=RANK["iters"], max_iter=RANK["iters"])
    kept_want, gap_want = kept_and_gap(rel_want)
    kept, gap = kept_and_gap(got.relevance)
    err = wh_error(got.w, got.h, want.w, want.h, x)
    print(f"ard rank recovery beta={beta}: device relevances {np.sort(got.relevance)[::-1]}, gap {gap:.3g} (float64 {gap_want:.3g}); "
          f"600-iteration trajectory vs float64: wh_error {err:.2e} (recorded, not asserted)")
    assert got.i == RANK["iters"] - 1 and len(got.obj_history) == RANK["iters"] + 1
    assert got.experiment.b == pytest.approx(b, rel=1e-14) and got.experiment[-3:] == (RANK["phi"], RANK["a"], got.experiment.b)
    assert got.k_eff == RANK["rank"]
    assert gap > GAP and gap_want > GAP
    assert kept == kept_want
    assert got.relevance.dtype == np.float64 and got.relevance.shape == (RANK["k"],)


def run_data(seed=3):
    return R.planted_matrix(300, 200, 12, seed=seed, dtype=np.float64) + 0.01


def test_run_against_the_float64_run():
    x = run_data()
    x[np.random.RandomState(8).rand(*x.shape) < 0.05] = 0.0        # zeros are data for beta > 0
    phi, a = 0.5, 5.0
    b = ard_default_b(x, 12, a)
    np.random.seed(4)
    got = _ard(x.copy(), 12, beta=0.5, phi=phi, a=a, min_iter=30, max_iter=30)
    np.random.seed(4)
    want = ard_mur(x, 12, 0.5, phi, a, b, min_iter=30, max_iter=30)
    assert got.i == want.i == 29 and len(got.obj_history) == len(want.obj_history) == 31
    err = wh_error(got.w, got.h, want.w, want.h, x)
    hist = np.asarray(got.obj_history)
    rel = np.max(np.abs(hist - want.obj_history) / np.abs(want.obj_history))
    rel_lam = np.max(np.abs(got.relevance - ard_relevance(want.trace["lam"], x.shape, a, b)) / ard_relevance(want.trace["lam"], x.shape, a, b))
    print(f"ard run (beta=0.5): wh_error {err:.2e}, history rel {rel:.2e}, relevance rel {rel_lam:.2e}")
    assert err < WH_TOL
    assert got.experiment.distance_type == "beta" and got.experiment.beta == 0.5 and got.experiment.phi == phi
    assert (got.w >= 0).all() and (got.h >= 0).all()
    assert np.all(hist[1:] <= hist[:-1] + OBJ_RTOL * np.abs(hist[:-1]))          # monotone within the objective's own bar
    lam = (got.relevance + 1.0) * (b / (x.shape[0] + x.shape[1] + a + 1.0))
    assert objective_error(hist[-1], x, got.w, got.h, lam, 0.5, phi, a, b) <= OBJ_RTOL


def test_a_stopped_run_returns_the_relevance_of_the_pair_it_stopped_at():
    """tol2 so large that rule 2 fires at the first tested index, min_iter + 1: the H update and the relevance step of that
    iteration are skipped, and factors, relevance and the last objective belong to the same pair."""
    x = run_data(5)
    phi, a = 0.5, 5.0
    np.random.seed(2)
    got = _ard(x.copy(), 12, beta=1.5, phi=phi, a=a, min_iter=3, max_iter=200, tol2=1e12)
    np.random.seed(2)
    want = ard_mur(x, 12, 1.5, phi, a, got.experiment.b, min_iter=3, max_iter=200, tol2=1e12)
    assert got.i == want.i == 4 and len(got.obj_history) == 6
    lam = ard_lambda(got.w, got.h, a, got.experiment.b)
    rel = np.max(np.abs(got.relevance - ard_relevance(lam, x.shape, a, got.experiment.b)) / ard_relevance(lam, x.shape, a, got.experiment.b))
    print(f"ard stop: relevance vs the returned factors {rel:.2e}, wh_error {wh_error(got.w, got.h, want.w, want.h, x):.2e}")
    assert rel <= 1e-9                                             # (relevance = lambda / floor - 1: lambda's 1e-10 and a little cancellation)
    assert objective_error(got.obj_history[-1], x, got.w, got.h, lam, 1.5, phi, a, got.experiment.b) <= OBJ_RTOL


# ---- 5. determinism and isolation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted_run", [False, True])
def test_two_runs_bit_identical(weighted_run):
    x = run_data(5)
    kw = dict(weights=log_uniform_weights(x.shape, seed=11).astype(np.float64)) if weighted_run else {}
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(_ard(x.copy(), 24, beta=0.5, phi=0.5, min_iter=15, max_iter=15, **kw))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))
    assert np.array_equal(out[0].relevance, out[1].relevance) and out[0].k_eff == out[1].k_eff


def _beta_run(eng, w0, h0, lw=0.0, lh=0.0, steps=2):
    from nmf_amd import _lib as L
    eng.set_factors(w0, h0)
    eng.mur_run(L.BETA, lw, lh, NEVER, 0, 0, 0, steps)
    eng.mur_finish(L.BETA, NEVER, 0, 0, steps)
    return eng.get_factors() + (eng.objectives(0, steps + 1),)


def test_clear_ard_leaves_a_handle_that_runs_like_a_fresh_one():
    from nmf_amd.engine import Engine
    v, w0, h0 = make_inputs(300, 200, 33, seed=21)
    with Engine(300, 200, 33) as eng:
        eng.upload_v(v)
        eng.set_beta(0.5)
        eng.set_ard(PHI, A, 0.7)
        with_ard = _beta_run(eng, w0, h0)
        eng.set_beta(1.5)                                          # keeps ARD; the relevances are recomputed
        other_beta = _beta_run(eng, w0, h0)
        eng.clear_ard()
        got = _beta_run(eng, w0, h0, 0.05, 0.02)                   # ... and lambda is accepted again
    with Engine(300, 200, 33) as fresh:
        fresh.upload_v(v)
        fresh.set_beta(1.5)
        want = _beta_run(fresh, w0, h0, 0.05, 0.02)
        fresh.set_ard(PHI, A, 0.7)
        want_other = _beta_run(fresh, w0, h0)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    for a, b in zip(other_beta, want_other):
        assert np.array_equal(a, b)
    assert not np.array_equal(with_ard[0], other_beta[0])


def test_error_codes_at_the_abi():
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    lib = L.require_gpu()
    assert lib.nmfx_version() >= 360
    v, w0, h0 = make_inputs(200, 160, 8, seed=9)
    lam = np.empty(8)
    lam_p = lam.ctypes.data_as(C.c_void_p)
    with Engine(200, 160, 8) as eng:
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        h = eng.h
        assert lib.nmfx_set_ard(h, 0.1, 5.0, 1.0) == L.NMFX_E_STATE and b"beta" in lib.nmfx_last_error(h)      # no beta yet
        assert lib.nmfx_get_relevance(h, lam_p) == L.NMFX_E_STATE
        eng.set_beta(0.5)
        for bad in ((0.0, 5.0, 1.0), (-1.0, 5.0, 1.0), (0.1, 0.0, 1.0), (0.1, 5.0, 0.0), (float("nan"), 5.0, 1.0),
                    (0.1, float("inf"), 1.0), (0.1, 5.0, float("nan"))):
            assert lib.nmfx_set_ard(h, *bad) == L.NMFX_E_ARG, bad
        plain = _beta_run(eng, w0, h0, 0.1, 0.0)                   # ... which stored nothing: lambda is still accepted
        eng.set_ard(0.1, 5.0, 1.0)
        eng.set_factors(w0, h0)
        for args in ((L.BETA, 0.1, 0.0), (L.BETA, 0.0, 0.1), (L.KL, 0.0, 0.0), (L.EU, 0.0, 0.0), (L.IS, 0.0, 0.0)):
            rc = lib.nmfx_mur_run(h, args[0], args[1], args[2], NEVER, 0.0, 0.0, 0, 1)
            assert rc == L.NMFX_E_ARG and b"relevance" in lib.nmfx_last_error(h), args
        assert lib.nmfx_mur_finish(h, L.KL, NEVER, 0.0, 0.0, 0) == L.NMFX_E_ARG
        i64, dbl = C.c_int64(), C.c_double()
        calls = {
            "mur_phase_a": lambda: lib.nmfx_mur_phase_a(h, L.EU, 0.0, 0),
            "mur_phase_b": lambda: lib.nmfx_mur_phase_b(h, L.EU, 0.0, NEVER, 0.0, 0.0, 0),
            "mur_finish_a": lambda: lib.nmfx_mur_finish_a(h, L.EU, 0),
            "mur_run_sharded": lambda: lib.nmfx_mur_run_sharded(h, L.EU, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1),
            "mur_pair_run": lambda: lib.nmfx_mur_pair_run(h, (C.c_double * 2)(0, 0), (C.c_double * 2)(0, 0), NEVER, 0.0, 0.0, 0, 1),
            "anls_run": lambda: lib.nmfx_anls_run(h, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1),
            "profile_repeat": lambda: lib.nmfx_profile_repeat(h, b"wphase", L.EU, 1, C.byref(dbl)),
        }
        for name, call in calls.items():
            rc = call()
            msg = lib.nmfx_last_error(h)
            assert rc == L.NMFX_E_STATE and b"nmfx_set_ard" in msg, (name, rc, msg)
            st = eng.state()
            assert st[0] == 0 and st[2] == 0, (name, st)          # nothing was recorded, nothing stopped
        eng.clear_ard()
        again = _beta_run(eng, w0, h0, 0.1, 0.0)
        for a, b in zip(plain, again):
            assert np.array_equal(a, b)

    xs = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 4)
    with Engine.for_sparse(xs, 4) as eng:                         # a sparse handle
        assert lib.nmfx_set_ard(eng.h, 0.1, 5.0, 1.0) == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(eng.h)
    with Engine(200, 160, 200) as eng:                            # k > 128
        assert lib.nmfx_set_ard(eng.h, 0.1, 5.0, 1.0) == L.NMFX_E_ARG and b"128" in lib.nmfx_last_error(eng.h)
