"""MUR with per-entry weights on the device (kernels_phase.hip) against the float64 statement of tests/weighted_ref.py.
Runs only on a real MI355X (`-m gpu`).

Bars.  Half-steps: mur_step.BARS[("f32", kind)] = 2e-5, the project's bar for exact-f32 kernels; IS takes the KL entry as
tests/test_gpu_is.py argues (the square root halves the relative error of the quotient of sums, the q^2 doubles it).
Recorded objective: mur_step.OBJ_RTOL (1e-5), for eu / kl relative to max(|objective|, OBJ_FLOOR x the weighted data
scale 1/2 Sum om v^2 / Sum om v) -- the OBJ_FLOOR convention of mur_step.check_steps.  Whole runs: the project's WH_TOL.
Every comparison prints its figure before it asserts.

The measured maxima belong in DESIGN.md 4.4 (not measured yet)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from gpu_common import WH_TOL, wh_error
from mur_step import BARS, NEVER, OBJ_FLOOR, OBJ_RTOL, compare, make_inputs
from oracle import nmf_ref as R
from weighted_cases import log_uniform_weights, run_case, stop_margins, stop_run
from weighted_ref import weighted_h_step, weighted_mur, weighted_objective, weighted_w_step

pytestmark = pytest.mark.gpu

KINDS = ("eu", "kl", "is")


def _code(kind):
    from nmf_amd import _lib as L
    return {"eu": L.EU, "kl": L.KL, "is": L.IS}[kind]


def _bar(kind):
    return BARS[("f32", "kl" if kind == "is" else kind)]


def _mur(*a, **kw):
    from nmf_amd.mur import mur
    return mur(*a, **kw)


def drive(eng, kind, w0, h0, lw, lh, steps=(1, 2)):
    """The calls nmf_amd.mur.mur makes, with the stop rule off: {s: (W_s, H_s, recorded objectives 0 .. s)}."""
    out = {}
    for s in steps:
        eng.set_factors(w0, h0)
        eng.mur_run(_code(kind), lw, lh, NEVER, 0, 0, 0, s)
        eng.mur_finish(_code(kind), NEVER, 0, 0, s)
        w, h = eng.get_factors()
        out[s] = (w, h, eng.objectives(0, s + 1))
    return out


# ---- 1. half-steps element by element ------------------------------------------------------------------------------------
SHAPES = [(127, 1, 3, 0.0, 0.0), (700, 600, 16, 0.05, 0.0), (300, 200, 20, 0.0, 0.1), (300, 200, 33, 0.0, 0.1),
          (257, 130, 64, 0.1, 0.05), (700, 600, 100, 0.0, 0.0), (640, 384, 128, 0.02, 0.3)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n,k,lw,lh", SHAPES)
def test_half_steps_element_by_element(kind, m, n, k, lw, lh):
    from nmf_amd import weighted
    from nmf_amd.engine import Engine
    v, w0, h0 = make_inputs(m, n, k, seed=2000 + k)
    edges = n >= 8
    om = log_uniform_weights((m, n), seed=3000 + k, edges=edges)
    x = v.astype(np.float64)
    if edges:
        x[om == 0] = np.nan                                        # never read: the device receives 0 there
    x32, w32 = weighted.prepare(x, om, k, kind)
    with Engine(m, n, k) as eng:
        eng.upload_v(x32)
        eng.upload_weights(w32)
        runs = drive(eng, kind, w0, h0, lw, lh)
    omd = om.astype(np.float64)
    tag = f"weighted {kind} {m}x{n} k={k}"
    fails, worst, iterate = [], {}, {0: (w0, h0)}
    for s in sorted(runs):
        ws, hs, _ = runs[s]
        wp, hp = iterate[s - 1]
        for label, dev, ref in ((f"W{s}", ws, weighted_w_step(kind, x, omd, wp, hp, lw)),
                                (f"H{s}", hs, weighted_h_step(kind, x, omd, ws, hp, lh))):
            err, msg = compare(f"{tag} {label}", dev, ref, _bar(kind))
            worst[label] = err
            if msg:
                fails.append(msg)
        iterate[s] = (ws, hs)
    xo = np.where(omd > 0, x, 0.0)
    scale = {"eu": OBJ_FLOOR * 0.5 * float(np.sum(omd * xo * xo)), "kl": OBJ_FLOOR * float(np.sum(omd * xo)), "is": 0.0}[kind]
    for s, (_, _, hist) in sorted(runs.items()):
        for i in range(s + 1):
            want = weighted_objective(kind, x, omd, *iterate[i])
            rel = abs(float(hist[i]) - want) / max(abs(want), scale)
            worst[f"obj[{i}]/{s}"] = rel
            if not rel <= OBJ_RTOL:
                fails.append(f"{tag} obj[{i}] of the {s}-step run: recorded {hist[i]!r}, float64 {want!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    print(f"{tag}: worst relative errors", {key: f"{val:.2e}" for key, val in worst.items()})
    assert not fails, "\n".join(fails)
    if edges:                                                      # no weight at all: exactly 0, no NaN
        for s in runs:
            assert (runs[s][0][1:3] == 0).all() and (runs[s][1][:, 3] == 0).all()


# ---- 2. agreement with the existing paths ----------------------------------------------------------------------------------
def positive_planted(m, n, k, seed):
    return R.planted_matrix(m, n, k, seed=seed, dtype=np.float64) + 0.01


@pytest.mark.parametrize("kind", KINDS)
def test_zero_one_weights_agree_with_the_masked_path(kind):
    x = positive_planted(400, 300, 6, seed=2)
    m = np.random.RandomState(7).rand(*x.shape) < 0.3
    kw = dict(distance_type=kind, min_iter=30, max_iter=30, lambda_w=0.01)
    np.random.seed(9)
    got = _mur(x, 6, weights=m.astype(np.float32), **kw)
    np.random.seed(9)
    want = _mur(x, 6, mask=m, **kw)
    d = np.where(m, got.w @ got.h - want.w @ want.h, 0.0)
    seen = np.linalg.norm(d) / np.linalg.norm(np.where(m, x, 0.0))
    err = wh_error(got.w, got.h, want.w, want.h, x)
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    print(f"weights 0/1 vs mask= ({kind}): wh_error {err:.2e} (on the observed cells {seen:.2e}), history rel {rel:.2e}")
    assert err < WH_TOL
    assert got.i == want.i and len(got.obj_history) == len(want.obj_history)


@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_weights_agree_with_the_dense_f32_path(kind, monkeypatch):
    monkeypatch.setenv("NMFX_PRECISION", "f32")
    x = positive_planted(300, 220, 7, seed=21)
    kw = dict(distance_type=kind, min_iter=30, max_iter=30, lambda_h=0.01)
    np.random.seed(5)
    got = _mur(x, 7, weights=np.ones(x.shape), **kw)
    np.random.seed(5)
    want = _mur(x.copy(), 7, **kw)
    err = wh_error(got.w, got.h, want.w, want.h, x)
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    print(f"all-ones weights vs the dense f32 path ({kind}): wh_error {err:.2e}, history rel {rel:.2e}")
    assert err < WH_TOL
    assert got.i == want.i and len(got.obj_history) == len(want.obj_history)


# ---- 3. whole runs against the yardstick's own float64 run -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lw,lh", [(0.0, 0.0), (0.05, 0.02)])
def test_run_against_the_float64_run(kind, lw, lh):
    from nmf_amd import weighted
    x, om = run_case()
    kw = dict(distance_type=kind, min_iter=30, max_iter=30, lambda_w=lw, lambda_h=lh)
    np.random.seed(4)
    got = _mur(x, 5, weights=om, **kw)
    np.random.seed(4)
    want = weighted_mur(x, om, 5, **kw)
    assert got.i == want.i == 29 and len(got.obj_history) == len(want.obj_history) == 31
    xo = np.where(om > 0, x, 0.0)
    err = wh_error(got.w, got.h, want.w, want.h, xo)
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    xd = np.where(om > 0, x, np.nan).astype(np.float32).astype(np.float64)         # the values the device holds
    host = weighted.objective(xd, got.w, got.h, om.astype(np.float32), kind)
    own = abs(got.obj_history[-1] - host) / abs(host)
    print(f"weighted run ({kind}, lw={lw}): wh_error {err:.2e}, history rel {rel:.2e}, recorded vs float64 of the factors {own:.2e}")
    assert err < WH_TOL
    assert rel <= OBJ_RTOL and own <= OBJ_RTOL
    if lw == 0.0 and lh == 0.0:
        h = np.asarray(got.obj_history)
        assert np.all(h[1:] <= h[:-1] * (1 + OBJ_RTOL)), np.diff(h).max()
    assert got.experiment.distance_type == kind and (got.w >= 0).all() and (got.h >= 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_stop_rule_fires_where_the_float64_run_stops(kind):
    x, om, seed, kw, want = stop_run(kind)
    margins = stop_margins(want, kw["tol2"])
    print(f"weighted stop ({kind}): float64 run stops at i = {want.i}, margins of its last two decisions {margins} (x OBJ_RTOL x objective)")
    assert want.trace["stop_rule"] == 2 and kw["min_iter"] < want.i < 399 and min(margins) > 10      # the yardstick alone
    np.random.seed(seed)
    got = _mur(x, 5, weights=om, distance_type=kind, **kw)
    err = wh_error(got.w, got.h, want.w, want.h, np.where(om > 0, x, 0.0))
    print(f"weighted stop ({kind}): device i = {got.i}, factors at the stop vs the float64 run {err:.2e}")
    assert got.i == want.i and len(got.obj_history) == len(want.obj_history) == got.i + 2
    assert err < WH_TOL


# ---- 4. contract -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_bit_identical(kind):
    x, om = run_case(5)
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(_mur(x, 24, weights=om, distance_type=kind, min_iter=15, max_iter=15))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))


@pytest.mark.parametrize("kind,k", [("eu", 64), ("kl", 64), ("is", 12)])
def test_clear_weights_restores_the_unweighted_results(kind, k):
    from nmf_amd.engine import Engine
    v, w0, h0 = make_inputs(300, 200, k, seed=77)
    om = log_uniform_weights(v.shape, seed=78)
    with Engine(300, 200, k) as eng:
        eng.upload_v(v)
        before = drive(eng, kind, w0, h0, 0.01, 0.02, steps=(3,))[3]
        note = eng.note()
        eng.upload_weights(om)
        assert "exact-f32" in eng.note() and "weights" in eng.note(), eng.note()
        with_weights = drive(eng, kind, w0, h0, 0.01, 0.02, steps=(3,))[3]
        eng.clear_weights()
        eng.clear_weights()                                        # (idempotent)
        assert eng.note() == note
        after = drive(eng, kind, w0, h0, 0.01, 0.02, steps=(3,))[3]
    assert not np.array_equal(with_weights[0], before[0])
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def test_refusals_at_the_abi():
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    lib = L.require_gpu()
    rs = np.random.RandomState(0)
    om = np.ones((200, 160), dtype=np.float32)

    xs = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 4)
    with Engine.for_sparse(xs, 4) as eng:                         # a sparse handle
        rc = lib.nmfx_upload_weights(eng.h, om.ctypes.data_as(C.c_void_p), L.F32, 48, 0, 64)
        assert rc == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(eng.h)
    with Engine(200, 160, 129) as eng:                            # k > 128
        rc = lib.nmfx_upload_weights(eng.h, om.ctypes.data_as(C.c_void_p), L.F32, 160, 0, 200)
        assert rc == L.NMFX_E_ARG and b"128" in lib.nmfx_last_error(eng.h)

    v = rs.uniform(0.1, 1.0, (200, 160))
    with Engine(200, 160, 128) as eng:                            # (k = 128, split-bf16 by default: where pair mode would run)
        eng.upload_v(v)
        eng.upload_weights(om)
        eng.set_factors(np.abs(rs.randn(200, 128)), np.abs(rs.randn(128, 160)))
        h = eng.h
        i64, dbl, i32 = C.c_int64(), C.c_double(), C.c_int()
        two = (C.c_double * 2)(0.0, 0.0)
        u, s, vt = np.empty((200, 4)), np.empty(4), np.empty((4, 160))
        calls = {
            "mur_phase_a": lambda: lib.nmfx_mur_phase_a(h, L.EU, 0.0, 0),
            "mur_phase_b": lambda: lib.nmfx_mur_phase_b(h, L.EU, 0.0, NEVER, 0.0, 0.0, 0),
            "mur_finish_a": lambda: lib.nmfx_mur_finish_a(h, L.EU, 0),
            "mur_finish_b": lambda: lib.nmfx_mur_finish_b(h, NEVER, 0.0, 0.0, 0),
            "mur_chunk_info": lambda: lib.nmfx_mur_chunk_info(h, L.EU, C.byref(i64), C.byref(i64), C.byref(i64)),
            "mur_phase_a_head": lambda: lib.nmfx_mur_phase_a_head(h, L.EU, 0.0, 0),
            "mur_phase_a_cols": lambda: lib.nmfx_mur_phase_a_cols(h, L.EU, 0, 128),
            "mur_slice_info": lambda: lib.nmfx_mur_slice_info(h, L.EU, 1, C.byref(i64), C.byref(i64)),
            "mur_phase_b_slice": lambda: lib.nmfx_mur_phase_b_slice(h, L.EU, 0.0, NEVER, 0.0, 0.0, 0, 0, 64),
            "mur_phase_b_rest": lambda: lib.nmfx_mur_phase_b_rest(h, L.EU, 0, 64),
            "mur_run_sharded": lambda: lib.nmfx_mur_run_sharded(h, L.EU, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1),
            "mur_finish_sharded": lambda: lib.nmfx_mur_finish_sharded(h, L.EU, NEVER, 0.0, 0.0, 0),
            "mur_pair_run": lambda: lib.nmfx_mur_pair_run(h, two, two, NEVER, 0.0, 0.0, 0, 1),
            "mur_pair_finish": lambda: lib.nmfx_mur_pair_finish(h, NEVER, 0.0, 0.0, 0),
            "objective_f64": lambda: lib.nmfx_objective_f64(h, C.byref(dbl)),
            "profile_repeat": lambda: lib.nmfx_profile_repeat(h, b"wphase", L.EU, 1, C.byref(dbl)),
            "aoadmm_run": lambda: lib.nmfx_aoadmm_run(h, L.EU, 0, 0.0, 0, 0.0, 5, NEVER, 0.0, 0.0, 0, 1),
            "aoadmm_phase_h_products": lambda: lib.nmfx_aoadmm_phase_h_products(h, 0),
            "aoadmm_finish": lambda: lib.nmfx_aoadmm_finish(h, NEVER, 0.0, 0.0, 0),
            "objective_partial": lambda: lib.nmfx_objective_partial(h),
            "admm_run": lambda: lib.nmfx_admm_run(h, L.EU, 1.0, 0, 0.0, 0, 0.0, NEVER, 0.0, 0.0, 0, 1),
            "admm_phase_products": lambda: lib.nmfx_admm_phase_products(h, L.EU, 1.0, 0, 0, 0),
            "anls_run": lambda: lib.nmfx_anls_run(h, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1),
            "anls_phase_objective": lambda: lib.nmfx_anls_phase_objective(h, 0),
            "topk_svd": lambda: lib.nmfx_topk_svd(h, 4, 0, 0.0, 0, 0, u.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p),
                                                  vt.ctypes.data_as(C.c_void_p), C.byref(i32), C.byref(dbl)),
        }
        for name, call in calls.items():
            rc = call()
            msg = lib.nmfx_last_error(h)
            assert rc == L.NMFX_E_ARG and b"weights" in msg, (name, rc, msg)
            st = eng.state()
            assert st[0] == 0 and st[2] == 0, (name, st)          # nothing was recorded, nothing stopped
        w_before, h_before = eng.get_factors()
        note = lib.nmfx_get_note(h)
        assert b"exact-f32" in note and b"weights" in note, note
        eng.mur_run(L.KL, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1)        # ... and the weighted run itself works on this handle
        eng.mur_finish(L.KL, NEVER, 0.0, 0.0, 1)
        assert eng.state()[2] == 2
        w_after, _ = eng.get_factors()
        assert not np.array_equal(w_before, w_after) and np.isfinite(w_after).all()
        rc = lib.nmfx_mur_run(h, 7, 0.0, 0.0, NEVER, 0.0, 0.0, 1, 1)
        assert rc == L.NMFX_E_ARG
