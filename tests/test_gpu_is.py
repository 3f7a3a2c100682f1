"""MUR with the Itakura-Saito divergence on the device (kernels_phase.hip dense, kernels_sparse.hip masked) against the float64
statement of tests/is_ref.py.  Runs only on a real MI355X (`-m gpu`).

Bars.  Half-steps: the exact-f32 KL bar of tests/mur_step.py (2e-5) -- the square root halves the relative error of the
quotient of sums, the q^2 of the numerator doubles it, so IS sits in KL's class.  Recorded objective: mur_step.OBJ_RTOL
(1e-5) dense, 1e-6 masked (the KL bar of the sparse path, summed per entry in f64).  Whole runs: the project's WH_TOL.
Every comparison prints its figure before it asserts."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from gpu_common import WH_TOL, wh_error
from is_ref import is_h_step, is_mur, is_objective, is_w_step
from mur_step import BARS, NEVER, OBJ_RTOL, compare, make_inputs
from oracle import nmf_ref as R

pytestmark = pytest.mark.gpu

STEP_BAR = BARS[("f32", "kl")]          # 2e-5
OBJ_DENSE = OBJ_RTOL                    # 1e-5
OBJ_MASKED = 1e-6


def _mur(*a, **kw):
    from nmf_amd.mur import mur
    return mur(*a, distance_type="is", **kw)


def positive_planted(m, n, k, seed):
    return R.planted_matrix(m, n, k, seed=seed, dtype=np.float64) + 0.01


def drive(eng, w0, h0, lw, lh, steps=(1, 2)):
    from nmf_amd import _lib as L
    out = {}
    for s in steps:
        eng.set_factors(w0, h0)
        eng.mur_run(L.IS, lw, lh, NEVER, 0, 0, 0, s)
        eng.mur_finish(L.IS, NEVER, 0, 0, s)
        w, h = eng.get_factors()
        out[s] = (w, h, eng.objectives(0, s + 1))
    return out


def judge_steps(x, mask, w0, h0, runs, lw, lh, obj_bar, tag):
    fails, worst, iterate = [], {}, {0: (w0, h0)}
    for s in sorted(runs):
        ws, hs, _ = runs[s]
        wp, hp = iterate[s - 1]
        for label, dev, ref in ((f"W{s}", ws, is_w_step(x, wp, hp, lw, mask)), (f"H{s}", hs, is_h_step(x, ws, hp, lh, mask))):
            err, msg = compare(f"{tag} {label}", dev, ref, STEP_BAR)
            worst[label] = err
            if msg:
                fails.append(msg)
        iterate[s] = (ws, hs)
    for s, (_, _, hist) in sorted(runs.items()):
        for i in range(s + 1):
            want = is_objective(x, *iterate[i], mask)
            rel = abs(float(hist[i]) - want) / abs(want)
            worst[f"obj[{i}]/{s}"] = rel
            if not rel <= obj_bar:
                fails.append(f"{tag} obj[{i}] of the {s}-step run: recorded {hist[i]!r}, float64 {want!r}: rel {rel:.3e} > {obj_bar:.0e}")
    print(f"IS {tag}: worst relative errors", {key: f"{val:.2e}" for key, val in worst.items()})
    assert not fails, "\n".join(fails)


# ---- 1. half-steps element by element ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,lw,lh", [(127, 1, 3, 0.0, 0.0), (700, 600, 16, 0.05, 0.0), (300, 200, 20, 0.0, 0.1),
                                         (300, 200, 33, 0.0, 0.1), (257, 130, 64, 0.1, 0.05), (700, 600, 100, 0.0, 0.0),
                                         (640, 384, 128, 0.02, 0.3)])
def test_dense_half_steps_element_by_element(m, n, k, lw, lh):
    from nmf_amd.engine import Engine
    v, w0, h0 = make_inputs(m, n, k, seed=1000 + k)
    with Engine(m, n, k) as eng:
        eng.upload_v(v)
        runs = drive(eng, w0, h0, lw, lh)
    judge_steps(v.astype(np.float64), None, w0, h0, runs, lw, lh, OBJ_DENSE, f"dense {m}x{n} k={k}")


def masked_case(seed):
    """400 x 600, ~30 % observed: rows 1 and 2 / column 3 unobserved, row 0 and column 0 fully observed (600 and 400 > 256:
    pieces and fixup); strictly positive f32 values, garbage outside the mask."""
    rng = np.random.default_rng(seed)
    m_, n_ = 400, 600
    x = rng.uniform(0.05, 1.0, (m_, n_)).astype(np.float32).astype(np.float64)
    mask = rng.random((m_, n_)) < 0.3
    mask[0, :] = True
    mask[:, 0] = True
    mask[1:3, :] = False
    mask[:, 3] = False
    return x, mask


@pytest.mark.parametrize("kind", ["dense_x", "sparse_x"])
@pytest.mark.parametrize("k,lw,lh", [(12, 0.0, 0.0), (40, 0.05, 0.1), (200, 0.0, 0.02)])
def test_masked_half_steps_element_by_element(kind, k, lw, lh):
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    x, mask = masked_case(k)
    rng = np.random.default_rng(100 + k)
    w0 = rng.uniform(0.1, 1.0, (x.shape[0], k)).astype(np.float32).astype(np.float64)
    h0 = rng.uniform(0.1, 1.0, (k, x.shape[1])).astype(np.float32).astype(np.float64)
    data = np.where(mask, x, np.nan) if kind == "dense_x" else sp.csr_matrix(np.where(mask, x, 0.0))
    with Engine.for_sparse(masked.observed(data, mask, k), k, masked=True) as eng:
        runs = drive(eng, w0, h0, lw, lh)
    judge_steps(x, mask, w0, h0, runs, lw, lh, OBJ_MASKED, f"masked {kind} k={k}")
    ws, hs, _ = runs[2]
    assert (ws[1:3] == 0).all() and (hs[:, 3] == 0).all()           # no observed entry: exactly 0, no NaN


# ---- 2. whole runs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lw,lh", [(0.0, 0.0), (0.05, 0.02)])
def test_dense_run_against_the_float64_run(lw, lh):
    v = positive_planted(300, 220, 7, seed=11)
    kw = dict(min_iter=30, max_iter=30, lambda_w=lw, lambda_h=lh)
    np.random.seed(4)
    got = _mur(v.copy(), 7, **kw)
    np.random.seed(4)
    want = is_mur(v, 7, **kw)
    assert got.i == want.i == 29 and len(got.obj_history) == len(want.obj_history) == 31
    err = wh_error(got.w, got.h, want.w, want.h, v)
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    xd = v.astype(np.float32).astype(np.float64)                 # the values the device holds
    host = is_objective(xd, got.w, got.h)
    own = abs(got.obj_history[-1] - host) / abs(host)
    print(f"IS dense run lw={lw}: wh_error {err:.2e}, history rel {rel:.2e}, recorded vs float64 of the factors {own:.2e}")
    assert err < WH_TOL
    assert rel <= OBJ_DENSE and own <= OBJ_DENSE
    if lw == 0.0 and lh == 0.0:
        h = np.asarray(got.obj_history)
        assert np.all(h[1:] <= h[:-1] * (1 + OBJ_DENSE)), np.diff(h).max()
    assert got.experiment.distance_type == "is" and (got.w >= 0).all() and (got.h >= 0).all()


@pytest.mark.parametrize("lw,lh", [(0.0, 0.0), (0.02, 0.0)])
def test_masked_run_against_the_float64_run(lw, lh):
    rng = np.random.RandomState(7)
    x = positive_planted(400, 300, 6, seed=2)
    m = rng.rand(*x.shape) < 0.3
    xn = np.where(m, x, np.nan)
    xn[~m & (rng.rand(*x.shape) < 0.5)] = -3.0
    kw = dict(min_iter=30, max_iter=30, lambda_w=lw, lambda_h=lh)
    np.random.seed(9)
    got = _mur(xn, 6, mask=m, **kw)
    np.random.seed(9)
    want = is_mur(x, 6, m, **kw)
    assert got.i == want.i == 29 and len(got.obj_history) == 31
    d = np.where(m, got.w @ got.h - want.w @ want.h, 0.0)
    err = np.linalg.norm(d) / np.linalg.norm(np.where(m, x, 0.0))
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    from nmf_amd import masked
    host = masked.objective(x.astype(np.float32).astype(np.float64), got.w, got.h, m, "is")
    own = abs(got.obj_history[-1] - host) / abs(host)
    print(f"IS masked run lw={lw}: observed error {err:.2e}, history rel {rel:.2e}, recorded vs float64 of the factors {own:.2e}")
    assert err < WH_TOL
    assert own <= OBJ_MASKED
    assert rel <= OBJ_MASKED
    if lw == 0.0:
        h = np.asarray(got.obj_history)
        assert np.all(h[1:] <= h[:-1] * (1 + OBJ_MASKED))


@pytest.mark.parametrize("form", ["dense", "masked"])
def test_stop_rule_fires_where_the_float64_run_stops(form):
    x = positive_planted(250, 200, 5, seed=3)
    m = np.random.RandomState(1).rand(*x.shape) < 0.5 if form == "masked" else None
    kw = dict(min_iter=5, max_iter=400, tol1=1e-5, tol2=0.5)
    np.random.seed(2)
    want = is_mur(x, 5, m, **kw)
    np.random.seed(2)
    got = _mur(x.copy(), 5, **kw) if m is None else _mur(x, 5, mask=m, **kw)
    h = np.asarray(want.obj_history)
    print(f"IS stop ({form}): float64 run stops at i = {want.i}; decreases around the stop {h[-3] - h[-2]:.4f}, {h[-2] - h[-1]:.4f}; device i = {got.i}")
    assert want.trace["stop_rule"] == 2 and 5 < want.i < 399
    assert got.i == want.i and len(got.obj_history) == len(want.obj_history) == got.i + 2
    # the factors of the pair at the stop (the W buffer is chosen from the stop index: the launches queued behind it did nothing)
    d = got.w @ got.h - want.w @ want.h
    err = np.linalg.norm(d if m is None else np.where(m, d, 0.0)) / np.linalg.norm(x if m is None else np.where(m, x, 0.0))
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    xd = x.astype(np.float32).astype(np.float64)                 # the values the device holds
    host = is_objective(xd, got.w, got.h, m)
    own = abs(got.obj_history[-1] - host) / abs(host)
    print(f"IS stop ({form}): factors at the stop vs the float64 run {err:.2e}, history rel {rel:.2e} (over {got.i + 1} "
          f"iterations, not asserted), recorded vs float64 of the returned factors {own:.2e}")
    assert err < WH_TOL and own <= (OBJ_DENSE if m is None else OBJ_MASKED)


def test_all_ones_mask_agrees_with_the_dense_run():
    v = positive_planted(300, 220, 7, seed=21)
    kw = dict(min_iter=30, max_iter=30, lambda_w=0.01)
    np.random.seed(5)
    dense = _mur(v.copy(), 7, **kw)
    np.random.seed(5)
    full = _mur(v, 7, mask=np.ones(v.shape, dtype=bool), **kw)
    err = wh_error(full.w, full.h, dense.w, dense.h, v)
    print(f"IS all-ones mask vs dense: wh_error {err:.2e}")
    assert err < WH_TOL and full.i == dense.i
    np.testing.assert_allclose(full.obj_history, dense.obj_history, rtol=OBJ_DENSE)


@pytest.mark.parametrize("form", ["dense", "masked"])
def test_two_runs_bit_identical(form):
    x, mask = masked_case(21)
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(_mur(x.copy(), 24, min_iter=15, max_iter=15) if form == "dense"
                   else _mur(x, 24, mask=mask, min_iter=15, max_iter=15))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))


def test_nmf_class_and_grid_run_is():
    from nmf_amd import NMF
    from nmf_amd.grid import factorize_grid
    v = positive_planted(200, 150, 4, seed=8)
    np.random.seed(3)
    nmf = NMF(v.copy(), 4)
    nmf.factorize("mur", distance_type="is", min_iter=10, max_iter=10, lambda_h=0.01)
    np.random.seed(3)
    runs = factorize_grid(v.copy(), "mur", features=(4,), lambda_h=(0.01,), distance_type="is", min_iter=10, max_iter=10)
    assert len(runs) == 1 and np.array_equal(runs[0][1].w, nmf.w) and np.array_equal(runs[0][1].h, nmf.h)
    assert nmf.results.experiment.distance_type == "is" and len(nmf.results.obj_history) == 11


# ---- 3. the ABI's refusals -------------------------------------------------------------------------------------------------
def test_refusals_at_the_abi():
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    lib = L.require_gpu()
    rs = np.random.RandomState(0)

    def refused(rc, h):
        return rc == L.NMFX_E_ARG and b"IS" in lib.nmfx_last_error(h)

    xs = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 4)
    with Engine.for_sparse(xs, 4) as eng:                         # an unmasked sparse handle
        eng.set_factors(np.abs(rs.randn(64, 4)), np.abs(rs.randn(4, 48)))
        assert refused(lib.nmfx_mur_run(eng.h, L.IS, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1), eng.h)
        assert refused(lib.nmfx_mur_finish(eng.h, L.IS, NEVER, 0.0, 0.0, 0), eng.h)
        assert eng.state()[2] == 0                                # nothing was recorded
    v = rs.uniform(0.1, 1.0, (200, 160))
    with Engine(200, 160, 129) as eng:                            # k > 128 on a dense handle
        eng.upload_v(v)
        eng.set_factors(np.abs(rs.randn(200, 129)), np.abs(rs.randn(129, 160)))
        assert refused(lib.nmfx_mur_run(eng.h, L.IS, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1), eng.h)
        assert eng.state()[2] == 0
    with Engine(200, 160, 8) as eng:                              # the phase entry points, the profiler, the f64 referee
        eng.upload_v(v)
        eng.set_factors(np.abs(rs.randn(200, 8)), np.abs(rs.randn(8, 160)))
        assert refused(lib.nmfx_mur_phase_a(eng.h, L.IS, 0.0, 0), eng.h)
        assert refused(lib.nmfx_mur_phase_b(eng.h, L.IS, 0.0, NEVER, 0.0, 0.0, 0), eng.h)
        assert refused(lib.nmfx_mur_finish_a(eng.h, L.IS, 0), eng.h)
        ms = C.c_double()
        assert refused(lib.nmfx_profile_repeat(eng.h, b"wphase", L.IS, 1, C.byref(ms)), eng.h)
        assert eng.state()[2] == 0
        eng.mur_run(L.IS, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1)
        out = C.c_double()
        assert refused(lib.nmfx_objective_f64(eng.h, C.byref(out)), eng.h)
    with Engine(200, 160, 64) as eng:                             # a handle in the split-bf16 mode: IS says that it runs exact f32
        eng.set_precision("bf16")
        assert eng.precision() == "bf16"
        eng.upload_v(v)
        eng.set_factors(np.abs(rs.randn(200, 64)), np.abs(rs.randn(64, 160)))
        assert b"Itakura" not in lib.nmfx_get_note(eng.h)
        eng.mur_run(L.IS, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 1)
        note = lib.nmfx_get_note(eng.h)
        assert b"Itakura-Saito" in note and b"exact-f32" in note, note


# ---- 4. a size-level case --------------------------------------------------------------------------------------------------
def test_size_level_case():
    m, n, k = 16384, 8192, 64
    rng = np.random.default_rng(0)
    a = rng.uniform(0.0, 1.0, (m, 16)).astype(np.float32)
    b = rng.uniform(0.0, 1.0, (16, n)).astype(np.float32)
    v = a @ b / 16 + np.float32(0.01) + np.float32(0.01) * rng.random((m, n), dtype=np.float32)
    np.random.seed(0)
    res = _mur(v, k, min_iter=10, max_iter=5)
    obj = np.asarray(res.obj_history)
    assert len(obj) == 6 and np.all(np.isfinite(obj)) and np.all(np.diff(obj) < 0), obj
    assert np.isfinite(res.w).all() and np.isfinite(res.h).all() and (res.w >= 0).all() and (res.h >= 0).all()
    host = is_objective(v, res.w, res.h)
    rel = abs(obj[-1] - host) / abs(host)
    print(f"IS 16384 x 8192 k = 64: objectives {obj}, recorded vs blocked float64 {rel:.2e}")
    assert rel <= OBJ_DENSE
