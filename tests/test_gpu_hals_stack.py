"""Stacked HALS on the device beyond single half-steps (tests/test_gpu_hals_stack_step.py has those): the per-problem stop
bookkeeping, the public call nmf_amd.hals.hals_stack against a float64 host loop, the entry guard, the C-ABI refusals and
factorize_grid(v, 'hals', ...)."""
import math

import numpy as np
import pytest

import anls_step as A
import hals_step as HS
import hals_stack_step as ST
from mur_step import NEVER

pytestmark = pytest.mark.gpu

M, N = 257, 200


def host_hals(v, w, h, lw, lh, sweeps, iters):
    """The float64 loop of tests/test_gpu_hals.py: (W, H, objective history of iters + 1 entries)."""
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


def host_alpha(v, w, h):
    wh = np.asarray(w, np.float32).astype(np.float64) @ np.asarray(h, np.float32).astype(np.float64)
    return float(np.vdot(np.asarray(v, np.float64), wh) / np.vdot(wh, wh))


def scaled_uniform(v, k, seed):
    rng = np.random.default_rng(seed)
    w, h = rng.uniform(0.1, 1.0, (M, k)), rng.uniform(0.1, 1.0, (k, N))
    a = math.sqrt(host_alpha(v, w, h))
    return A.f32(w * a), A.f32(h * a)


# ---- stop bookkeeping ---------------------------------------------------------------------------------------------------------
MIN_ITER, MAX_ITER, OFF = 2, 24, -1e30                   # tol2 = OFF: rule 2 never holds


@pytest.fixture(scope="module")
def stop_case():
    """Planted rank-6 data, k = (6, 1): problem 0 starts from the planted pair with every entry moved by up to 30 % (its objective
    falls by a fifth and more per iteration), problem 1 from a scaled uniform pair (a rank-1 fit stays far above).  The float64
    loops; tol1 inside the largest gap between two consecutive objectives of problem 0 from the second tested index on."""
    v, w6, h6 = A.planted(M, N, 6, 5, noise=0.0005, jitter=0.3, scale=3.0)
    starts = [(w6, h6), scaled_uniform(v, 1, 22)]
    hist = [host_hals(v, *starts[p], 0.0, 0.0, 1, MAX_ITER)[2] for p in (0, 1)]
    first = MIN_ITER + 3
    j = first + int(np.argmax(hist[0][first:-1] / hist[0][first + 1:]))
    tol1 = math.sqrt(hist[0][j] * hist[0][j + 1])
    return v, starts, hist, tol1


def test_the_stop_case_is_decided_by_a_wide_margin(stop_case):
    """On the CPU, with the float64 loops: no recorded value of either problem lies within 10 % of tol1; problem 0 crosses it
    behind min_iter and before max_iter, problem 1 stays above it."""
    _, _, hist, tol1 = stop_case
    for p in (0, 1):
        assert (np.abs(hist[p] / tol1 - 1) > 0.1).all(), p
    assert hist[0][MIN_ITER + 3] > tol1 > hist[0][-1] and hist[1].min() > tol1


def test_each_problem_keeps_its_own_stop(stop_case):
    from nmf_amd.engine import Engine
    v, starts, hist, tol1 = stop_case
    want_j = next(j for j in range(MIN_ITER + 2, MAX_ITER + 1) if hist[0][j] < tol1)         # rule 1 at loop index j - 1
    w0, h0 = ST.stack(starts, 7)
    with Engine(M, N, 7) as eng:
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        eng.hals_stack_set((6, 1))
        eng.hals_stack_run([0, 0], [0, 0], 1, MIN_ITER, tol1, OFF, 0, MAX_ITER)
        eng.hals_stack_finish(MIN_ITER, tol1, OFF, MAX_ITER)
        s0, s1 = eng.hals_stack_state(0), eng.hals_stack_state(1)
        assert eng.state()[0] == 0                       # (the handle's flag waits for ALL problems)
        obj0 = eng.hals_stack_objectives(0, 0, s0[2])
        obj1 = eng.hals_stack_objectives(1, 0, s1[2])
        kept = eng.hals_stack_get_factors(0)
        last = eng.hals_stack_get_factors(1)
        # a stack of one, run to the stop's iteration count with the rule off
        eng.set_factors(*ST.stack(starts[:1], 7))
        eng.hals_stack_set((6,))
        eng.hals_stack_run([0], [0], 1, NEVER, 0, 0, 0, want_j)
        alone = eng.hals_stack_get_factors(0)
        eng.set_factors(*ST.stack([(np.zeros((M, 6)), np.zeros((6, N))), starts[1]], 7))
        eng.hals_stack_set((6, 1))
        eng.hals_stack_run([0, 0], [0, 0], 1, NEVER, 0, 0, 0, MAX_ITER)
        alone1 = eng.hals_stack_get_factors(1)
    assert s0 == (1, want_j - 1, want_j + 1), (s0, want_j)
    assert s1 == (0, -1, MAX_ITER + 1), s1
    floor = ST.OBJ_FLOOR * 0.5 * float(np.sum(v.astype(np.float64) ** 2))      # (the trajectory tolerance of tests/test_gpu_hals.py, floored as every objective check)
    assert (np.abs(obj0 - hist[0][:want_j + 1]) <= 2e-4 * np.maximum(hist[0][:want_j + 1], floor)).all()
    assert (np.abs(obj1 - hist[1]) <= 2e-4 * np.maximum(hist[1], floor)).all()
    bar = ST.bar_of(ST.BY_NAME["kp16"])
    same = all(np.array_equal(a, b) for a, b in zip(kept, alone))
    print(f"problem 0 kept at its stop against a stack of one run to the same index: bit-identical: {same}")
    for a, b in zip(kept + last, alone + alone1):
        assert np.abs(a - b).max() <= bar * b.max()


# ---- the public call ----------------------------------------------------------------------------------------------------------
PROBLEMS = [dict(k=8, lambda_w=0.05, lambda_h=0.02), dict(k=3), dict(k=20, lambda_h=0.1)]


def public_run(v, sweeps=1):
    from nmf_amd.hals import hals_stack
    np.random.seed(5)
    res = hals_stack(v, PROBLEMS, sweeps=sweeps, max_iter=5, nndsvd_init=(False, "zero"))
    return res, list(hals_stack.last_alpha), np.random.rand(3)


@pytest.mark.parametrize("sweeps", [1, 2])
def test_public_call_matches_the_float64_loop(sweeps, capsys):
    v = ST.make_v(M, N)[0]
    keep = v.copy()
    res, alphas, after = public_run(v, sweeps)
    assert np.array_equal(v, keep) and len(res) == len(PROBLEMS)
    np.random.seed(5)                                    # the draws of consecutive hals calls: W then H, problem by problem
    for p, prob in enumerate(PROBLEMS):
        k = prob["k"]
        w0, h0 = np.random.rand(M, k), np.random.rand(k, N)
        a = host_alpha(v, w0, h0)
        assert abs(alphas[p] - a) <= 1e-6 * a, (p, alphas[p], a)
        lw, lh = prob.get("lambda_w", 0), prob.get("lambda_h", 0)
        wr, hr, hist = host_hals(v, A.f32(w0 * math.sqrt(a)), A.f32(h0 * math.sqrt(a)), lw, lh, sweeps, 5)
        r = res[p]
        assert r.w.shape == (M, k) and r.h.shape == (k, N) and (r.w >= 0).all() and (r.h >= 0).all()
        assert r.i == 4 and len(r.obj_history) == 6
        err = np.linalg.norm(r.w @ r.h - wr @ hr) / np.linalg.norm(v.astype(np.float64))
        print(f"problem {p} (k = {k}), sweeps = {sweeps}: WH error {err:.3e}")
        assert err < 1e-4, (p, err)
        np.testing.assert_allclose(r.obj_history, hist, rtol=2e-4)
        e = r.experiment
        assert (e.method, e.components, e.distance_type, e.lambda_w, e.lambda_h, e.sweeps, e.max_iter) == ("hals", k, "eu", lw, lh, sweeps, 5)
    assert np.array_equal(after, np.random.rand(3)), "the call drew more or less than consecutive hals calls"
    from nmf_amd.hals import hals_stack
    assert hals_stack.last_would_arm == [False] * len(PROBLEMS)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("[")]
    assert [l.split("]")[0] for l in lines[:15]] == [f"[{i}" for _ in PROBLEMS for i in range(5)]      # problem by problem


def test_two_identical_runs_are_bit_identical():
    v = ST.make_v(M, N)[0]
    a, _, _ = public_run(v)
    b, _, _ = public_run(v)
    for p, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.w, y.w) and np.array_equal(x.h, y.h) and np.array_equal(x.obj_history, y.obj_history), p


def test_rescale_start_off_and_an_engine_with_room():
    """rescale_start=False keeps the draws as they are; a resident engine with more components than the stack holds is taken."""
    from nmf_amd.engine import Engine
    from nmf_amd.hals import hals_stack
    v = ST.make_v(M, N)[0]
    with Engine(M, N, 64) as eng:
        eng.upload_v(v)
        np.random.seed(7)
        res = hals_stack(v, [dict(k=4), dict(k=5)], rescale_start=False, max_iter=2, nndsvd_init=(False, "zero"), engine=eng)
    assert hals_stack.last_alpha == [None, None] and [r.w.shape[1] for r in res] == [4, 5]
    np.random.seed(7)
    w0, h0 = np.random.rand(M, 4), np.random.rand(4, N)
    want = 0.5 * np.sum((v.astype(np.float64) - A.f32(w0) @ A.f32(h0)) ** 2)
    assert abs(res[0].obj_history[0] - want) <= 1e-4 * want


def test_default_start_against_single_hals_calls():
    """The definition, end to end with the default NNDSVD start: problem p of the stack against hals(x, k_p, ...) -- same
    width of handle (kp = 16, exact f32), three iterations.  The factors within the half-step bar of that width (the two
    routes to alpha agree to rounding, not to the bit); the histories within the objective bar of the decomposition."""
    from nmf_amd.hals import hals, hals_stack
    v = ST.make_v(M, N)[0]
    probs = [dict(k=3, lambda_w=0.05), dict(k=5, lambda_h=0.02)]
    res = hals_stack(v, probs, max_iter=3)
    bar, obar = ST.BARS["kp16"][1], ST.BARS["kp16"][3]
    floor = ST.OBJ_FLOOR * 0.5 * float(np.sum(v.astype(np.float64) ** 2))
    for p, prob in enumerate(probs):
        one = hals(v, prob["k"], lambda_w=prob.get("lambda_w", 0), lambda_h=prob.get("lambda_h", 0), max_iter=3)
        same = np.array_equal(one.w, res[p].w) and np.array_equal(one.h, res[p].h)
        print(f"problem {p}: factors bit-identical to the single hals call: {same}")
        assert np.abs(one.w - res[p].w).max() <= bar * one.w.max() and np.abs(one.h - res[p].h).max() <= bar * one.h.max(), p
        assert res[p].i == one.i == 2 and one.experiment == res[p].experiment
        assert (np.abs(np.array(res[p].obj_history) - np.array(one.obj_history)) <= obar * np.maximum(one.obj_history, floor)).all(), p


# ---- the entry guard and the C ABI --------------------------------------------------------------------------------------------
T = (NEVER, 1e-3, 1e-3)


def _handle(k=16):
    from nmf_amd.engine import Engine
    c = ST.BY_NAME["tail"]
    v, starts = ST.make_case(c)
    eng = Engine(M, N, k)
    eng.upload_v(v)
    eng.set_factors(*ST.stack(starts, k))
    return eng, starts


def test_the_stack_is_a_family_of_its_own():
    from nmf_amd._lib import NmfxError
    eng, starts = _handle()
    with eng as e:
        e.hals_stack_set((5, 6))
        e.hals_stack_run([0, 0], [0, 0], 1, *T, 0, 1)
        for other in (lambda: e.hals_run(0.0, 0.0, 1, *T, 1, 1), lambda: e.anls_run(0.0, 0.0, *T, 1, 1), lambda: e.mur_run(0, 0.0, 0.0, *T, 1, 1)):
            with pytest.raises(NmfxError, match="another solver"):
                other()
        with pytest.raises(NmfxError, match="nmfx_set_factors"):
            e.hals_stack_set((5, 5))                     # (the partition belongs to the run)
        e.hals_stack_run([0, 0], [0, 0], 1, *T, 1, 1)    # (the refusals changed nothing the run depends on)
        two = e.get_factors()
        e.set_factors(*ST.stack(starts, 16))
        e.hals_run(0.0, 0.0, 1, *T, 0, 1)
        with pytest.raises(NmfxError, match="another solver"):
            e.hals_stack_run([0, 0], [0, 0], 1, *T, 1, 1)
        e.set_factors(*ST.stack(starts, 16))             # the partition survives set_factors
        e.hals_stack_run([0, 0], [0, 0], 1, *T, 0, 2)
        again = e.get_factors()
    for x, y in zip(two, again):
        np.testing.assert_array_equal(x, y)


def test_c_abi_refusals():
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    import ctypes as C
    lib = L.load()
    two = (C.c_double * 2)(0.0, 0.0)
    eng, _ = _handle()
    with eng as e:
        assert lib.nmfx_hals_stack_run(e.h, two, two, 1, *T, 0, 1) == L.NMFX_E_STATE and b"nmfx_hals_stack_set" in lib.nmfx_last_error(e.h)
        for ks, word in (((10, 7), b"more than the handle's k"), ((5, 0), b"k_p >= 1"), ((5, -1), b"k_p >= 1")):
            assert lib.nmfx_hals_stack_set(e.h, len(ks), (C.c_int * len(ks))(*ks)) == L.NMFX_E_ARG and word in lib.nmfx_last_error(e.h), ks
        e.hals_stack_set((5, 6))
        neg = (C.c_double * 2)(0.0, -1.0)
        nan = (C.c_double * 2)(float("nan"), 0.0)
        for args, word in (((two, two, 0) + T + (0, 1), b"sweeps"), ((two, two, 17) + T + (0, 1), b"sweeps"), ((neg, two, 1) + T + (0, 1), b"lambda"),
                           ((two, nan, 1) + T + (0, 1), b"lambda"), ((two, two, 1) + T + (-1, 1), b"range"), ((two, two, 1) + T + (0, -1), b"range")):
            assert lib.nmfx_hals_stack_run(e.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(e.h), args
        assert lib.nmfx_hals_stack_get_state(e.h, 2, None, None, None) == L.NMFX_E_ARG
        e.hals_stack_run([0, 0], [0, 0], 1, *T, 0, 1)    # (a refused call joins no family and leaves the handle usable)
        e.upload_weights(np.ones((M, N), dtype=np.float32))
        for call in (lambda: lib.nmfx_hals_stack_run(e.h, two, two, 1, *T, 1, 1), lambda: lib.nmfx_hals_stack_set(e.h, 0, None),
                     lambda: lib.nmfx_hals_stack_terms(e.h, two), lambda: lib.nmfx_hals_stack_finish(e.h, *T, 1)):
            assert call() == L.NMFX_E_ARG and b"weights" in lib.nmfx_last_error(e.h)
    rng = np.random.default_rng(0)
    one = (C.c_int * 1)(3)
    with Engine(40, 30, 130) as big:                     # beyond 128 components
        big.upload_v(rng.uniform(0.1, 1, (40, 30)).astype(np.float32))
        big.set_factors(rng.uniform(0.1, 1, (40, 130)), rng.uniform(0.1, 1, (130, 30)))
        assert lib.nmfx_hals_stack_set(big.h, 1, one) == L.NMFX_E_ARG and b"128" in lib.nmfx_last_error(big.h)
        assert lib.nmfx_hals_stack_run(big.h, two, two, 1, *T, 0, 1) == L.NMFX_E_ARG and b"128" in lib.nmfx_last_error(big.h)
    import scipy.sparse as sp
    from nmf_amd import sparse
    xs = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 4)
    with Engine.for_sparse(xs, 4) as se:
        assert lib.nmfx_hals_stack_set(se.h, 1, one) == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(se.h)
        assert lib.nmfx_hals_stack_run(se.h, two, two, 1, *T, 0, 1) == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(se.h)


def test_terms_are_the_start_scale():
    eng, starts = _handle()
    v = ST.make_case(ST.BY_NAME["tail"])[0].astype(np.float64)
    with eng as e:
        e.hals_stack_set((5, 6))
        terms = e.hals_stack_terms()
    for p, (w, h) in enumerate(starts):
        wh = w @ h
        assert abs(terms[p, 0] - np.vdot(v, wh)) <= 1e-6 * np.vdot(v, wh) and abs(terms[p, 1] - np.vdot(wh, wh)) <= 1e-9 * np.vdot(wh, wh), p


# ---- factorize_grid -----------------------------------------------------------------------------------------------------------
def test_grid_equals_the_stacks_of_one_in_the_legacy_order():
    from nmf_amd.engine import Engine
    from nmf_amd.grid import factorize_grid
    from nmf_amd.hals import hals_stack
    v = ST.make_v(M, N)[0]
    kw = dict(max_iter=6, nndsvd_init=(False, "zero"))
    np.random.seed(9)
    runs = factorize_grid(v, "hals", features=(3, 5), lambda_h=(0, 0.1), **kw)
    after = np.random.rand(3)
    assert [p for p, _ in runs] == [dict(features=k, lambda_w=0.0, lambda_h=lh) for k in (3, 5) for lh in (0, 0.1)]
    np.random.seed(9)
    with Engine(M, N, 128) as eng:
        eng.upload_v(v)
        for params, res in runs:
            one, = hals_stack(v, [dict(k=params["features"], lambda_w=params["lambda_w"], lambda_h=params["lambda_h"])], engine=eng, **kw)
            assert np.array_equal(res.w, one.w) and np.array_equal(res.h, one.h), params
            assert np.array_equal(res.obj_history, one.obj_history) and res.i == one.i == 5 and res.experiment == one.experiment, params
    assert np.array_equal(after, np.random.rand(3))
