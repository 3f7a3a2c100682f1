"""nmf_amd.hals.hals_sparse_wide on the device: the public call against the float64 host loop of the same definition, the
monotone objective, the stop rule, the caller's matrix, the input formats, and the refusals and the family rule of the C ABI.
Single half-steps, problem by problem: tests/test_gpu_hals_sparse_wide_step.py."""
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_hals_wide_step as SW
from sparse_hals_step import A

pytestmark = pytest.mark.gpu

NO_NNDSVD = (False, "zero")
CASE = SW.Case("base", 200, "scaled", 1)
ITERS = 5
SEED = 5


def scaled_start(x, k, seed):
    """The draw hals_sparse_wide makes with nndsvd_init=(False, 'zero') after np.random.seed(seed), scaled by the float64 alpha of
    the float32 values the device holds."""
    rng = np.random.RandomState(seed)
    w0, h0 = rng.rand(x.shape[0], k), rng.rand(k, x.shape[1])
    w, h = A.f32(w0), A.f32(h0)
    a = float(np.sum(sp.csr_matrix(x, dtype=np.float64).multiply(w @ h))) / float(np.sum((w.T @ w) * (h @ h.T)))
    return A.f32(w0 * math.sqrt(a)), A.f32(h0 * math.sqrt(a))


@functools.lru_cache(maxsize=None)
def reference():
    x = SW.matrix(CASE.matrix)
    return SW.host_hals(x, *scaled_start(x, CASE.k, SEED), *SW.lam_of(CASE), CASE.sweeps, ITERS)


@functools.lru_cache(maxsize=None)
def device():
    from nmf_amd.hals import hals_sparse_wide
    x = SW.matrix(CASE.matrix)
    lw, lh = SW.lam_of(CASE)
    np.random.seed(SEED)
    return hals_sparse_wide(x.copy(), CASE.k, lambda_w=lw, lambda_h=lh, max_iter=ITERS, min_iter=ITERS, nndsvd_init=NO_NNDSVD)


def test_public_call_matches_the_float64_loop():
    """Five iterations from the same start.  The rule: a half-step of this case from the same iterate is within the step bar of
    the case, relative to the largest entry of a problem's solution (tests/sparse_hals_wide_step.py), and the run is ten
    half-steps, each starting from the one before: W H, relative to its largest entry, and the history, relative to its
    entries, are held to ten step bars.  W H is compared on every non-zero and on a seeded dense sample of 20000 entries."""
    x = SW.matrix(CASE.matrix)
    wr, hr, hist = reference()
    res = device()
    bar = 2 * ITERS * SW.bar_of(CASE)
    assert res.i == ITERS - 1 and len(res.obj_history) == ITERS + 1
    assert res.w.shape == (700, CASE.k) and res.h.shape == (CASE.k, 600) and (res.w >= 0).all() and (res.h >= 0).all()
    rows = np.repeat(np.arange(x.shape[0]), np.diff(x.indptr))
    rng = np.random.RandomState(1)
    rows = np.concatenate([rows, rng.randint(0, x.shape[0], 20000)])
    cols = np.concatenate([x.indices, rng.randint(0, x.shape[1], 20000)])
    got = np.einsum("ij,ji->i", res.w[rows], res.h[:, cols])
    want = np.einsum("ij,ji->i", wr[rows], hr[:, cols])
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    rel = float(np.max(np.abs(np.asarray(res.obj_history) / hist - 1)))
    print(f"k = {CASE.k}: WH error {err:.3e}, history rel {rel:.3e}, bar {bar:.1e}")
    assert err <= bar, err
    assert rel <= bar, rel
    exp = res.experiment
    lw, lh = SW.lam_of(CASE)
    assert (exp.method, exp.components, exp.sweeps, exp.distance_type, exp.lambda_w, exp.lambda_h) == ("hals", CASE.k, 1, "eu", lw, lh)


def test_objective_does_not_increase():
    obj = np.asarray(device().obj_history)
    assert (obj[1:] <= obj[:-1] * (1 + 1e-6)).all(), obj


def test_recorded_objective_is_the_float64_objective_of_the_result():
    res = device()
    want = SW.objective(SW.matrix(CASE.matrix), res.w, res.h)
    assert abs(res.obj_history[-1] - want) <= SW.OBJ_RTOL * abs(want)


def test_x_is_unmodified():
    from nmf_amd.hals import hals_sparse_wide
    x = sp.csr_matrix(SW.matrix(CASE.matrix), copy=True)
    keep = x.copy()
    np.random.seed(SEED)
    hals_sparse_wide(x, 129, max_iter=2, nndsvd_init=NO_NNDSVD)
    assert (x != keep).nnz == 0 and np.array_equal(x.data, keep.data) and np.array_equal(x.indices, keep.indices)
    assert np.array_equal(x.indptr, keep.indptr)


@pytest.mark.parametrize("fmt", ["csc_matrix", "coo_matrix"])
def test_any_sparse_format_gives_the_bits_of_csr(fmt):
    from nmf_amd.hals import hals_sparse_wide
    x = SW.matrix(CASE.matrix)
    out = []
    for xx in (x, getattr(sp, fmt)(x)):
        np.random.seed(SEED)
        out.append(hals_sparse_wide(xx, 129, max_iter=2, nndsvd_init=NO_NNDSVD))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))


def test_stop_rule_stops_where_the_float64_loop_stops():
    """tol2 is the geometric mean of the float64 loop's decreases at two consecutive indices (131.9 and 74.5).  Under the history
    bar of test_public_call_matches_the_float64_loop an entry of the device's history is within bar x obj[0] of the float64
    one, a decrease within twice that; tol2 is further than that from every decrease the rule is tested on (asserted), so
    float32 iterates cannot move the stop: the device stops at the same i, the history has i + 2 entries and the returned pair
    is the one its last entry belongs to."""
    from nmf_amd.hals import hals_sparse_wide
    x = SW.matrix(CASE.matrix)
    lw, lh = SW.lam_of(CASE)
    _, _, hist = reference()
    bar = 2 * ITERS * SW.bar_of(CASE)
    dec = hist[:-1] - hist[1:]                          # dec[i]: the decrease iteration i brings
    stop = 3
    tol2 = math.sqrt(dec[stop - 1] * dec[stop])         # the rule is tested at i = 1, 2, ...: it must hold at 3 and not before
    margin = 2 * bar * hist[0]
    assert dec[stop] + margin <= tol2 and (dec[1:stop] >= tol2 + margin).all(), (dec, tol2, margin)      # the precondition
    np.random.seed(SEED)
    res = hals_sparse_wide(x, CASE.k, lambda_w=lw, lambda_h=lh, min_iter=0, max_iter=ITERS, tol1=1e-3, tol2=float(tol2),
                           nndsvd_init=NO_NNDSVD)
    assert res.i == stop and len(res.obj_history) == res.i + 2, (res.i, stop, len(res.obj_history))
    want = SW.objective(x, res.w, res.h)
    assert abs(res.obj_history[-1] - want) <= SW.OBJ_RTOL * abs(want), (res.obj_history[-1], want)
    np.testing.assert_allclose(res.obj_history, hist[:stop + 2], rtol=bar)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_and_the_family_rule():
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    lib = L.load()
    assert lib.nmfx_version() >= 397
    x = SW.matrix(CASE.matrix)
    T = (10, 1e-3, 1e-3)
    rs = np.random.RandomState(1)

    def refused(eng, word, *args):
        before = eng.state()
        assert lib.nmfx_hals_sparse_wide_run(eng.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h), lib.nmfx_last_error(eng.h)
        assert b"nmfx_hals_sparse_wide_run" in lib.nmfx_last_error(eng.h)
        assert lib.nmfx_hals_sparse_wide_finish(eng.h, *T, 0) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h)
        assert b"nmfx_hals_sparse_wide_finish" in lib.nmfx_last_error(eng.h)
        assert eng.state() == before                    # nothing recorded

    with Engine(64, 48, 200) as eng:
        eng.upload_v(rs.rand(64, 48))
        eng.set_factors(rs.rand(64, 200), rs.rand(200, 48))
        refused(eng, b"sparse handle", 0.0, 0.0, 1, *T, 0, 1)
    with Engine.for_sparse(x, 200, masked=True) as eng:
        eng.set_factors(rs.rand(700, 200), rs.rand(200, 600))
        refused(eng, b"masked", 0.0, 0.0, 1, *T, 0, 1)
    with Engine.for_sparse(x, 64) as eng:
        eng.set_factors(rs.rand(700, 64), rs.rand(64, 600))
        refused(eng, b"nmfx_hals_sparse_run", 0.0, 0.0, 1, *T, 0, 1)
    with Engine.for_sparse(x, 200) as eng:
        w0, h0 = SW.start(CASE)
        eng.set_factors(w0, h0)
        for args, word in (((0.0, 0.0, 0, *T, 0, 1), b"sweeps"), ((0.0, 0.0, 17, *T, 0, 1), b"sweeps"), ((0.0, 0.0, 1, *T, -1, 1), b"range"),
                           ((-1.0, 0.0, 1, *T, 0, 1), b"lambda"), ((0.0, float("nan"), 1, *T, 0, 1), b"lambda")):
            assert lib.nmfx_hals_sparse_wide_run(eng.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h), (args, lib.nmfx_last_error(eng.h))
        # nmfx_hals_sparse_run goes on refusing kp = 256
        before = eng.state()
        assert lib.nmfx_hals_sparse_run(eng.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"128" in lib.nmfx_last_error(eng.h)
        assert eng.state() == before
        # HALS family: nmfx_mur_run does not continue a wide HALS run without nmfx_set_factors
        eng.hals_sparse_wide_run(0, 0, 1, *T, 0, 1)
        assert lib.nmfx_mur_run(eng.h, L.EU, 0.0, 0.0, *T, 1, 1) == L.NMFX_E_STATE and b"another solver" in lib.nmfx_last_error(eng.h)
        eng.set_factors(w0, h0)
        eng.mur_run(L.EU, 0.0, 0.0, *T, 0, 1)
        assert lib.nmfx_hals_sparse_wide_run(eng.h, 0.0, 0.0, 1, *T, 1, 1) == L.NMFX_E_STATE
