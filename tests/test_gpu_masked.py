"""Masked MUR (mur(x, k, mask=...), kernels_sparse.hip on a masked handle) against the reference's goldens with an all-ones
mask and against the float64 restatement of tests/masked_ref.py.  Runs only on a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from gpu_common import WH_TOL, run_fixture, wh_error
from masked_ref import masked_h_step, masked_mur, masked_w_step
from mur_step import BARS, NEVER, compare
from oracle import nmf_ref as R

pytestmark = pytest.mark.gpu

OBJ_RTOL = {"eu": 4e-5, "kl": 2e-6}      # the bars of tests/test_gpu_sparse.py
STEP_BAR = BARS[("f32", "eu")]           # 2e-5: the exact-f32 bar of tests/mur_step.py (eu and kl alike)


def mur_masked(x, k, mask, **kw):
    from nmf_amd.mur import mur
    return mur(x, k, mask=mask, **kw)


def observed_error(w, h, w_ref, h_ref, x, m):
    """||M.(W H - W_ref H_ref)|| / ||M.X||"""
    d = np.where(m, w @ h - w_ref @ h_ref, 0.0)
    return np.linalg.norm(d) / np.linalg.norm(np.where(m, x, 0.0))


def planted(m, n, k, seed):
    return R.planted_matrix(m, n, k, seed=seed, dtype=np.float64)


# ---- 1. an all-ones mask is the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mur_eu_lambda", "mur_eu_ragged", "mur_kl", "mur_kl_lambda"])
def test_goldens_with_all_ones_mask(name):
    z, meta, v, res = run_fixture(name, lambda v, k, **kw: mur_masked(v, k, np.ones(v.shape, dtype=bool), **kw))
    loss = "kl" if name.startswith("mur_kl") else "eu"
    assert res.i == int(z["i"]) and len(res.obj_history) == res.i + 2
    assert wh_error(res.w, res.h, z["w"], z["h"], v) < WH_TOL
    np.testing.assert_allclose(res.obj_history, z["obj_history"], rtol=OBJ_RTOL[loss])


@pytest.mark.parametrize("loss,lw,lh", [("eu", 0.0, 0.0), ("eu", 0.1, 0.05), ("kl", 0.0, 0.0), ("kl", 0.05, 0.1)])
def test_planted_with_all_ones_mask(loss, lw, lh):
    v = planted(300, 220, 7, seed=11)
    kw = dict(distance_type=loss, min_iter=3, max_iter=60, tol1=1e-5, tol2=1e-5, lambda_w=lw, lambda_h=lh)
    np.random.seed(4)
    got = mur_masked(v, 7, np.ones(v.shape, dtype=bool), **kw)
    np.random.seed(4)
    want = R.mur(v.copy(), 7, **kw)
    assert got.i == want.i and len(got.obj_history) == len(want.obj_history)
    assert wh_error(got.w, got.h, want.w, want.h, v) < WH_TOL
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])


# ---- 2. random masks against the float64 restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.05, 0.30, 0.90])
@pytest.mark.parametrize("loss", ["eu", "kl"])
def test_random_masks_against_masked_reference(frac, loss):
    rng = np.random.RandomState(int(frac * 100) + (loss == "kl"))
    x = planted(400, 300, 6, seed=2)
    m = rng.rand(*x.shape) < frac
    xn = np.where(m, x, np.nan)                      # unobserved cells are never read
    xn[~m & (rng.rand(*x.shape) < 0.5)] = -3.0
    kw = dict(distance_type=loss, min_iter=30, max_iter=30, lambda_w=0.02, lambda_h=0.0)
    np.random.seed(9)
    got = mur_masked(xn, 6, m, **kw)
    np.random.seed(9)
    want = masked_mur(x, m, 6, **kw)
    assert got.i == want.i == 29 and len(got.obj_history) == 31
    assert observed_error(got.w, got.h, want.w, want.h, x, m) < WH_TOL
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])
    assert np.isfinite(got.w).all() and np.isfinite(got.h).all() and (got.w >= 0).all() and (got.h >= 0).all()


@pytest.mark.parametrize("loss,tol2", [("eu", 3e-3), ("kl", 5e-3)])
def test_stop_rule_fires_where_the_reference_stops(loss, tol2):
    # (the reference stops at i = 204 / 217, with the decreases around the stop about 1 % away from tol2)
    x = planted(250, 200, 5, seed=3)
    m = np.random.RandomState(1).rand(*x.shape) < 0.5
    kw = dict(distance_type=loss, min_iter=5, max_iter=400, tol1=1e-5, tol2=tol2)
    np.random.seed(2)
    got = mur_masked(x, 5, m, **kw)
    np.random.seed(2)
    want = masked_mur(x, m, 5, **kw)
    assert want.trace["stop_rule"] and got.i == want.i and len(got.obj_history) == len(want.obj_history)
    assert observed_error(got.w, got.h, want.w, want.h, x, m) < WH_TOL
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])


@pytest.mark.parametrize("loss", ["eu", "kl"])
def test_nndsvd_start_of_the_observed_matrix(loss):
    x = planted(300, 200, 5, seed=13)
    m = np.random.RandomState(13).rand(*x.shape) < 0.4
    kw = dict(distance_type=loss, min_iter=20, max_iter=20, nndsvd_init=(True, "mean"))
    got = mur_masked(np.where(m, x, np.nan), 5, m, **kw)
    want = masked_mur(x, m, 5, **kw)
    assert observed_error(got.w, got.h, want.w, want.h, x, m) < WH_TOL
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])


# ---- 3. element-wise half-steps -------------------------------------------------------------------------------------------
def step_case(seed):
    """400 x 600: rows 1 and 2 / column 3 unobserved, row 0 and column 0 fully observed (600 and 400 > 256: pieces and fixup),
    observed zeros scattered; W0, H0 hold f32 values."""
    rng = np.random.default_rng(seed)
    m_, n_ = 400, 600
    x = rng.uniform(0.05, 1.0, (m_, n_)).astype(np.float32).astype(np.float64)
    mask = rng.random((m_, n_)) < 0.3
    mask[0, :] = True
    mask[:, 0] = True
    mask[1:3, :] = False
    mask[:, 3] = False
    x[(rng.random((m_, n_)) < 0.05) & mask] = 0.0
    return x, mask


def run_steps(x, mask, k, kind, w0, h0, lw, lh, steps=(1, 2)):
    from nmf_amd import _lib as L
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    dist = L.EU if kind == "eu" else L.KL
    out = {}
    with Engine.for_sparse(masked.observed(x, mask, k), k, masked=True) as eng:
        for s in steps:
            eng.set_factors(w0, h0)
            eng.mur_run(dist, lw, lh, NEVER, 0, 0, 0, s)
            eng.mur_finish(dist, NEVER, 0, 0, s)
            w, h = eng.get_factors()
            out[s] = (w, h, eng.objectives(0, s + 1))
    return out


@pytest.mark.parametrize("kind,k,lw,lh", [("eu", 12, 0.0, 0.0), ("eu", 64, 0.1, 0.05), ("kl", 12, 0.0, 0.0), ("kl", 40, 0.05, 0.1)])
def test_half_steps_element_by_element(kind, k, lw, lh):
    from nmf_amd import masked
    x, mask = step_case(k)
    rng = np.random.default_rng(100 + k)
    w0 = rng.uniform(0.1, 1.0, (x.shape[0], k)).astype(np.float32).astype(np.float64)
    h0 = rng.uniform(0.1, 1.0, (k, x.shape[1])).astype(np.float32).astype(np.float64)
    runs = run_steps(x, mask, k, kind, w0, h0, lw, lh)
    fails, worst, iterate = [], {}, {0: (w0, h0)}
    for s in (1, 2):
        ws, hs, _ = runs[s]
        wp, hp = iterate[s - 1]
        for label, dev, ref in ((f"W{s}", ws, masked_w_step(kind, x, mask, wp, hp, lw)),
                                (f"H{s}", hs, masked_h_step(kind, x, mask, ws, hp, lh))):
            err, msg = compare(label, dev, ref, STEP_BAR)
            worst[label] = err
            if msg:
                fails.append(msg)
        iterate[s] = (ws, hs)
    for s, (_, _, hist) in runs.items():
        for i in range(s + 1):
            want = masked.objective(x, *iterate[i], mask, kind)
            if abs(hist[i] - want) > (1e-9 if kind == "eu" else 1e-6) * abs(want):
                fails.append(f"obj[{i}] of the {s}-step run: {hist[i]!r} vs {want!r}")
    assert not fails, "\n".join(fails)
    ws, hs, _ = runs[2]
    assert (ws[1:3] == 0).all() and (hs[:, 3] == 0).all()           # no observed entry: exactly 0, no NaN
    print(f"worst relative error per half-step ({kind}, k = {k}):", {key: f"{val:.2e}" for key, val in worst.items()})


# ---- 4. edge cases --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["eu", "kl"])
def test_empty_rows_and_columns_and_long_rows(loss):
    x, mask = step_case(7)
    np.random.seed(3)
    got = mur_masked(x, 9, mask, distance_type=loss, min_iter=20, max_iter=20)
    np.random.seed(3)
    want = masked_mur(x, mask, 9, distance_type=loss, min_iter=20, max_iter=20)
    assert np.isfinite(got.w).all() and np.isfinite(got.h).all()
    assert (got.w[1:3] == 0).all() and (got.h[:, 3] == 0).all()
    assert observed_error(got.w, got.h, want.w, want.h, x, mask) < WH_TOL
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])


def test_power_law_pattern():
    rng = np.random.default_rng(4)
    m_, n_, nnz = 2000, 900, 60000
    p = np.arange(1, m_ + 1, dtype=np.float64) ** -1.0
    rows = rng.choice(m_, size=nnz, p=rng.permutation(p / p.sum()))
    cols = rng.integers(0, n_, nnz)
    mask = np.zeros((m_, n_), dtype=bool)
    mask[rows, cols] = True
    assert mask.sum(axis=1).max() > 256
    x = planted(m_, n_, 6, seed=5)
    for loss in ("eu", "kl"):
        np.random.seed(6)
        got = mur_masked(x, 16, sp.csr_matrix(mask), distance_type=loss, min_iter=15, max_iter=15)
        np.random.seed(6)
        want = masked_mur(x, mask, 16, distance_type=loss, min_iter=15, max_iter=15)
        assert observed_error(got.w, got.h, want.w, want.h, x, mask) < WH_TOL, loss
        np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])


@pytest.mark.parametrize("loss", ["eu", "kl"])
def test_observed_zeros_change_the_answer(loss):
    """The same sparse x: unmasked, its unstored cells are observed zeros; masked with its stored pattern, they are unknown."""
    from nmf_amd.mur import mur
    rng = np.random.RandomState(8)
    x = sp.random(300, 250, density=0.1, format="csr", random_state=rng, data_rvs=lambda s: rng.uniform(0.1, 1.0, s))
    pattern = x.copy()
    pattern.data[:] = 1
    kw = dict(distance_type=loss, min_iter=20, max_iter=20)
    np.random.seed(1)
    plain = mur(x, 5, **kw)
    np.random.seed(1)
    got = mur(x, 5, mask=pattern, **kw)
    m = pattern.toarray() != 0
    np.random.seed(1)
    want = masked_mur(x.toarray(), m, 5, **kw)
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])
    assert observed_error(got.w, got.h, want.w, want.h, x.toarray(), m) < WH_TOL
    assert observed_error(plain.w, plain.h, want.w, want.h, x.toarray(), m) > 100 * WH_TOL
    assert abs(plain.obj_history[-1] - got.obj_history[-1]) > 1e-3 * got.obj_history[-1]


# ---- 5. every padding boundary of kp --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256])
def test_k_at_padding_boundaries(k):
    loss = "eu" if k % 2 else "kl"
    rng = np.random.RandomState(k)
    x = planted(300, 280, 8, seed=k)
    m = rng.rand(*x.shape) < 0.3
    m[5, :] = True                                              # a row longer than 256 observed entries
    np.random.seed(k)
    got = mur_masked(x, k, m, distance_type=loss, min_iter=6, max_iter=6, lambda_h=0.01)
    np.random.seed(k)
    want = masked_mur(x, m, k, distance_type=loss, min_iter=6, max_iter=6, lambda_h=0.01)
    assert got.w.shape == (300, k) and got.h.shape == (k, 280)
    assert observed_error(got.w, got.h, want.w, want.h, x, m) < WH_TOL
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])


# ---- 6. the recorded objective is float64-grade ---------------------------------------------------------------------------
@pytest.mark.parametrize("loss,rtol", [("eu", 1e-9), ("kl", 1e-6)])
def test_recorded_objective_is_f64_grade(loss, rtol):
    from nmf_amd import masked
    x = planted(500, 400, 6, seed=12)
    m = np.random.RandomState(12).rand(*x.shape) < 0.2
    np.random.seed(2)
    res = mur_masked(x, 20, m, distance_type=loss, min_iter=15, max_iter=15)
    xd = x.astype(np.float32).astype(np.float64)                  # the values the device holds
    host = masked.objective(xd, res.w, res.h, m, loss)
    assert abs(res.obj_history[-1] - host) <= rtol * abs(host), (res.obj_history[-1], host)


# ---- 7. determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["eu", "kl"])
def test_two_runs_bit_identical(loss):
    x, mask = step_case(21)
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(mur_masked(x, 24, mask, distance_type=loss, min_iter=15, max_iter=15))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))


# ---- 8. ABI ---------------------------------------------------------------------------------------------------------------
def test_set_masked_only_between_create_and_upload():
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    lib = L.require_gpu()
    with Engine(64, 48, 4) as eng:                                # a dense handle
        assert lib.nmfx_set_masked(eng.h, 1) == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(eng.h)
    x = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 4)
    rs = np.random.RandomState(0)
    w0, h0 = np.abs(rs.randn(64, 4)), np.abs(rs.randn(4, 48))

    def run(eng):
        eng.set_factors(w0, h0)
        eng.mur_run(L.EU, 0.0, 0.0, NEVER, 0.0, 0.0, 0, 5)
        eng.mur_finish(L.EU, NEVER, 0.0, 0.0, 5)
        return eng.get_factors(), eng.objectives(0, 6)

    with Engine.for_sparse(x, 4) as eng:                          # after the upload: refused, the handle stays unmasked
        assert lib.nmfx_set_masked(eng.h, 1) == L.NMFX_E_STATE and b"upload" in lib.nmfx_last_error(eng.h)
        after = run(eng)
    with Engine.for_sparse(x, 4) as eng:
        fresh = run(eng)
    assert np.array_equal(after[0][0], fresh[0][0]) and np.array_equal(after[0][1], fresh[0][1])
    assert np.array_equal(after[1], fresh[1])
    with Engine.for_sparse(x, 4, masked=True) as eng:            # ... while a masked handle on the same entries differs
        masked_run = run(eng)
    assert not np.array_equal(masked_run[1], fresh[1])


# ---- 9. capability --------------------------------------------------------------------------------------------------------
def test_capability_shape():
    """1,048,576 x 131,072 with 1.4e7 observed entries (dense f32 V: 512 GiB)."""
    from nmf_amd import masked
    m_, n_, nnz = 1 << 20, 1 << 17, 14_000_000
    rng = np.random.default_rng(0)
    r, c = rng.integers(0, m_, nnz), rng.integers(0, n_, nnz)
    x = sp.csr_matrix((rng.uniform(0.1, 1.0, nnz).astype(np.float32), (r, c)), shape=(m_, n_))
    mask = sp.csr_matrix((np.ones(nnz, dtype=np.int8), (r, c)), shape=(m_, n_))
    np.random.seed(0)
    res = mur_masked(x, 32, mask, distance_type="eu", min_iter=10, max_iter=4)
    obj = np.asarray(res.obj_history)
    assert len(obj) == 5 and np.all(np.isfinite(obj)) and np.all(np.diff(obj) < 0), obj
    assert np.isfinite(res.w).all() and np.isfinite(res.h).all() and (res.w >= 0).all() and (res.h >= 0).all()
    host = masked.objective(x, res.w, res.h, mask, "eu")
    assert abs(obj[-1] - host) <= 1e-9 * host, (obj[-1], host)
