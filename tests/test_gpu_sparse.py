"""MUR on scipy.sparse input (kernels_sparse.hip) against the reference's goldens and the oracle on x.toarray().
Runs only on a real MI355X (`-m gpu`)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from gpu_common import WH_TOL, run_fixture, wh_error
from oracle import nmf_ref as R

pytestmark = pytest.mark.gpu

OBJ_RTOL = {"eu": 4e-5, "kl": 2e-6}      # the bars of tests/test_gpu_mur.py


def mur_csr(v, k, **kw):
    from nmf_amd.mur import mur
    return mur(sp.csr_matrix(v), k, **kw)


@pytest.mark.parametrize("name", ["mur_eu_cfg1_random", "mur_eu_cfg1_nndsvdz", "mur_eu_lambda", "mur_eu_f32v", "mur_eu_ragged",
                                  "mur_eu_converge", "mur_kl", "mur_kl_lambda", "mur_kl_sparse"])
def test_goldens_as_csr(name):
    z, meta, v, res = run_fixture(name, mur_csr)
    loss = "kl" if name.startswith("mur_kl") else "eu"
    assert res.w.dtype == np.float64 and res.h.dtype == np.float64
    assert res.i == int(z["i"]) and len(res.obj_history) == res.i + 2
    assert wh_error(res.w, res.h, z["w"], z["h"], v) < WH_TOL
    np.testing.assert_allclose(res.obj_history, z["obj_history"], rtol=OBJ_RTOL[loss])
    assert (res.w >= 0).all() and (res.h >= 0).all()


def test_signed_golden_as_csr_raises():
    with pytest.raises(ValueError, match="toarray"):
        run_fixture("mur_eu_signed", mur_csr)


def sparse_case(m, n, density, seed, dense_row=None, dense_col=None, empty_rows=(), empty_cols=()):
    rng = np.random.RandomState(seed)
    x = sp.random(m, n, density=density, format="lil", random_state=rng, data_rvs=lambda s: rng.uniform(0.1, 1.0, s))
    if dense_row is not None:
        x[dense_row, :] = rng.uniform(0.1, 1.0, (1, n))
    if dense_col is not None:
        x[:, dense_col] = rng.uniform(0.1, 1.0, (m, 1))
    for r in empty_rows:
        x[r, :] = 0
    for c in empty_cols:
        x[:, c] = 0
    return x.tocsr()


# (k, density, loss, lambda_w, lambda_h): every k of the issue, each density with both losses, lambda > 0 on one side
CASES = [(1, 0.02, "eu", 0.0, 0.0), (5, 0.005, "kl", 0.0, 0.0), (16, 0.10, "eu", 0.0, 0.1), (33, 0.02, "kl", 0.1, 0.0),
         (64, 0.005, "eu", 0.0, 0.0), (100, 0.10, "kl", 0.0, 0.0), (128, 0.02, "eu", 0.1, 0.0), (256, 0.10, "kl", 0.0, 0.1),
         (8, 0.005, "eu", 0.0, 0.0), (64, 0.10, "eu", 0.0, 0.0), (32, 0.02, "kl", 0.0, 0.0)]


@pytest.mark.parametrize("k,density,loss,lw,lh", CASES)
def test_random_sparse_against_oracle(k, density, loss, lw, lh):
    from nmf_amd.mur import mur
    # 700 x 600: the dense row (600 non-zeros) and the dense column (700) are longer than a unit (256): the split path runs
    x = sparse_case(700, 600, density, seed=k, dense_row=3, dense_col=11, empty_rows=(0, 350), empty_cols=(1, 599))
    x_before = x.copy()
    kw = dict(distance_type=loss, min_iter=30, max_iter=30, lambda_w=lw, lambda_h=lh)
    np.random.seed(5)
    got = mur(x, k, **kw)
    np.random.seed(5)
    want = R.mur(x.toarray(), k, **kw)
    assert (x != x_before).nnz == 0                       # the caller's matrix is untouched
    assert got.i == want.i == 29 and len(got.obj_history) == 31
    assert wh_error(got.w, got.h, want.w, want.h, x.toarray()) < WH_TOL
    np.testing.assert_allclose(got.obj_history, want.obj_history, rtol=OBJ_RTOL[loss])
    assert (got.w >= 0).all() and (got.h >= 0).all()


@pytest.mark.parametrize("loss", ["eu", "kl"])
def test_two_runs_bit_identical(loss):
    from nmf_amd.mur import mur
    x = sparse_case(900, 500, 0.03, seed=9, dense_row=7, dense_col=2)
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(mur(x, 24, distance_type=loss, min_iter=20, max_iter=20))
    assert np.array_equal(out[0].w, out[1].w) and np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))


@pytest.mark.parametrize("loss,rtol", [("eu", 1e-9), ("kl", 1e-6)])
def test_recorded_objective_is_f64_grade(loss, rtol):
    from nmf_amd.mur import mur
    x = sparse_case(800, 700, 0.02, seed=4, dense_row=5)
    np.random.seed(2)
    res = mur(x, 20, distance_type=loss, min_iter=15, max_iter=15)
    xd = x.astype(np.float32).toarray().astype(np.float64)          # the values the device holds
    host = R.objective(xd, res.w @ res.h, loss)
    assert abs(res.obj_history[-1] - host) <= rtol * abs(host), (res.obj_history[-1], host)


def test_capability_shape_dense_would_need_512_gib():
    """1,048,576 x 131,072 at density 1e-4: 1.4e7 non-zeros (dense f32 V: 512 GiB)."""
    from nmf_amd import sparse
    from nmf_amd.mur import mur
    m, n, nnz = 1 << 20, 1 << 17, 14_000_000
    rng = np.random.default_rng(0)
    x = sp.csr_matrix((rng.uniform(0.1, 1.0, nnz).astype(np.float32), (rng.integers(0, m, nnz), rng.integers(0, n, nnz))),
                      shape=(m, n))
    np.random.seed(0)
    res = mur(x, 32, distance_type="eu", min_iter=10, max_iter=5)
    obj = np.asarray(res.obj_history)
    assert len(obj) == 6 and np.all(np.diff(obj) < 0), obj
    assert np.isfinite(res.w).all() and np.isfinite(res.h).all() and (res.w >= 0).all() and (res.h >= 0).all()
    assert abs(obj[-1] - direct_residual(x, res.w, res.h)) <= 1e-9 * obj[-1]
    host = sparse.objective(sparse.normalise(x, 32), res.w, res.h, "eu")
    assert abs(obj[-1] - host) <= 1e-9 * host, (obj[-1], host)


def direct_residual(x, w, h, rows=4096):
    """1/2 sum (x - w h)^2 over all m n entries, in float64, row block by row block on the GPU (torch): the residual
    itself, not the decomposition the engine records."""
    import torch
    dev = torch.device("cuda")
    c = sp.csr_matrix(x, dtype=np.float32)
    c.sum_duplicates()
    hd = torch.from_numpy(h).to(dev)
    total = 0.0
    for a in range(0, c.shape[0], rows):
        b = min(c.shape[0], a + rows)
        blk = c[a:b].tocoo()
        d = torch.from_numpy(w[a:b]).to(dev) @ hd                                   # (b - a) x n of w h
        r = torch.from_numpy(blk.row.astype(np.int64)).to(dev)
        q = torch.from_numpy(blk.col.astype(np.int64)).to(dev)
        d.index_put_((r, q), d[r, q] - torch.from_numpy(blk.data.astype(np.float64)).to(dev))   # w h - x
        total += float(torch.sum(d * d))
    return 0.5 * total


@pytest.mark.parametrize("loss", ["eu", "kl"])
def test_set_factors_resets_a_stopped_handle(loss):
    """nmfx_set_factors on a sparse handle resets the iteration state (stop flag, stop index, objective count, stop guard) as on
    a dense one: a run after it equals the same run on a fresh handle, bit for bit."""
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    dist = L.EU if loss == "eu" else L.KL
    x = sparse.normalise(sparse_case(300, 200, 0.05, seed=3, dense_row=1), 12)
    rs = np.random.RandomState(0)
    w0, h0 = np.abs(rs.randn(300, 12)), np.abs(rs.randn(12, 200))
    w1, h1 = np.abs(rs.randn(300, 12)), np.abs(rs.randn(12, 200))

    def second_run(eng):
        eng.set_factors(w1, h1)
        eng.mur_run(dist, 0.0, 0.0, 10 ** 9, 0.0, 0.0, 0, 9)
        eng.mur_finish(dist, 10 ** 9, 0.0, 0.0, 9)
        rule, stop_i, n_obj = eng.state()
        w, h = eng.get_factors()
        return rule, stop_i, eng.objectives(0, n_obj), w, h

    with Engine.for_sparse(x, 12) as eng:
        eng.set_factors(w0, h0)
        eng.set_stop_guard(1e30)
        eng.mur_run(dist, 0.0, 0.0, 2, 0.0, 0.0, 0, 13)        # the stop rule fires at loop index 3; 9 launches behind it do nothing
        if loss == "eu":                                        # the f64 objective is that of the pair at the stop (before any get_state)
            f64 = eng.objective_f64()
            assert f64 == pytest.approx(eng.objectives(4, 1)[0], rel=1e-12), (f64, eng.objectives(0, 5))
        assert eng.state()[:2] == (2, 3)
        again = second_run(eng)
    with Engine.for_sparse(x, 12) as eng:
        fresh = second_run(eng)
    assert again[0] == fresh[0] == 0 and again[1] == fresh[1] == -1
    assert len(again[2]) == 10
    for a, b in zip(again[2:], fresh[2:]):
        assert np.array_equal(a, b)


def test_sparse_handle_rejects_dense_only_entry_points():
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    x = sparse.normalise(sparse_case(64, 48, 0.1, seed=1), 4)
    with Engine.for_sparse(x, 4) as eng:
        lib = eng.lib
        rc = lib.nmfx_aoadmm_run(eng.h, L.EU, 0, 0.0, 0, 0.0, 10, 10, 1e-3, 1e-3, 0, 1)
        assert rc == L.NMFX_E_ARG and b"sparse handle" in lib.nmfx_last_error(eng.h)
        u = np.empty((64, 4)); s = np.empty(4); vt = np.empty((4, 48))
        sweeps, resid = C.c_int(), C.c_double()
        rc = lib.nmfx_topk_svd(eng.h, 4, 0, 0.0, 0, 0, u.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p),
                               vt.ctypes.data_as(C.c_void_p), C.byref(sweeps), C.byref(resid))
        assert rc == L.NMFX_E_ARG and b"nmfx_topk_svd" in lib.nmfx_last_error(eng.h)
        v = np.zeros((64, 48), dtype=np.float32)
        assert lib.nmfx_upload_v(eng.h, v.ctypes.data_as(C.c_void_p), L.F32, 48, 0, 64) == L.NMFX_E_ARG


def test_upload_csr_checks_row_ptr_before_reading_the_entries():
    """A row_ptr that runs past nnz in one row and comes back in the next is refused before any entry is read."""
    from nmf_amd import _lib as L
    lib = L.require_gpu()
    h = C.c_void_p()
    L.check(lib.nmfx_create_csr(C.byref(h), 0, 2, 4, 2, 5))
    try:
        row_ptr = np.array([0, 100, 5], dtype=np.int64)
        col_idx = np.array([0, 1, 2, 0, 3], dtype=np.int32)
        vals = np.ones(5, dtype=np.float32)
        rc = lib.nmfx_upload_csr(h, row_ptr.ctypes.data_as(C.c_void_p), col_idx.ctypes.data_as(C.c_void_p),
                                 vals.ctypes.data_as(C.c_void_p), L.F32)
        assert rc == L.NMFX_E_ARG and b"row_ptr" in lib.nmfx_last_error(h)
    finally:
        lib.nmfx_destroy(h)
