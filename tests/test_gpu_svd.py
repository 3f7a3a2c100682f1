"""Device top-k SVD (nmfx_topk_svd) and the NNDSVD built on it against numpy's LAPACK SVD
(what nmf/utils.py:50 calls)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
os.environ.setdefault("NMF_AMD_QUIET", "1")


def _align(u, ref):
    """flip the sign of each column of u to match ref"""
    sgn = np.sign(np.sum(u * ref, axis=0))
    sgn[sgn == 0] = 1
    return u * sgn, sgn


CASES = [
    ("planted", 700, 330, 12),       # rank-12 + noise: large gap after the k-th value
    ("uniform", 512, 256, 8),        # np.random.rand: one dominant value, then a gap-less bulk
    ("wide", 200, 900, 5),
    ("f64", 300, 280, 16),
]


@pytest.mark.parametrize("kind,m,n,k", CASES)
def test_topk_svd_matches_lapack(kind, m, n, k):
    from oracle import nmf_ref as R
    from nmf_amd.engine import Engine
    if kind == "planted":
        v = R.planted_matrix(m, n, k, seed=5, dtype=np.float32)
    else:
        v = np.random.RandomState(6).rand(m, n).astype(np.float64 if kind == "f64" else np.float32)
    with Engine(m, n, k) as eng:
        eng.upload_v(v)
        u, s, vt, sweeps, resid = eng.topk_svd(k)
    v32 = v.astype(np.float32).astype(np.float64)          # the engine holds V in f32
    ur, sr, vtr = np.linalg.svd(v32, full_matrices=False)
    assert resid <= 1e-11, (sweeps, resid)
    np.testing.assert_allclose(s, sr[:k], rtol=1e-12)
    ua, sgn = _align(u, ur[:, :k])
    # vector error ~ residual / gap: compare through the subspace-insensitive rank-k reconstruction
    # and, where the spectrum is separated, vector by vector
    rec, rec_ref = (ua * s) @ (vt * sgn[:, None]), (ur[:, :k] * sr[:k]) @ vtr[:k]
    assert np.linalg.norm(rec - rec_ref) / np.linalg.norm(rec_ref) < 1e-9
    gaps = np.minimum(np.abs(np.diff(sr[:k + 1]))[:-1] if k > 1 else np.inf, np.abs(np.diff(sr[:k + 1]))[1:] if k > 1 else np.inf)
    for j in range(k):
        gap = min(abs(sr[j] - sr[j - 1]) if j else np.inf, abs(sr[j] - sr[j + 1]))
        if gap > 1e-3 * sr[0]:
            assert np.max(np.abs(ua[:, j] - ur[:, j])) < 1e-7, j
            assert np.max(np.abs(vt[j] * sgn[j] - vtr[j])) < 1e-7, j
    assert np.max(np.abs(u.T @ u - np.eye(k))) < 1e-10


@pytest.mark.parametrize("variant", ["zero", "mean"])
def test_device_nndsvd_matches_host_nndsvd(variant):
    from oracle import nmf_ref as R
    from nmf_amd import utils
    from nmf_amd.engine import Engine
    m, n, k = 640, 384, 10
    v = R.planted_matrix(m, n, k, seed=9, dtype=np.float32)
    w_ref, h_ref = utils.nndsvd(v.astype(np.float64), k, variant=variant)
    with Engine(m, n, k) as eng:
        eng.upload_v(v)
        w, h = utils.nndsvd_device(eng, v, k, variant=variant)
    np.testing.assert_allclose(w, w_ref, rtol=0, atol=1e-7 * np.max(w_ref))
    np.testing.assert_allclose(h, h_ref, rtol=0, atol=1e-7 * np.max(h_ref))


def test_solver_with_device_nndsvd_matches_oracle(monkeypatch):
    """End to end: ao_admm started from the device NNDSVD equals the oracle started from LAPACK's."""
    from oracle import nmf_ref as R
    from nmf_amd.ao_admm import ao_admm
    monkeypatch.setenv("NMFX_NNDSVD", "device")
    m, n, k = 520, 300, 12
    v = R.planted_matrix(m, n, k, seed=31, dtype=np.float32)
    kw = dict(distance_type="eu", reg_w=(0.1, "l1n"), reg_h=(0.05, "l1n"), min_iter=8, max_iter=8, admm_iter=10,
              nndsvd_init=(True, "zero"))
    ref = R.ao_admm(v.astype(np.float64), k, **kw)
    res = ao_admm(v.copy(), k, **kw)
    err = np.linalg.norm(res.w @ res.h - ref.w @ ref.h) / np.linalg.norm(v.astype(np.float64))
    assert err < 1e-4, err
    assert res.i == ref.i
    np.testing.assert_allclose(res.obj_history, ref.obj_history, rtol=1e-5)      # (measured: 9.8e-7)


# ---- every block width, edge shape and rank (tests/svd_ref.py; CPU side tests/test_svd_bars.py) ------------------------------------
import ctypes as C      # noqa: E402

import svd_ref as S     # noqa: E402


def _run_case(c, **over):
    """(u, s, vt, sweeps, resid) of case c on a fresh handle"""
    from nmf_amd.engine import Engine
    kw = dict(c.kw)
    kw.update(over)
    with Engine(c.m, c.n, c.k) as eng:
        eng.upload_v(S.make_input(c))
        return eng.topk_svd(c.k, **kw)


def _hold(c, out, bars=None, label=None):
    """check_triplets and the sweep cap of case c; records the worst-to-bar ratios"""
    u, s, vt, sweeps, resid = out
    bars = bars or S.bars_of(c)
    fails, dev = S.check_triplets(S.make_input(c), u, s, vt, resid, c.k, bars)
    dev["sweeps"] = sweeps
    print(f"{c.id}: sweeps {sweeps} (cap {bars['sweep_cap']}), resid {resid:.2e}, " + ", ".join(f"{q} {dev[q]:.2e}" for q in ("values", "null", "orth", "vectors", "recon")))
    S.record(label or c.id, dev, bars)
    assert not fails, f"{c.id} ({sweeps} sweeps, resid {resid:.2e}):\n" + "\n".join(fails)
    assert sweeps <= bars["sweep_cap"], (c.id, sweeps, bars["sweep_cap"])
    return dev


@pytest.mark.parametrize("c", S.CASES, ids=[c.id for c in S.CASES])
def test_topk_svd_case(c):
    out = _run_case(c)
    _hold(c, out)
    if c.id == "zero-row-col":
        assert not out[0][3].any() and not out[2][:, 5].any()          # exact zeros


def test_seeds_agree_within_the_bars():
    cases = [S.BY_ID[f"k70-seed{s}"] for s in range(4)]
    outs = [_run_case(c) for c in cases]
    bars = S.bars_of(cases[0])
    rec = [(u * s) @ vt for u, s, vt, _, _ in outs]
    for a in range(1, 4):
        assert np.max(np.abs(outs[a][1] - outs[0][1]) / outs[0][1]) <= 2 * bars["values"], a
        assert np.linalg.norm(rec[a] - rec[0]) / np.linalg.norm(rec[0]) <= 2 * bars["recon"], a
    assert any(not np.array_equal(outs[a][0], outs[0][0]) for a in range(1, 4))     # (the seed does reach the start block)


def test_identical_calls_are_bit_identical():
    c = S.BY_ID["k70-seed0"]
    a, b = _run_case(c), _run_case(c)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and a[4] == b[4]


def test_wide_block_never_reports_convergence_with_a_wrong_answer():
    """block = 192 at k = 40: a block that loses rank under the filter must not end as converged.  Either every check holds or
    the call says resid > tol; the k triplets are orthonormal and the reported residual honest in both cases."""
    c = S.WIDE_BLOCK
    u, s, vt, sweeps, resid = _run_case(c)
    bars = S.bars_of(c)
    fails, dev = S.check_triplets(S.make_input(c), u, s, vt, resid, c.k, dict(bars, resid=None))
    dev["sweeps"] = sweeps
    print(f"{c.id}: sweeps {sweeps}, resid {resid:.2e}, {dev}")
    if resid <= 1e-11:
        S.record(c.id, dev, bars)
        assert not fails, "\n".join(fails)
    else:
        assert sweeps == 250
        assert not [f for f in fails if f.startswith("[orthonormality]") or f.startswith("[residual]")], "\n".join(fails)


def test_max_sweeps_is_kept_and_the_residual_is_honest():
    c = S.TWO_SWEEPS
    u, s, vt, sweeps, resid = _run_case(c)
    host = S.recompute_resid(S.make_input(c), u, s, vt)
    print(f"{c.id}: sweeps {sweeps}, resid {resid:.3e}, recomputed {host:.3e}")
    assert sweeps == 2 and resid > 1e-9
    assert 0.5 <= resid / host <= 2.0, (resid, host)
    assert np.max(np.abs(u.T @ u - np.eye(c.k))) < 1e-10 and np.max(np.abs(vt @ vt.T - np.eye(c.k))) < 1e-10


def test_tol_argument_stops_earlier():
    c = S.BY_ID["L96-k64"]
    loose, tight = _run_case(c, tol=1e-6), _run_case(c)
    assert loose[3] <= tight[3] and tight[4] <= 1e-11 and loose[4] <= 1e-6
    assert 0.5 * S.recompute_resid(S.make_input(c), *loose[:3]) - 1e-13 <= loose[4]


# ---- NNDSVD from the device triplets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["zero", "mean"])
@pytest.mark.parametrize("k", [33, 64, 128])
def test_device_nndsvd_at_wider_blocks(k, variant, monkeypatch):
    from nmf_amd import utils
    from nmf_amd.engine import Engine
    monkeypatch.setenv("NMFX_NNDSVD", "device")             # (no fall-back to the host behind a slow convergence)
    c = S.BY_ID[f"L{S.block_width(k)}-k{k}"]
    v = S.make_input(c)
    w_ref, h_ref = utils.nndsvd(v.astype(np.float64), k, variant=variant)
    with Engine(c.m, c.n, k) as eng:
        eng.upload_v(v)
        w, h = utils.nndsvd_device(eng, v, k, variant=variant)
    np.testing.assert_allclose(w, w_ref, rtol=0, atol=1e-7 * np.max(w_ref))
    np.testing.assert_allclose(h, h_ref, rtol=0, atol=1e-7 * np.max(h_ref))


@pytest.mark.parametrize("variant", ["zero", "mean"])
@pytest.mark.parametrize("cid", ["rank6-k10", "tiled8-k12"])
def test_device_nndsvd_of_a_matrix_of_rank_below_k(cid, variant, monkeypatch):
    """Null triplets give zero columns of W0 and rows of H0 (filled by the mean in that variant), never 0 / 0.  With 'mean' the
    host's own W0 H0 depends on the signs LAPACK happens to give its null vectors (their zero parts are what the mean fills), so
    there the product is compared over the r columns that are defined."""
    from nmf_amd import utils
    from nmf_amd.engine import Engine
    monkeypatch.setenv("NMFX_NNDSVD", "device")
    c = S.BY_ID[cid]
    v = S.make_input(c)
    x = v.astype(np.float64)
    sr = S.lapack(v)[2]
    r = int(np.sum(sr > S.RANK_REL * sr[0]))
    wr, hr = utils.nndsvd(x, c.k, variant=variant)
    with Engine(c.m, c.n, c.k) as eng:
        eng.upload_v(v)
        w, h = utils.nndsvd_device(eng, v, c.k, variant=variant)
    assert np.isfinite(w).all() and np.isfinite(h).all() and w.min() >= 0 and h.min() >= 0
    np.testing.assert_allclose(w[:, :r], wr[:, :r], rtol=0, atol=1e-7 * wr.max())
    np.testing.assert_allclose(h[:r], hr[:r], rtol=0, atol=1e-7 * hr.max())
    c0 = c.k if variant == "zero" else r
    np.testing.assert_allclose(w[:, :c0] @ h[:c0], wr[:, :c0] @ hr[:c0], rtol=0, atol=1e-7 * (wr @ hr).max())


@pytest.mark.parametrize("cid", ["rank6-k10", "tiled8-k12"])
def test_mur_from_the_device_nndsvd_of_a_matrix_of_rank_below_k(cid, monkeypatch):
    from nmf_amd.mur import mur
    monkeypatch.setenv("NMFX_NNDSVD", "device")
    c = S.BY_ID[cid]
    res = mur(S.make_input(c).copy(), c.k, distance_type="eu", min_iter=5, max_iter=5, nndsvd_init=(True, "zero"))
    hist = np.asarray(res.obj_history, dtype=np.float64)
    assert np.isfinite(res.w).all() and np.isfinite(res.h).all() and np.isfinite(hist).all()
    assert len(hist) >= 5 and np.all(np.diff(hist) < 0), hist


def _cap_sweeps(monkeypatch, cap):
    from nmf_amd.engine import Engine
    orig = Engine.topk_svd

    def capped(self, k, block=0, tol=0.0, max_sweeps=0, seed=0):
        return orig(self, k, block=block, tol=tol, max_sweeps=cap, seed=seed)
    monkeypatch.setattr(Engine, "topk_svd", capped)


def test_nndsvd_falls_back_to_the_host_or_raises(monkeypatch, caplog):
    from nmf_amd import utils
    from nmf_amd.engine import Engine
    c = S.TWO_SWEEPS
    v = S.make_input(c)
    _cap_sweeps(monkeypatch, 2)
    want = utils.nndsvd(np.asarray(v), c.k, variant="zero")
    with Engine(c.m, c.n, c.k) as eng:
        eng.upload_v(v)
        monkeypatch.setenv("NMFX_NNDSVD", "auto")
        got = utils.nndsvd_device(eng, v, c.k, variant="zero")
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        monkeypatch.setenv("NMFX_NNDSVD", "device")
        with pytest.raises(RuntimeError, match="did not converge"):
            utils.nndsvd_device(eng, v, c.k, variant="zero")


# ---- refusals at the ABI ------------------------------------------------------------------------------------------------------
def _abi_call(eng, k, m, n, null=False):
    u = np.empty((m, max(k, 1))); s = np.empty(max(k, 1)); vt = np.empty((max(k, 1), n))
    sweeps, resid = C.c_int(), C.c_double()
    rc = eng.lib.nmfx_topk_svd(eng.h, k, 0, 0.0, 0, 0, None if null else u.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p),
                               vt.ctypes.data_as(C.c_void_p), C.byref(sweeps), C.byref(resid))
    return rc, eng.lib.nmfx_last_error(eng.h) or b""


def test_refusals_leave_the_handle_usable():
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    c = S.BY_ID["L32-k16"]
    v = S.make_input(c)
    with Engine(c.m, c.n, c.k) as eng:
        rc, msg = _abi_call(eng, c.k, c.m, c.n)
        assert rc == L.NMFX_E_STATE and b"upload V first" in msg
        eng.upload_v(v)
        for k, null, text in ((0, False, b"k must be at least 1"), (c.n + 1, False, b"k exceeds min(m, n)"), (c.k, True, b"must not be null")):
            rc, msg = _abi_call(eng, k, c.m, c.n, null=null)
            assert rc == L.NMFX_E_ARG and text in msg, (k, null, rc, msg)
            _hold(c, eng.topk_svd(c.k), label=f"{c.id} after a refusal")
    big = S.BY_ID["L192-plain-640x384-k150"]
    with Engine(big.m, big.n, big.k) as eng:
        eng.upload_v(S.make_input(big))
        rc, msg = _abi_call(eng, 193, big.m, big.n)
        assert rc == L.NMFX_E_ARG and b"k too large" in msg
        _hold(big, eng.topk_svd(big.k, **dict(big.kw)), label=f"{big.id} after a refusal")
