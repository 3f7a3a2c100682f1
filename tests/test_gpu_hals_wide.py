"""nmf_amd.hals.hals_wide on the device: the public call against the float64 host loop of tests/test_gpu_hals.py, the monotone
objective of exact coordinate descent, the reported objective, the start, and the NMF front end beyond 128 components.  Single
half-steps, problem by problem: tests/test_gpu_hals_wide_step.py."""
import math
import os

import numpy as np
import pytest

import anls_step as A
import hals_step as HS
import hals_wide_step as HW
from test_gpu_hals import host_alpha, host_hals, planted

pytestmark = pytest.mark.gpu


# ---- the public call against the float64 loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,sweeps", HW.PUBLIC_CASES, ids=[HW.public_id(*c) for c in HW.PUBLIC_CASES])
def test_public_call_matches_the_float64_loop(m, n, k, sweeps):
    """Same start (the seeded uniform draw, scaled by the float64 alpha), 5 iterations, lambda on both sides: the bars of
    tests/test_gpu_hals.py, the final product within 1e-4 of ||V|| and the history at rtol 2e-4 (the emulated trajectory stays
    under half of both: tests/test_hals_wide_step_bars.py)."""
    from nmf_amd.hals import hals_wide
    v = HW.public_v(m, n, k)
    lw, lh = HW.PUBLIC_LAMS
    w0, h0 = HW.public_start(m, n, k)
    a = host_alpha(v, w0, h0)
    wr, hr, hist = host_hals(v, A.f32(w0 * math.sqrt(a)), A.f32(h0 * math.sqrt(a)), lw, lh, sweeps, HW.PUBLIC_ITERS)
    np.random.seed(HW.PUBLIC_SEED)
    keep = v.copy()
    res = hals_wide(v, k, sweeps=sweeps, lambda_w=lw, lambda_h=lh, max_iter=HW.PUBLIC_ITERS, nndsvd_init=(False, "zero"))
    assert np.array_equal(v, keep)
    assert res.i == HW.PUBLIC_ITERS - 1 and len(res.obj_history) == res.i + 2
    assert res.w.shape == (m, k) and res.h.shape == (k, n) and (res.w >= 0).all() and (res.h >= 0).all()
    assert abs(hals_wide.last_alpha - a) <= 1e-6 * a
    err = np.linalg.norm(res.w @ res.h - wr @ hr) / np.linalg.norm(v.astype(np.float64))
    rel = float(np.max(np.abs(np.asarray(res.obj_history) / hist - 1)))
    print(f"{m} x {n}, k = {k}, sweeps = {sweeps}: WH error {err:.3e}, history {rel:.3e}")
    assert err < HW.PUBLIC_WH_BAR, err
    np.testing.assert_allclose(res.obj_history, hist, rtol=HW.PUBLIC_HIST_RTOL)
    exp = res.experiment
    assert (exp.method, exp.components, exp.sweeps, exp.distance_type, exp.lambda_w) == ("hals", k, sweeps, "eu", lw)


def test_kl_only_selects_the_reported_objective():
    from nmf_amd.hals import hals_wide
    v = planted(160)
    out = {}
    for kind in ("eu", "kl"):
        np.random.seed(5)
        out[kind] = hals_wide(v, 160, distance_type=kind, max_iter=4, nndsvd_init=(False, "zero"))
    assert np.array_equal(out["eu"].w, out["kl"].w) and np.array_equal(out["eu"].h, out["kl"].h)
    want = HS.objective("kl", v, out["kl"].w, out["kl"].h)
    assert abs(out["kl"].obj_history[-1] - want) <= HS.OBJ_RTOL * abs(want)
    assert out["kl"].experiment.distance_type == "kl"


# ---- exact coordinate descent cannot increase the objective ---------------------------------------------------------------------
@pytest.mark.parametrize("k", [160, 300])
def test_objective_is_monotone(k):
    from nmf_amd.hals import hals_wide
    np.random.seed(2)
    res = hals_wide(planted(k), k, min_iter=40, max_iter=40, nndsvd_init=(False, "zero"))
    obj = np.asarray(res.obj_history)
    assert len(obj) == 41 and res.i == 39
    up = obj[1:] / obj[:-1] - 1
    assert (obj[1:] <= obj[:-1] * (1 + 1e-6)).all(), f"iteration {int(np.argmax(up))}: {up.max():.2e}"


# ---- rescale_start ---------------------------------------------------------------------------------------------------------------
def test_without_rescale_the_start_is_bit_exact():
    """rescale_start=False: one iteration of the public call is one iteration of the engine from the seeded draw itself."""
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    from nmf_amd.hals import hals_wide
    k = 160
    v = planted(k)
    np.random.seed(4)
    w0, h0 = np.random.rand(*(v.shape[0], k)), np.random.rand(*(k, v.shape[1]))
    np.random.seed(4)
    res = hals_wide(v, k, rescale_start=False, max_iter=1, nndsvd_init=(False, "zero"))
    assert hals_wide.last_alpha is None
    with Engine(v.shape[0], v.shape[1], k) as eng:
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        eng.anls_set_distance(L.EU)
        eng.hals_wide_run(0, 0, 1, 10, 1e-3, 1e-3, 0, 1)
        w, h = eng.get_factors()
    assert np.array_equal(res.w, w) and np.array_equal(res.h, h)
    np.random.seed(4)
    scaled = hals_wide(v, k, rescale_start=True, max_iter=1, nndsvd_init=(False, "zero"))
    assert not np.array_equal(scaled.w, w)


# ---- the NMF front end -----------------------------------------------------------------------------------------------------------
def test_nmf_factorize_hals_beyond_128(tmp_path):
    """factorize('hals') routes dense, unmasked data with k > 128 to hals_wide: the default start (NNDSVD), 12 iterations."""
    from nmf_amd.hals import hals_wide
    from nmf_amd.nmf import NMF
    v = planted(160)
    hals_wide.last_alpha = "unset"
    nmf = NMF(v, 160)
    nmf.factorize("hals", max_iter=12)
    assert hals_wide.last_alpha != "unset"               # (hals_wide ran)
    assert nmf.w.shape == (v.shape[0], 160) and nmf.h.shape == (160, v.shape[1]) and nmf.results.experiment.method == "hals"
    assert nmf.results.experiment.components == 160 and len(nmf.results.obj_history) >= 2
    assert nmf.results.obj_history[-1] < nmf.results.obj_history[0]
    nmf.save_factorization(save_dir=str(tmp_path))
    files = os.listdir(tmp_path)
    assert len(files) == 1 and files[0].startswith("nmf_hals_160_eu_") and files[0].endswith(".npz")
