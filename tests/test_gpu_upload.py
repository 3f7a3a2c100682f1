"""Every way V and the weights reach the device (nmfx_upload_v, nmfx_upload_v_device, nmfx_upload_weights), and every solver
on a handle whose V changed under it.  Runs only on a real MI355X (`-m gpu`).

A wrong or stale copy of V gives a valid factorisation of the wrong matrix, which nothing downstream notices.  So:
  * one delivery per configuration (a single contiguous float32 upload) is compared with the float64 step,
    mur_step.check_steps at mur_step.BARS;
  * every other delivery of the same float32 values must give W_1, H_1, W_2, H_2 and the recorded objectives bit for bit
    (np.array_equal): the device holds the same V and the kernels are deterministic (the test_two_runs_bit_identical tests);
  * a used handle that receives new rows of V must afterwards equal, bit for bit, a fresh handle given the merged matrix.
No tolerance of its own: the bars are mur_step.BARS and, for the weighted step, those of tests/test_gpu_weighted.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import upload_cases as U
from mur_step import BARS, NEVER, OBJ_FLOOR, OBJ_RTOL, check_steps, compare, make_inputs, ref_h, ref_w
from upload_cases import M, N, NEW

pytestmark = pytest.mark.gpu


def _engine(*a, **kw):
    from nmf_amd.engine import Engine
    return Engine(*a, **kw)


# ---- a. one V, many deliveries ---------------------------------------------------------------------------------------------
CONFIGS = [(40, "bf16", "eu"), (40, "f32", "eu"), (40, "bf16", "kl"), (40, "f32", "kl"), (16, None, "eu"), (160, None, "eu")]
CONFIG_IDS = [f"k{k}-{p or 'default'}-{kind}" for k, p, kind in CONFIGS]


@functools.lru_cache(maxsize=None)
def baseline(k, precision, kind):
    """One contiguous float32 upload of the base problem, checked against the float64 step; computed once, never changed."""
    v, w0, h0 = U.base(k)
    runs, arith = U.run_mur(lambda eng: eng.upload_v(v), kind, k, precision, w0, h0)
    check_steps(kind, v, w0, h0, runs, 0.0, 0.0, BARS[(arith, kind)], tag=f"baseline k={k} {precision} {kind} ")
    return U.flat(runs)


@pytest.mark.parametrize("k,precision,kind", CONFIGS, ids=CONFIG_IDS)
def test_baseline_upload_against_the_float64_step(k, precision, kind):
    baseline(k, precision, kind)


@pytest.mark.parametrize("form,dt", U.HOST_DELIVERIES, ids=[f"{f}-{d}" for f, d in U.HOST_DELIVERIES])
@pytest.mark.parametrize("k,precision,kind", CONFIGS, ids=CONFIG_IDS)
def test_host_deliveries_equal_the_single_upload(k, precision, kind, form, dt):
    v, w0, h0 = U.base(k)
    runs, _ = U.run_mur(lambda eng: U.deliver_host(eng.upload_v, v, form, dt), kind, k, precision, w0, h0)
    U.same(U.flat(runs), baseline(k, precision, kind), f"upload_v {form} {dt}")


@pytest.mark.parametrize("dt,parts,ld", U.DEVICE_DELIVERIES, ids=[f"{d}-{p}-ld{l}" for d, p, l in U.DEVICE_DELIVERIES])
@pytest.mark.parametrize("k,precision,kind", CONFIGS, ids=CONFIG_IDS)
def test_device_deliveries_equal_the_single_upload(k, precision, kind, dt, parts, ld):
    v, w0, h0 = U.base(k)
    runs, _ = U.run_mur(lambda eng: U.deliver_device(eng, v, dt, parts, ld), kind, k, precision, w0, h0)
    U.same(U.flat(runs), baseline(k, precision, kind), f"upload_v_device {dt} {parts} ld={ld}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("k,precision,kind", CONFIGS, ids=CONFIG_IDS)
def test_sliding_window_view_equals_its_contiguous_copy(k, precision, kind, dt):
    """V is a Hankel view (rows one element apart); the baseline is its contiguous float32 copy."""
    view = U.hankel(U.NP_DTYPE[dt])
    assert view.shape == (M, N) and view.strides == (view.itemsize, view.itemsize)
    copy = np.ascontiguousarray(view, dtype=np.float32)
    _, w0, h0 = U.base(k)
    want, arith = U.run_mur(lambda eng: eng.upload_v(copy), kind, k, precision, w0, h0)
    check_steps(kind, copy, w0, h0, want, 0.0, 0.0, BARS[(arith, kind)], tag="hankel ")
    got, _ = U.run_mur(lambda eng: eng.upload_v(view), kind, k, precision, w0, h0)
    U.same(U.flat(got), U.flat(want), f"sliding-window view {dt}")


def rounding_matrix(huge):
    """Float64 values that float32 cannot represent, with the cases that pin round-to-nearest-even: the value halfway between
    two float32 numbers on either side of an even mantissa, a float64 subnormal, a value float32 holds only as a subnormal;
    huge: also one above FLT_MAX / 2."""
    v64 = np.random.default_rng(77).uniform(0.05, 1.0, (M, N))
    v64[10, 3] = 1.0 + 2.0 ** -24                   # halfway between 1 and 1 + 2^-23: to the even one, 1
    v64[10, 4] = 1.0 + 3 * 2.0 ** -24               # halfway between 1 + 2^-23 and 1 + 2^-22: to the even one, 1 + 2^-22
    v64[200, 150] = 5e-324                          # the smallest float64 subnormal: 0
    v64[130, 70] = 1e-310                           # a float64 subnormal: 0
    v64[131, 71] = 1e-40                            # a float32 subnormal
    if huge:
        v64[256, 199] = 2.5e38                      # above FLT_MAX / 2 = 1.7e38
    v32 = v64.astype(np.float32)
    assert v32[10, 3] == 1.0 and v32[10, 4] == np.float32(1.0 + 2.0 ** -22) and v32[200, 150] == 0 and v32[130, 70] == 0
    assert np.count_nonzero(v32.astype(np.float64) != v64) > 0.99 * v64.size
    return v64, v32


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("k,precision,kind", [(40, "bf16", "eu"), (40, "f32", "kl"), (16, None, "eu")])
def test_float64_is_rounded_to_nearest_even(k, precision, kind, path):
    """Both conversions on the device (copy_rows_in and nmfx_upload_v_device) round as numpy's astype(float32) does."""
    v64, v32 = rounding_matrix(huge=False)
    _, w0, h0 = U.base(k)
    want, arith = U.run_mur(lambda eng: eng.upload_v(v32), kind, k, precision, w0, h0)
    check_steps(kind, v32, w0, h0, want, 0.0, 0.0, BARS[(arith, kind)], tag="rounded ")
    deliver = (lambda eng: eng.upload_v(v64)) if path == "host" else (lambda eng: U.deliver_device(eng, v64, "f64", "whole", N))
    got, _ = U.run_mur(deliver, kind, k, precision, w0, h0)
    U.same(U.flat(got), U.flat(want), f"float64 through the {path} path")


@pytest.mark.parametrize("path", ["host", "device"])
def test_float64_above_half_flt_max_arrives(path):
    """A value above FLT_MAX / 2.  Every product that sums over rows overflows with it, so only W_1 of a Euclidean step is
    compared: row r of W_1 depends on row r of V alone, stays finite (2.5e38 x h, h < 1), and sees every entry of V."""
    v64, v32 = rounding_matrix(huge=True)
    _, w0, h0 = U.base(16)
    out = {}
    for name, deliver in (("f32", lambda eng: eng.upload_v(v32)),
                          ("f64", (lambda eng: eng.upload_v(v64)) if path == "host" else (lambda eng: U.deliver_device(eng, v64, "f64", "whole", N)))):
        with _engine(M, N, 16) as eng:
            deliver(eng)
            eng.set_factors(w0, h0)
            eng.mur_run(U.code("eu"), 0.0, 0.0, NEVER, 0, 0, 0, 1)
            out[name] = eng.get_factors()[0]
    assert np.isfinite(out["f32"]).all() and out["f32"][256].max() > 1e35
    _, msg = compare("W1 with a value above FLT_MAX / 2", out["f32"], ref_w("eu", v32, w0, h0, 0.0), BARS[("f32", "eu")])
    assert msg is None, msg
    assert np.array_equal(out["f64"], out["f32"])


# ---- b. tall and narrow float64 ----------------------------------------------------------------------------------------------
TALL = (70001, 100, 16)     # more rows than one grid.y holds, fewer than 128 columns: one 64 MiB staging chunk would be 83,886 rows


@functools.lru_cache(maxsize=None)
def tall_inputs():
    m, n, k = TALL
    v, w0, h0 = make_inputs(m, n, k, seed=8300)
    return v, w0, h0


@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_tall_narrow_float64_upload(kind):
    m, n, k = TALL
    v, w0, h0 = tall_inputs()
    v64 = v.astype(np.float64)
    want, arith = U.run_mur(lambda eng: eng.upload_v(v), kind, k, None, w0, h0, m=m, n=n)
    got, _ = U.run_mur(lambda eng: eng.upload_v(v64), kind, k, None, w0, h0, m=m, n=n)
    check_steps(kind, v, w0, h0, got, 0.0, 0.0, BARS[(arith, kind)], tag=f"tall float64 {kind} ")
    U.same(U.flat(got), U.flat(want), "tall float64 upload_v")
    if kind == "eu":                                # the device conversion walks the same row chunks
        dev, _ = U.run_mur(lambda eng: U.deliver_device(eng, v64, "f64", "whole", n), kind, k, None, w0, h0, m=m, n=n)
        U.same(U.flat(dev), U.flat(want), "tall float64 upload_v_device")


@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_tall_narrow_float64_weights(kind):
    """All-ones weights as float64 against all-ones weights as float32 (both on the weighted kernels of kernels_phase.hip; the
    unweighted run takes other kernels and need not agree bit for bit)."""
    m, n, k = TALL
    v, w0, h0 = tall_inputs()
    out = {}
    for dt in (np.float32, np.float64):
        def deliver(eng, dt=dt):
            eng.upload_v(v)
            eng.upload_weights(np.ones((m, n), dtype=dt))
        out[dt], _ = U.run_mur(deliver, kind, k, None, w0, h0, m=m, n=n)
    U.same(U.flat(out[np.float64]), U.flat(out[np.float32]), "tall float64 upload_weights")


# ---- c. new rows on a used handle ----------------------------------------------------------------------------------------------
def _mur(kind, lw=0.0, lh=0.0):
    return lambda eng, w0, h0: U.flat(U.drive(eng, kind, w0, h0, lw, lh))


# name -> (k, precision, solver, set-up of the handle, what else the case needs)
USED = {
    "mur-eu-k40-bf16": (40, "bf16", _mur("eu"), {}),
    "mur-eu-k40-f32": (40, "f32", _mur("eu"), {}),
    "mur-kl-k40-bf16": (40, "bf16", _mur("kl"), {}),
    "mur-kl-k40-f32": (40, "f32", _mur("kl"), {}),
    "mur-eu-k160-bf16": (160, "bf16", _mur("eu"), {}),
    "mur-eu-k160-f32": (160, "f32", _mur("eu"), {}),
    "mur-kl-k160-bf16": (160, "bf16", _mur("kl"), {}),
    "mur-kl-k160-f32": (160, "f32", _mur("kl"), {}),
    "mur-eu-k16": (16, None, _mur("eu"), {}),
    "mur-kl-k16": (16, None, _mur("kl"), {}),
    "pair": (128, None, U.solver_pair, dict(kstart=64)),
    "phase-is": (40, None, _mur("is"), dict(positive=True)),
    "phase-beta1.5": (40, None, _mur("beta"), dict(beta=1.5)),
    "phase-weighted-eu": (40, None, _mur("eu"), dict(weighted=True)),
    "hals": (40, None, U.solver_hals, {}),
    "hals-stack": (40, None, U.solver_hals_stack, {}),
    "anls": (40, None, U.solver_anls, {}),
    "aoadmm-eu": (40, None, U.solver_aoadmm, {}),
    "admm-eu": (40, None, U.solver_admm("eu"), {}),
    "admm-kl": (40, None, U.solver_admm("kl"), {}),
    "svd": (40, None, U.solver_svd, dict(warm=True)),
    "objective-f64": (40, None, U.solver_objective_f64, dict(warm=True)),
}
MUR_KIND = {name: name.split("-")[1] for name in USED if name.startswith("mur-")}


def used_and_fresh(name, k, precision, solver, opt):
    """(result of the used handle after rows NEW of V_b arrived, result of a fresh handle on the merged matrix, merged, W0, H0)."""
    positive = opt.get("positive", False)
    kstart = opt.get("kstart", k)
    va, w0, h0 = U.base(kstart, 0, positive)
    vb = U.base(kstart, 1, positive)[0]
    oma, omb = U.weights(0), U.weights(1)
    r0, r1 = NEW
    both = U.merged(va, vb)

    def setup(eng):
        if precision is not None:
            eng.set_precision(precision)
        if "beta" in opt:
            eng.set_beta(opt["beta"])

    with _engine(M, N, k) as eng:
        setup(eng)
        eng.upload_v(va)
        if opt.get("weighted"):
            eng.upload_weights(oma)
        if opt.get("warm"):                         # two iterations first, so that every derived copy of V_a exists
            U.drive(eng, "eu", w0, h0, steps=(2,))
        first = solver(eng, w0, h0)
        eng.upload_v(vb[r0:r1], row0=r0)
        if opt.get("weighted"):
            eng.upload_weights(omb[r0:r1], row0=r0)
        got = solver(eng, w0, h0)
    with _engine(M, N, k) as eng:
        setup(eng)
        eng.upload_v(both)
        if opt.get("weighted"):
            eng.upload_weights(U.merged(oma, omb))
        want = solver(eng, w0, h0)
    assert not all(np.array_equal(a, b) for a, b in zip(first, want)), f"{name}: the new rows change nothing: the case cannot see a stale copy"
    return got, want, both, w0, h0


@pytest.mark.parametrize("name", list(USED))
def test_new_rows_on_a_used_handle(name):
    k, precision, solver, opt = USED[name]
    got, want, both, w0, h0 = used_and_fresh(name, k, precision, solver, opt)
    U.same(got, want, f"{name}: used handle with new rows {NEW} against a fresh handle on the merged matrix")
    if name in MUR_KIND:
        kind = MUR_KIND[name]
        arith = "f32" if k == 16 else precision
        runs = {1: got[0:3], 2: got[3:6]}
        check_steps(kind, both, w0, h0, runs, 0.0, 0.0, BARS[(arith, kind)], tag=f"{name} on the merged matrix ")


@pytest.mark.parametrize("drop", [None, "1"], ids=["kept", "dropped"])
@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_new_rows_between_two_runs_without_set_factors(kind, drop, monkeypatch):
    """mur_run(0, 2), new rows of V, mur_run(2, 1): the only place where what a handle keeps across calls (kl_h_iter, the images
    and partials of the KL epilogue) meets a changed V, and the only one where the upload's own clearing of bf_ready decides
    whether Vt / Vtile are rebuilt (nmfx_set_factors clears it too).  W_3 and H_3 against the float64 step on the merged
    matrix, fed the device's own W_2 and H_2.  dropped: the same with the row-major V freed after the first prepare
    (NMFX_DROP_V=1), so that the rows go into a V rebuilt from Vtile."""
    if drop:
        monkeypatch.setenv("NMFX_DROP_V", drop)
    k = 40
    va, w0, h0 = U.base(k, 0)
    vb = U.base(k, 1)[0]
    both = U.merged(va, vb)
    r0, r1 = NEW
    with _engine(M, N, k) as eng:
        eng.set_precision("bf16")
        assert eng.precision() == "bf16"
        eng.upload_v(va)
        eng.set_factors(w0, h0)
        eng.mur_run(U.code(kind), 0.0, 0.0, NEVER, 0, 0, 0, 2)
        w2, h2 = eng.get_factors()
        eng.upload_v(vb[r0:r1], row0=r0)
        eng.mur_run(U.code(kind), 0.0, 0.0, NEVER, 0, 0, 2, 1)
        eng.mur_finish(U.code(kind), NEVER, 0, 0, 3)
        w3, h3 = eng.get_factors()
    bar = BARS[("bf16", kind)]
    fails = [msg for _, msg in (compare(f"{kind} W3 after new rows", w3, ref_w(kind, both, w2, h2, 0.0), bar),
                                compare(f"{kind} H3 after new rows", h3, ref_h(kind, both, w3, h2, 0.0), bar)) if msg]
    assert not fails, "\n".join(fails)


# ---- d. dropped row-major V ------------------------------------------------------------------------------------------------------
def test_dropped_v_partial_upload(monkeypatch):
    monkeypatch.setenv("NMFX_DROP_V", "1")
    for kind in ("eu", "kl"):
        got, want, both, w0, h0 = used_and_fresh(f"dropped {kind}", 40, "bf16", _mur(kind), {})
        U.same(got, want, f"dropped V, {kind}: new rows {NEW} against a fresh handle on the merged matrix")
        check_steps(kind, both, w0, h0, {1: got[0:3], 2: got[3:6]}, 0.0, 0.0, BARS[("bf16", kind)], tag=f"dropped V {kind} ")


@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_dropped_v_switch_to_f32(kind, monkeypatch):
    monkeypatch.setenv("NMFX_DROP_V", "1")
    v, w0, h0 = U.base(40)
    with _engine(M, N, 40) as eng:
        eng.set_precision("bf16")
        eng.upload_v(v)
        U.drive(eng, kind, w0, h0, steps=(2,))
        eng.set_precision("f32")
        runs = U.drive(eng, kind, w0, h0)
    check_steps(kind, v, w0, h0, runs, 0.0, 0.0, BARS[("f32", kind)], tag=f"dropped V then f32 {kind} ")


@pytest.mark.parametrize("name", ["hals", "objective-f64", "svd"])
def test_dropped_v_other_consumers(name, monkeypatch):
    """Each consumer of the row-major V behind two split-bf16 iterations that dropped it: what it gives with the copy kept."""
    solver = USED[name][2]
    v, w0, h0 = U.base(40)
    out = {}
    for drop in ("1", "0"):
        monkeypatch.setenv("NMFX_DROP_V", drop)
        with _engine(M, N, 40) as eng:
            eng.set_precision("bf16")
            eng.upload_v(v)
            U.drive(eng, "eu", w0, h0, steps=(2,))
            out[drop] = solver(eng, w0, h0)
    U.same(out["1"], out["0"], f"{name} with the row-major V dropped against the same handle with it kept")


# ---- e. weights ------------------------------------------------------------------------------------------------------------------
WKINDS = ("eu", "kl", "is")


def weighted_problem():
    """(V, weights, W0, H0): weight 0 wherever V is 0, so that every loss has a value in every weighted cell."""
    v, w0, h0 = U.base(40)
    om = np.where(v > 0, U.weights(0), np.float32(0)).astype(np.float32)
    return v, om, w0, h0


def run_weighted(kind, deliver_weights):
    v, om, w0, h0 = weighted_problem()

    def deliver(eng):
        eng.upload_v(v)
        deliver_weights(eng, om)
    return U.run_mur(deliver, kind, 40, None, w0, h0)[0]


@functools.lru_cache(maxsize=None)
def weighted_baseline(kind):
    return U.flat(run_weighted(kind, lambda eng, om: eng.upload_weights(om)))


@pytest.mark.parametrize("form,dt", U.HOST_DELIVERIES, ids=[f"{f}-{d}" for f, d in U.HOST_DELIVERIES])
@pytest.mark.parametrize("kind", WKINDS)
def test_weight_deliveries_equal_the_single_upload(kind, form, dt):
    runs = run_weighted(kind, lambda eng, om: U.deliver_host(eng.upload_weights, om, form, dt))
    U.same(U.flat(runs), weighted_baseline(kind), f"upload_weights {form} {dt}")


@pytest.mark.parametrize("kind", WKINDS)
def test_rows_never_uploaded_weigh_zero(kind):
    from weighted_ref import weighted_h_step, weighted_objective, weighted_w_step
    v, om, w0, h0 = weighted_problem()
    r0, r1 = NEW
    holed = om.copy()
    holed[r0:r1] = 0

    def two_blocks(eng, om):
        eng.upload_weights(om[:r0], row0=0)
        eng.upload_weights(om[r1:], row0=r1)
    got = run_weighted(kind, two_blocks)
    want = run_weighted(kind, lambda eng, om: eng.upload_weights(holed))
    U.same(U.flat(got), U.flat(want), "weights of rows [0,100) and [140,257) against the full upload with zeros between")
    assert not np.array_equal(got[2][0], np.asarray(weighted_baseline(kind)[3]))          # (the hole matters)
    # ... and against the float64 weighted step, at the bars of tests/test_gpu_weighted.py
    bar = BARS[("f32", "kl" if kind == "is" else kind)]
    x, omd = v.astype(np.float64), holed.astype(np.float64)
    fails, iterate = [], {0: (w0, h0)}
    for s in sorted(got):
        ws, hs, _ = got[s]
        wp, hp = iterate[s - 1]
        for label, dev, ref in ((f"W{s}", ws, weighted_w_step(kind, x, omd, wp, hp, 0.0)), (f"H{s}", hs, weighted_h_step(kind, x, omd, ws, hp, 0.0))):
            err, msg = compare(f"weights with a hole, {kind} {label}", dev, ref, bar)
            print(f"weights with a hole, {kind} {label}: {err:.2e} (bar {bar:.0e})")
            if msg:
                fails.append(msg)
        iterate[s] = (ws, hs)
    scale = {"eu": OBJ_FLOOR * 0.5 * float(np.sum(omd * x * x)), "kl": OBJ_FLOOR * float(np.sum(omd * x)), "is": 0.0}[kind]
    for s, (_, _, hist) in sorted(got.items()):
        for i in range(s + 1):
            ref = weighted_objective(kind, x, omd, *iterate[i])
            rel = abs(float(hist[i]) - ref) / max(abs(ref), scale)
            print(f"weights with a hole, {kind} obj[{i}] of the {s}-step run: {rel:.2e} (bar {OBJ_RTOL:.0e})")
            if not rel <= OBJ_RTOL:
                fails.append(f"{kind} obj[{i}] of the {s}-step run: recorded {hist[i]!r}, float64 {ref!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    assert not fails, "\n".join(fails)
    assert (got[2][0][r0:r1] == 0).all()            # no weight in the row: W is exactly 0 there


# ---- f. refusals -----------------------------------------------------------------------------------------------------------------
def _bad_calls(fn, src, n):
    """(what, call) for one upload entry point: every refusal of its argument check."""
    from nmf_amd import _lib as L
    return [("row0 + rows > m", lambda h: fn(h, src, L.F32, n, 250, 8)),
            ("row0 + rows > m, row0 = m", lambda h: fn(h, src, L.F32, n, M, 1)),
            ("row0 < 0", lambda h: fn(h, src, L.F32, n, -1, 8)),
            ("rows < 0", lambda h: fn(h, src, L.F32, n, 0, -1)),
            ("ld < n", lambda h: fn(h, src, L.F32, n - 1, 0, 8)),
            ("ld = 1", lambda h: fn(h, src, L.F32, 1, 0, 8)),
            ("NULL source", lambda h: fn(h, None, L.F32, n, 0, 8)),
            ("dtype 2", lambda h: fn(h, src, 2, n, 0, 8)),
            ("dtype -1", lambda h: fn(h, src, -1, n, 0, 8))]


@pytest.mark.parametrize("weighted", [False, True], ids=["v", "weights"])
def test_refused_uploads_change_nothing(weighted):
    import torch
    from nmf_amd import _lib as L
    lib = L.require_gpu()
    v, om, w0, h0 = weighted_problem()
    junk = np.full((M, N), 3.25, dtype=np.float32)
    dev = torch.from_numpy(junk).cuda()
    torch.cuda.synchronize()
    host_ptr, dev_ptr = junk.ctypes.data_as(C.c_void_p), C.c_void_p(dev.data_ptr())
    with _engine(M, N, 40) as eng:
        eng.upload_v(v)
        if weighted:
            eng.upload_weights(om)
            entries = [("upload_weights", lib.nmfx_upload_weights, host_ptr)]
        else:
            entries = [("upload_v", lib.nmfx_upload_v, host_ptr), ("upload_v_device", lib.nmfx_upload_v_device, dev_ptr)]
        before = U.flat(U.drive(eng, "kl", w0, h0))
        for name, fn, src in entries:
            for what, call in _bad_calls(fn, src, N):
                rc = call(eng.h)
                msg = lib.nmfx_last_error(eng.h)
                assert rc == L.NMFX_E_ARG and name.encode() in msg, (name, what, rc, msg)
            assert fn(eng.h, src, L.F32, N, 10, 0) == L.NMFX_OK, name         # rows == 0: nothing to do, nothing changed
            assert fn(eng.h, src, L.F64, N, M, 0) == L.NMFX_OK, name
        after = U.flat(U.drive(eng, "kl", w0, h0))
    U.same(after, before, "a run after the refused uploads against the run before them")
    del dev
