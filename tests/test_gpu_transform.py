"""Fold-in on the device (nmfx_foldin_run, kernels_phase.hip) against the float64 statement of tests/transform_ref.py.
Runs only on a real MI355X (`-m gpu`).

Bars.  H steps: mur_step.BARS[("f32", "kl")] = 2e-5, the project's bar for exact-f32 kernels; where the yardstick is exactly
0 the device must be exactly 0.  Recorded objective: mur_step.OBJ_RTOL (1e-5), relative to max(|objective|, OBJ_FLOOR x the
data scale) with the data scale of each loss as tests/test_gpu_beta.py and tests/test_gpu_weighted.py take it (1/2 Sum om
x^2 for 'eu', Sum om x for 'kl', 0 for 'is', Sum om x^beta / |beta (beta - 1)| for 'beta').  Whole runs: the project's
WH_TOL.  Every comparison prints its figure before it asserts.

The measured maxima belong in DESIGN.md 4.7."""
import numpy as np
import pytest
import scipy.sparse as sp

from gpu_common import WH_TOL, wh_error
from mur_step import BARS, NEVER, OBJ_FLOOR, OBJ_RTOL, compare, make_inputs
from oracle import nmf_ref as R
from transform_ref import h_step, objective, transform_ref
from weighted_cases import log_uniform_weights, stop_margins

pytestmark = pytest.mark.gpu

BAR = BARS[("f32", "kl")]
CODES = {"eu": "EU", "kl": "KL", "is": "IS", "beta": "BETA"}


def _transform(*a, **kw):
    from nmf_amd.transform import transform
    return transform(*a, **kw)


def code_of(kind):
    from nmf_amd import _lib as L
    return getattr(L, CODES[kind])


def drive(eng, code, w0, h0, lh, steps=(1, 2)):
    """The calls nmf_amd.transform.transform makes, with the stop rule off: {s: (W, H_s, recorded objectives 0 .. s)}."""
    out = {}
    for s in steps:
        eng.set_factors(w0, h0)
        eng.foldin_run(code, lh, NEVER, 0, 0, 0, s)
        eng.foldin_finish(code, NEVER, 0, 0, s)
        w, h = eng.get_factors()
        out[s] = (w, h, eng.objectives(0, s + 1))
    return out


def data_scale(kind, x, om, beta):
    omd = np.ones(x.shape) if om is None else om
    with np.errstate(invalid="ignore"):
        xo = np.where(omd > 0, x, 0.0)
    if kind == "eu":
        return 0.5 * float(np.sum(omd * xo * xo))
    if kind == "kl" or (kind == "beta" and beta == 1):
        return float(np.sum(omd * xo))
    if kind == "is" or beta == 0:
        return 0.0
    live = (omd > 0) & (xo > 0) if beta < 0 else omd > 0
    return float(np.sum(omd[live] * xo[live] ** beta)) / abs(beta * (beta - 1.0))


def check(tag, kind, x, om, beta, w0, h0, lh, runs):
    """W read back = the f32 image of w, bit for bit; every H step against the yardstick fed the device's previous H; every
    recorded objective against the float64 objective of (w, H_i).  Returns the worst figures; raises naming every failure."""
    fails, worst, iterate = [], {}, {0: h0}
    w32 = w0.astype(np.float32).astype(np.float64)
    for s in sorted(runs):
        ws, hs, _ = runs[s]
        if not np.array_equal(ws, w32):
            fails.append(f"{tag}: W after {s} steps is not the f32 image of w ({int((ws != w32).sum())} entries differ)")
        err, msg = compare(f"{tag} H{s}", hs, h_step(kind, x, w32, iterate[s - 1], lh, om, beta), BAR)
        worst[f"H{s}"] = err
        if msg:
            fails.append(msg)
        iterate[s] = hs
    scale = OBJ_FLOOR * data_scale(kind, x, om, beta)
    for s, (_, _, hist) in sorted(runs.items()):
        for i in range(s + 1):
            want = objective(kind, x, w32, iterate[i], om, beta)
            rel = abs(float(hist[i]) - want) / max(abs(want), scale)
            worst[f"obj[{i}]/{s}"] = rel
            if not rel <= OBJ_RTOL:
                fails.append(f"{tag} obj[{i}] of the {s}-step run: recorded {hist[i]!r}, float64 {want!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    print(f"{tag}: worst relative errors", {key: f"{val:.2e}" for key, val in worst.items()})
    assert not fails, "\n".join(fails)
    return worst


# ---- 1. H steps element by element -----------------------------------------------------------------------------------------
# (m, n, k, lambda_h, betas): padded ranks 16, 32, 64, 64, 128; n = 1; ragged edges.  Every padded rank sees a beta of each
# gamma branch (beta < 1, 1 <= beta <= 2, beta > 2) and both limit forms of the objective (beta = 0, beta = 1).
SHAPES = [(127, 1, 3, 0.0, (0.0, 1.0, 2.5)), (130, 70, 20, 0.02, (0.0, 1.0, 3.0)), (300, 200, 33, 0.1, (-1.0, 1.5, 3.0)),
          (257, 130, 64, 0.0, (0.0, 1.0, 2.5)), (640, 384, 128, 0.3, (0.0, 1.0, 2.5))]
PLAIN = [(m, n, k, lh, kind, None) for m, n, k, lh, _ in SHAPES for kind in ("eu", "kl", "is")]
PLAIN += [(m, n, k, lh, "beta", b) for m, n, k, lh, bs in SHAPES for b in bs]


def h_splits(m, n, k, ncu=256):
    """phase_splits of kernels_phase.hip for the H-side grid: splits of the contracted dimension m."""
    kp = 16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128
    mp, np_ = -(-m // 128) * 128, -(-n // 128) * 128
    blocks_x = np_ // (16 * (2 if kp == 128 else 4))
    want = -(-2 * ncu // blocks_x)
    return max(1, min(want, 16, (mp // 16) // 8))


def test_the_shapes_reach_every_padded_rank_and_both_split_regimes():
    assert h_splits(127, 1, 3) == 1 and h_splits(257, 130, 64) > 1 and h_splits(640, 384, 128) > 1
    for kp in (16, 32, 64, 128):
        bs = {b for m, n, k, lh, kind, b in PLAIN if kind == "beta" and (16 if k <= 16 else 32 if k <= 32 else 64 if k <= 64 else 128) == kp}
        assert {0.0, 1.0} <= bs and any(b < 1 for b in bs) and any(1 <= b <= 2 for b in bs) and any(b > 2 for b in bs), (kp, bs)
    assert {c[3] == 0 for c in PLAIN} == {True, False}


def plain_inputs(m, n, k, kind, beta, seed):
    """make_inputs with exact zeros scattered in W0 and H0.  'eu', 'kl' and beta > 0: about 30 % of V are exact zeros (zeros
    are data there), plus -- m, n >= 8 -- an all-zero row and column.  'is' and beta <= 0: V strictly positive."""
    v, w0, h0 = make_inputs(m, n, k, seed=seed, zeros=True)
    if kind in ("eu", "kl") or (kind == "beta" and beta > 0):
        rng = np.random.default_rng(seed + 1)
        v[rng.random(v.shape) < 0.3] = 0
        if m >= 8 and n >= 8:
            v[1, :] = 0
            v[:, 2] = 0
    return v, w0, h0


@pytest.mark.parametrize("m,n,k,lh,kind,beta", PLAIN)
def test_h_steps_element_by_element(m, n, k, lh, kind, beta):
    from nmf_amd.engine import Engine
    v, w0, h0 = plain_inputs(m, n, k, kind, beta, seed=7000 + k)
    x = v.astype(np.float64)
    with Engine(m, n, k) as eng:
        eng.upload_v(v)
        if kind == "beta":
            eng.set_beta(beta)
        runs = drive(eng, code_of(kind), w0, h0, lh)
        assert "fold-in" in eng.note() and "exact-f32" in eng.note(), eng.note()
    check(f"{kind} beta={beta} {m}x{n} k={k}", kind, x, None, beta, w0, h0, lh, runs)
    zero = h0 == 0                                                  # exact zeros of the start stay exact zeros
    for s in runs:
        assert np.isfinite(runs[s][1]).all() and (runs[s][1][zero] == 0).all()
        if (kind in ("eu", "kl") or (kind == "beta" and beta > 0)) and m >= 8 and n >= 8:
            assert (runs[s][1][:, 2] == 0).all()                   # an all-zero column of V: exactly 0


# ---- 2. the same with weights ----------------------------------------------------------------------------------------------
WEIGHTED = [(m, n, k, lh, kind, b) for kind, b in (("eu", None), ("kl", None), ("is", None), ("beta", 0.5))
            for m, n, k, lh in [(300, 200, 33, 0.1), (257, 130, 64, 0.0), (640, 384, 128, 0.3)]]


@pytest.mark.parametrize("m,n,k,lh,kind,beta", WEIGHTED)
def test_weighted_h_steps_element_by_element(m, n, k, lh, kind, beta):
    from nmf_amd import weighted
    from nmf_amd.engine import Engine
    v, w0, h0 = make_inputs(m, n, k, seed=8000 + k, zeros=True)
    om = log_uniform_weights((m, n), seed=9000 + k, edges=True)
    x = v.astype(np.float64)
    x[om == 0] = np.nan                                            # never read: the device receives 0 there
    x32, w32 = weighted.prepare(x, om, k, kind, beta=beta)
    with Engine(m, n, k) as eng:
        eng.upload_v(x32)
        eng.upload_weights(w32)
        if kind == "beta":
            eng.set_beta(beta)
        runs = drive(eng, code_of(kind), w0, h0, lh)
    check(f"weighted {kind} beta={beta} {m}x{n} k={k}", kind, x, om.astype(np.float64), beta, w0, h0, lh, runs)
    for s in runs:                                                 # a column without any weight: exactly 0, no NaN
        assert np.isfinite(runs[s][1]).all() and (runs[s][1][:, 3] == 0).all()


# ---- 3. whole runs ---------------------------------------------------------------------------------------------------------
def run_data(seed=3):
    """(x 300 x 200 strictly positive, a dictionary w 300 x 12)."""
    x = R.planted_matrix(300, 200, 12, seed=seed, dtype=np.float64) + 0.01
    return x, np.random.RandomState(21).uniform(0.1, 1.0, (300, 12))


@pytest.mark.parametrize("kind,beta,pattern", [("kl", None, False), ("is", None, False), ("beta", 1.5, False), ("beta", 0.5, True)])
def test_run_against_the_float64_run(kind, beta, pattern):
    x, w = run_data()
    om = None
    if pattern:                                                    # a 0 / 1 hold-out pattern, NaN where nothing is known
        om = (np.random.RandomState(7).rand(*x.shape) < 0.7).astype(np.float64)
        x = np.where(om > 0, x, np.nan)
    keep = x.copy(), w.copy()
    np.random.seed(4)
    got = _transform(x, w, distance_type=kind, beta=beta, weights=om, min_iter=30, max_iter=30)
    np.random.seed(4)
    want = transform_ref(x, w, kind, beta=beta, om=om, min_iter=30, max_iter=30)
    assert got.i == want.i == 29 and len(got.obj_history) == len(want.obj_history) == 31
    err = wh_error(w, got.h, w, want.h, np.nan_to_num(x))
    hist = np.asarray(got.obj_history)
    rel = np.max(np.abs(hist - want.obj_history) / np.abs(want.obj_history))
    print(f"fold-in run ({kind}, beta={beta}, pattern={pattern}): wh_error {err:.2e}, history rel {rel:.2e}, "
          f"largest step of the history {np.diff(hist).max():.3e}")
    assert err < WH_TOL
    assert rel <= OBJ_RTOL
    assert np.all(np.diff(hist) <= 0)                              # lambda_h = 0: the MM step never increases it
    assert got.h.shape == (12, 200) and got.h.dtype == np.float64 and (got.h >= 0).all()
    assert got.experiment.method == "transform" and got.experiment.distance_type == kind
    if kind == "beta":
        assert got.experiment.beta == beta
    np.testing.assert_array_equal(x, keep[0])
    np.testing.assert_array_equal(w, keep[1])


@pytest.mark.parametrize("kind,beta,weighted_run", [("is", None, False), ("beta", 1.5, False), ("kl", None, True)])
def test_the_start_objective_is_the_one_mur_recorded_last(kind, beta, weighted_run):
    from nmf_amd.mur import mur
    x, _ = run_data()
    kw = dict(distance_type=kind, beta=beta)
    if weighted_run:
        kw["weights"] = log_uniform_weights(x.shape, seed=11).astype(np.float64)
    np.random.seed(2)
    fit = mur(x.copy(), 12, min_iter=6, max_iter=6, **kw)
    got = _transform(x, fit.w, h0=fit.h, min_iter=1, max_iter=1, **kw)
    rel = abs(got.obj_history[0] - fit.obj_history[-1]) / abs(fit.obj_history[-1])
    print(f"tie to mur ({kind}, beta={beta}, weighted={weighted_run}): mur's last {fit.obj_history[-1]!r}, fold-in's first "
          f"{got.obj_history[0]!r}: rel {rel:.2e}")
    assert rel <= OBJ_RTOL


# chosen on the CPU (float64 run of transform_ref): with these the run stops at i = 6 and its last two decisions sit more
# than 1000 x OBJ_RTOL x objective from the threshold
STOP = dict(min_iter=3, max_iter=400, tol1=1e-5, tol2=100.0)


def test_stop_rule_fires_where_the_float64_run_stops():
    x, w = run_data()
    np.random.seed(3)
    want = transform_ref(x, w, "is", **STOP)
    margins = stop_margins(want, STOP["tol2"])
    print(f"fold-in stop: float64 run stops at i = {want.i}, margins of its last two decisions {margins} (x OBJ_RTOL x objective)")
    assert want.trace["stop_rule"] == 2 and STOP["min_iter"] < want.i < STOP["max_iter"] - 1 and min(margins) >= 150      # the yardstick alone
    np.random.seed(3)
    got = _transform(x, w, distance_type="is", **STOP)
    err = wh_error(w, got.h, w, want.h, x)
    print(f"fold-in stop: device i = {got.i}, H at the stop vs the float64 run {err:.2e}")
    assert got.i == want.i and len(got.obj_history) == len(want.obj_history) == got.i + 2
    assert err < WH_TOL


@pytest.mark.parametrize("kind,beta,weighted_run", [("kl", None, False), ("eu", None, False), ("beta", 0.5, True)])
def test_two_runs_bit_identical(kind, beta, weighted_run):
    x, w = run_data(5)
    w = np.hstack([w, w[:, ::-1]])                                 # k = 24
    kw = dict(weights=log_uniform_weights(x.shape, seed=11).astype(np.float64)) if weighted_run else {}
    out = []
    for _ in range(2):
        np.random.seed(1)
        out.append(_transform(x, w, distance_type=kind, beta=beta, min_iter=15, max_iter=15, **kw))
    assert np.array_equal(out[0].h, out[1].h)
    assert np.array_equal(np.asarray(out[0].obj_history), np.asarray(out[1].obj_history))


def test_a_fold_in_leaves_nothing_behind_on_the_handle():
    """An 'is' MUR run on a handle that did a fold-in before equals a fresh handle's bit for bit."""
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    v, w0, h0 = make_inputs(257, 130, 20, seed=12)

    def is_run(eng):
        eng.set_factors(w0, h0)
        eng.mur_run(L.IS, 0.0, 0.01, NEVER, 0, 0, 0, 3)
        eng.mur_finish(L.IS, NEVER, 0, 0, 3)
        return eng.get_factors() + (eng.objectives(0, 4),)

    with Engine(257, 130, 20) as eng:
        eng.upload_v(v)
        drive(eng, L.KL, w0, h0, 0.1, steps=(3,))
        drive(eng, L.IS, w0, h0, 0.0, steps=(2,))
        got = is_run(eng)
    with Engine(257, 130, 20) as fresh:
        fresh.upload_v(v)
        want = is_run(fresh)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


# ---- 4. ABI ----------------------------------------------------------------------------------------------------------------
def test_refusals_at_the_abi():
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    lib = L.require_gpu()
    assert lib.nmfx_version() >= 370

    def both(h, dist):
        return (lib.nmfx_foldin_run(h, dist, 0.0, NEVER, 0.0, 0.0, 0, 1), lib.nmfx_foldin_finish(h, dist, NEVER, 0.0, 0.0, 0))

    v, w0, h0 = make_inputs(200, 160, 8, seed=9)
    with Engine(200, 160, 8) as eng:
        h = eng.h
        assert both(h, L.KL) == (L.NMFX_E_STATE,) * 2 and b"upload V" in lib.nmfx_last_error(h)      # no V, no factors
        eng.upload_v(v)
        assert both(h, L.KL) == (L.NMFX_E_STATE,) * 2 and b"factors" in lib.nmfx_last_error(h)       # no factors
        eng.set_factors(w0, h0)
        assert both(h, 7) == (L.NMFX_E_ARG,) * 2 and b"distance" in lib.nmfx_last_error(h)           # unknown distance
        assert both(h, L.BETA) == (L.NMFX_E_STATE,) * 2 and b"beta" in lib.nmfx_last_error(h)        # NMFX_BETA without a beta
        eng.set_beta(0.5)
        eng.set_ard(0.1, 5.0, 1.0)
        for dist in (L.BETA, L.KL):                                                                  # ARD set
            assert both(h, dist) == (L.NMFX_E_STATE,) * 2 and b"relevance" in lib.nmfx_last_error(h)
        st = eng.state()
        assert st[0] == 0 and st[2] == 0                           # nothing was recorded, nothing stopped
        eng.clear_ard()
        runs = drive(eng, L.BETA, w0, h0, 0.0)                     # ... and the handle folds in as a fresh one does
    with Engine(200, 160, 8) as fresh:
        fresh.upload_v(v)
        fresh.set_beta(0.5)
        want = drive(fresh, L.BETA, w0, h0, 0.0)
    for s in runs:
        for a, b in zip(runs[s], want[s]):
            assert np.array_equal(a, b)

    xs = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 4)
    with Engine.for_sparse(xs, 4) as eng:                          # a sparse handle
        rs = np.random.RandomState(0)
        eng.set_factors(np.abs(rs.randn(64, 4)), np.abs(rs.randn(4, 48)))
        assert both(eng.h, L.KL) == (L.NMFX_E_ARG,) * 2 and b"sparse" in lib.nmfx_last_error(eng.h)
        assert eng.state()[2] == 0
    v2, w2, h2 = make_inputs(200, 160, 200, seed=10)
    with Engine(200, 160, 200) as eng:                             # padded rank above 128
        eng.upload_v(v2)
        eng.set_factors(w2, h2)
        assert both(eng.h, L.EU) == (L.NMFX_E_ARG,) * 2 and b"128" in lib.nmfx_last_error(eng.h)
        assert eng.state()[2] == 0


# ---- 5. a single column, and the class -------------------------------------------------------------------------------------
def test_a_single_column_through_the_function_and_the_class():
    from nmf_amd import NMF
    x, _ = run_data()
    np.random.seed(6)
    nmf = NMF(x.copy(), 12)
    nmf.factorize(method="mur", distance_type="is", min_iter=5, max_iter=5)
    col = x[:, 17:18]
    np.random.seed(8)
    got = nmf.transform(col, min_iter=20, max_iter=20)             # 'is', as the factorize before it
    np.random.seed(8)
    same = _transform(col, nmf.w, distance_type="is", min_iter=20, max_iter=20)
    np.random.seed(8)
    want = transform_ref(col, nmf.w, "is", min_iter=20, max_iter=20)
    assert got.experiment.distance_type == "is" and got.h.shape == (12, 1)
    assert np.array_equal(got.h, same.h) and got.obj_history == same.obj_history
    err = wh_error(nmf.w, got.h, nmf.w, want.h, col)
    rel = np.max(np.abs(np.asarray(got.obj_history) - want.obj_history) / np.abs(want.obj_history))
    print(f"single column: wh_error {err:.2e}, history rel {rel:.2e}")
    assert err < WH_TOL and got.i == want.i == 19
    np.random.seed(8)
    other = nmf.transform(col, distance_type="kl", min_iter=20, max_iter=20)      # another loss on request
    np.random.seed(8)
    want = transform_ref(col, nmf.w, "kl", min_iter=20, max_iter=20)
    assert other.experiment.distance_type == "kl" and wh_error(nmf.w, other.h, nmf.w, want.h, col) < WH_TOL
