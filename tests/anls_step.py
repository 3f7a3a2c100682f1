"""Problem-by-problem checks of single ANLS half-steps (tests/test_gpu_anls_step.py, tests/test_anls_step_bars.py).

One ANLS half-step solves one NNLS problem per row of W / column of H (oracle/nmf_ref.py:anls_w_step, anls_h_step).  The
device runs s = 1 and s = 2 iterations from the same start; every half-step is compared with the float64 problem fed the
exact f32 values the device held before it:

    W_s  against  argmin_{x >= 0} for (V, H_{s-1}, lambda_w)
    H_s  against  argmin_{x >= 0} for (V, W_s,     lambda_h)     (the device's own W_s)

Everything below is written for problems stored as COLUMNS: a half-step is (F, B, lambda) with one problem
min ||F x - B[:, c]||^2 + lambda ||x||^2, x >= 0 per column c, i.e. G = F^T F + 2 lambda I, r = F^T B.  The H half-step is
(W, V), the W half-step is (H^T, V^T).

Check A (kkt): the KKT conditions of every problem in float64 -- complete, because G is positive definite.
Check B (values): element by element against float64 Lawson-Hanson, on every problem or on a fixed set of them.

Which NNLS kernel solves a problem depends on the number of zeros of its own solution (csrc/kernels_anls.hip: the
complement workspace MC); the input regimes below are built so that the reference alone says which kernels a launch
needs, and the fall-back counters of the run say which ones ran."""
import math
import os
from collections import namedtuple

import numpy as np
import scipy.optimize as sopt

from mur_step import NEVER, OBJ_FLOOR, OBJ_RTOL, _record, make_inputs, objective
from oracle import nmf_ref as R

KKT_BAR = 5e-5              # check A: |dual| / max|r_c| (tests/test_gpu_fullsize.py holds the k = 64 half-steps to the same bar)
STRICT = 5e-5               # a reference zero with a dual above STRICT * max|r_c| is strictly active: the device value must be 0
CHOL_FROM = 65              # from this k on the reference is nnls on the Cholesky factor of the float64 G (host_shard.py)
B_BUDGET = 3.0              # seconds of float64 reference per case; beyond it check B covers the fixed set of b_columns
LAMS = [(0.0, 0.0), (0.05, 0.0), (0.0, 0.02)]      # by k % 3


def kp_of(k):
    """k padded as the engine pads it (16, 32, 64, 128; multiples of 128 beyond)."""
    for kp in (16, 32, 64, 128):
        if k <= kp:
            return kp
    return -(-k // 128) * 128


def mc_of(k, second=False):
    """Largest complement (number of zeros) the inverse + complement pass solves: 28 for kp <= 64, 36 at kp = 128 and 56 in its
    second pass; None beyond 128 components (gx_nnls has no such workspace)."""
    if k > 128:
        return None
    return 28 if kp_of(k) <= 64 else (56 if second else 36)


def wrap_stride(k, ncu=256):
    """Problems one round of the grid-stride loops covers with `ncu` CUs: 2 ncu blocks of 6 waves (kp <= 64), ncu blocks of 2
    waves (kp = 128; its second pass: 512 blocks of one wave), 4 ncu blocks (gx_nnls)."""
    if k > 128:
        return 4 * ncu
    return 2 * ncu * 6 if kp_of(k) <= 64 else ncu * 2


def ref_cost(k):
    """Seconds of float64 Lawson-Hanson per problem on the host, about 1.2e-6 k^2 (measured: 0.5 ms at k = 17, 2-3 ms at 40,
    5-7 ms at 64, 12-20 ms at 128 in the Cholesky form -- most where the solution has few zeros)."""
    return 1.2e-6 * k * k


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def planted(m, n, k, seed, noise=0.02, jitter=0.05, ramp=None, strict=0.0, scale=1.0):
    """(V f32, W0, H0): V = W* H* / k + noise U(0, 1); the start is (W*, H*) / sqrt(k) with every entry moved by up to
    `jitter` (relative), so that its support is the planted one.  scale: factors times scale, V times scale^2 (the weight of
    a given lambda against the Gram matrices falls with scale^2).
    ramp = (lo, hi): row i of W* and column j of H* carry zeros with probability lo + (hi - lo) min(1, (i % 16) / 11)^2; with `strict`
    V is built from the signed factors W* - d Z (Z: the planted zeros; d = min(strict, (1 - p) / 4 p) per row: the row sums of V stay positive), so
    that the planted zeros are strictly active in the problems of a step and a problem's zero count follows its row's p."""
    rng = np.random.default_rng(seed)
    ws = rng.uniform(0.1, 1.0, (m, k))
    hs = rng.uniform(0.1, 1.0, (k, n))
    wm, hm = ws, hs
    if ramp:
        lo, hi = ramp
        pr = (lo + (hi - lo) * np.minimum(1.0, (np.arange(m) % 16) / 11.0) ** 2)[:, None]
        pc = (lo + (hi - lo) * np.minimum(1.0, (np.arange(n) * 5 % 16) / 11.0) ** 2)[None, :]
        zw, zh = rng.random(ws.shape) < pr, rng.random(hs.shape) < pc
        ws[zw] = 0
        hs[zh] = 0
        wm = ws - zw * np.minimum(strict, 0.25 * (1 - pr) / pr)
        hm = hs - zh * np.minimum(strict, 0.25 * (1 - pc) / pc)
    v = wm @ hm / k
    v = np.maximum(v, 1e-3 * v.mean()) + noise * v.mean() * rng.uniform(0, 1, (m, n))
    w0 = f32(scale * ws / math.sqrt(k) * (1 + jitter * rng.uniform(-1, 1, ws.shape)))
    h0 = f32(scale * hs / math.sqrt(k) * (1 + jitter * rng.uniform(-1, 1, hs.shape)))
    return (scale * scale * v).astype(np.float32), w0, h0


MIXED_AMP = 0.02            # scale of the uniform rows and columns of the mixed regime (V and start), relative to the planted
                            # part: they weigh 0.04 % in the least-squares problems of the planted rows and columns they cross


def mixed_ramp(k):
    """Planted zero fractions of the mixed regime (tuned on the host, test_anls_step_bars.test_regimes): from nearly dense to
    14 zeros more than the first workspace holds."""
    return 0.04, min(0.93, ((mc_of(k) or 36) + 14.0) / k)


def make_case(regime, m, n, k, seed=0):
    """(V f32, W0, H0 f32-valued float64) of an input regime:
    settled     planted, start next to the planted pair: few zeros per problem, the complement pass solves everything
    cold        uniform V and uniform positive factors (mur_step.make_inputs): many zeros, the elimination kernels
    mixed       planted with the zero fractions of mixed_ramp, strictly active; every third row and every third column of V
                replaced by uniform draws at MIXED_AMP of the planted scale (the start scaled alike)
    zero        cold, with every fifth column of H0 and every fifth row of W0 all zero (an empty passive set)
    dead        settled with lambda = 0 in mind: row 1 of H0 zero under a positive column of W0 (the W step meets a vanished
                pivot in its warm-start passive set), and column 3 of W0 with row 3 of H0 both zero (never passive); k >= 4"""
    seed = seed + 7 * m + 3 * n + k
    if regime in ("cold", "zero"):
        v, w0, h0 = make_inputs(m, n, k, seed)
        if regime == "zero":
            h0[:, 1::5] = 0
            w0[1::5, :] = 0
        return v, w0, h0
    if regime in ("settled", "dead"):
        v, w0, h0 = planted(m, n, k, seed, noise=0.002, jitter=0.01, scale=3.0)
        if regime == "dead":
            h0[1] = 0
            w0[:, 3] = 0
            h0[3] = 0
        return v, w0, h0
    if regime == "mixed":
        v, w0, h0 = planted(m, n, k, seed, noise=0.001, jitter=0.002, ramp=mixed_ramp(k), strict=0.1)
        rng = np.random.default_rng(seed + 1)
        hi = MIXED_AMP * 2 * float(v.mean())
        v[0::3, :] = rng.uniform(0.05 * hi, hi, v[0::3, :].shape).astype(np.float32)
        v[:, 0::3] = rng.uniform(0.05 * hi, hi, v[:, 0::3].shape).astype(np.float32)
        w0[0::3, :] = f32(w0[0::3, :] * MIXED_AMP)
        h0[:, 0::3] = f32(h0[:, 0::3] * MIXED_AMP)
        return v, w0, h0
    raise ValueError(regime)


DEAD_VARS = (1, 3)          # the components of the dead regime that stay at zero


# ---- device runners -------------------------------------------------------------------------------------------------------
Run = namedtuple("Run", "w h objectives diagnostics fallbacks")


def _arith(eng, k, precision):
    requested = precision or ("f32" if os.environ.get("NMFX_PRECISION") in ("f32", "fp32") else "bf16")
    gx = os.environ.get("NMFX_GX_ANLS_BF16", "1") != "0"
    return "bf16" if eng.precision() == "bf16" or (k > 128 and requested == "bf16" and gx) else "f32"


def _dist(kind):
    from nmf_amd import _lib as L
    return L.EU if kind == "eu" else L.KL


def run_anls(v, w0, h0, lw=0.0, lh=0.0, kind="eu", precision=None, steps=(1, 2)):
    """The calls nmf_amd.anls.anls makes, with the stop rule off, on a fresh dense handle: ({s: Run}, arithmetic).  The
    counters are read after each run (set_factors resets them)."""
    from nmf_amd.engine import Engine
    m, n = v.shape
    k = w0.shape[1]
    out = {}
    with Engine(m, n, k) as eng:
        if precision is not None:
            eng.set_precision(precision)
        arith = _arith(eng, k, precision)
        eng.upload_v(v)
        for s in steps:
            eng.set_factors(w0, h0)
            eng.anls_set_distance(_dist(kind))
            eng.anls_run(lw, lh, NEVER, 0, 0, 0, s)
            eng.aoadmm_finish(NEVER, 0, 0, s)
            w, h = eng.get_factors()
            out[s] = Run(w, h, eng.objectives(0, s + 1), eng.diagnostics(), eng.nnls_fallbacks())
    return out, arith


def run_phases(v, w0, h0, lw=0.0, lh=0.0, kind="eu", precision=None, steps=(1, 2)):
    """The same steps through the row-sharded protocol with a world of one (nmf_amd.dist.anls_sharded without its
    all-reduces).  Returns ({s: Run}, arithmetic, W_1 read after anls_phase_w alone, before H moves)."""
    from nmf_amd.engine import Engine
    m, n = v.shape
    k = w0.shape[1]
    out = {}
    with Engine(m, n, k) as eng:
        if precision is not None:
            eng.set_precision(precision)
        arith = _arith(eng, k, precision)
        if k > 128:
            arith = "f32"                               # (the phase form beyond 128 components runs the exact-f32 products)
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        eng.anls_set_distance(_dist(kind))
        eng.anls_phase_objective(0)
        eng.anls_phase_w(lw, NEVER, 0, 0, 0)
        w_mid, h_mid = eng.get_factors()
        if not np.array_equal(h_mid, f32(h0)):
            raise AssertionError("anls_phase_w moved H")
        for s in steps:
            eng.set_factors(w0, h0)
            eng.anls_set_distance(_dist(kind))
            for j in range(s):
                eng.anls_phase_objective(j)
                eng.anls_phase_w(lw, NEVER, 0, 0, j)
                eng.anls_phase_h(lh, j)
            eng.objective_partial()
            eng.mur_finish_b(NEVER, 0, 0, s)
            w, h = eng.get_factors()
            out[s] = Run(w, h, eng.objectives(0, s + 1), eng.diagnostics(), eng.nnls_fallbacks())
    return out, arith, w_mid


# ---- float64 references -----------------------------------------------------------------------------------------------------
def gram_rhs(f, b, lam, block=2048):
    """G = F^T F + 2 lambda I (k x k) and r = F^T B (k x problems) in float64, summed over row blocks of F and B."""
    k = f.shape[1]
    g = np.zeros((k, k))
    r = np.zeros((k, b.shape[1]))
    for a in range(0, f.shape[0], block):
        fb = np.asarray(f[a:a + block], dtype=np.float64)
        g += fb.T @ fb
        r += fb.T @ np.asarray(b[a:a + block], dtype=np.float64)
    return g + 2 * lam * np.eye(k), r


def ref_stacked(f, b, lam, cols=None):
    """oracle anls_h_step (scipy nnls on the stacked system [F; sqrt(2 lambda) I]) for the problems `cols` (all: None)."""
    bb = np.asarray(b if cols is None else b[:, cols], dtype=np.float64)
    return R.anls_h_step(bb, np.asarray(f, dtype=np.float64), lam)


def ref_chol(g, r, cols=None):
    """nnls on the Cholesky factor of the float64 G (tests/host_shard.py: G = L L^T, the problem (L^T, L^-1 r)), over the
    live variables: one with G_ii = 0 (a dead component at lambda = 0) stays at zero, as Lawson-Hanson leaves it."""
    rr = r if cols is None else r[:, cols]
    live = np.nonzero(np.diag(g) > 0)[0]
    chol = np.linalg.cholesky(g[np.ix_(live, live)])
    rhs = np.linalg.solve(chol, rr[live])
    out = np.zeros_like(rr)
    for c in range(rr.shape[1]):
        out[live, c] = sopt.nnls(chol.T, rhs[:, c])[0]
    return out


def reference(f, b, lam, g, r, cols=None):
    """The float64 Lawson-Hanson solutions (k x len(cols)): stacked below CHOL_FROM, the Cholesky form from there on."""
    if f.shape[1] >= CHOL_FROM:
        return ref_chol(g, r, cols)
    return ref_stacked(f, b, lam, cols)


def b_columns(nprob, k, seed=0):
    """The problems check B covers: all of them while their reference fits B_BUDGET / 4 per half-step; else the first and last
    8, 8 on each side of every multiple of the grid-stride wrap (wrap_stride: the first index a wave or block takes in its
    next round; every such index is a multiple of the 4- and 6-problem blocks too) and a seeded sample: of 128 where the
    launch wraps, of what the budget allows (at least 16) elsewhere."""
    if nprob * ref_cost(k) <= B_BUDGET / 4:
        return np.arange(nprob)
    pick = set(range(min(8, nprob))) | set(range(max(0, nprob - 8), nprob))
    for edge in range(wrap_stride(k), nprob, wrap_stride(k)):
        pick |= set(range(max(0, edge - 8), min(nprob, edge + 8)))
    size = 128 if nprob > wrap_stride(k) else max(16, int(B_BUDGET / 4 / ref_cost(k)) - 16)
    rng = np.random.default_rng(seed + nprob + k)
    pick |= set(rng.choice(nprob, size=min(size, nprob), replace=False).tolist())
    return np.array(sorted(pick))


# ---- comparators ----------------------------------------------------------------------------------------------------------
def duals(g, r, x):
    """(y = G x - r, max|r_c| per problem)."""
    return g @ x - r, np.abs(r).max(axis=0)


def kkt(label, g, r, x, bar=KKT_BAR, info="", record=True):
    """Check A.  (worst, message or None, per-problem violation).  Violation of problem c, relative to max|r_c|: |y_i| where
    x_i > 0, max(-y_i, 0) where x_i = 0; inf for a negative or non-finite x (or a non-zero x where r_c = 0)."""
    x = np.asarray(x, dtype=np.float64)
    finite = np.isfinite(x)
    xs = np.where(finite, x, 0.0)
    y, scale = duals(g, r, xs)
    s = np.where(scale > 0, scale, 1.0)
    viol = np.where(xs > 0, np.abs(y), np.maximum(-y, 0.0)) / s
    viol = np.where(finite & (xs >= 0), viol, np.inf)
    viol = np.where((scale == 0) & (xs != 0), np.inf, viol)
    per = viol.max(axis=0) if viol.size else np.zeros(0)
    worst = float(per.max()) if per.size else 0.0
    if record:
        _record(label + " kkt", worst, bar)
    if worst <= bar:
        return worst, None, per
    c = int(np.argmax(per))
    i = int(np.argmax(viol[:, c]))
    zeros = int(np.sum(xs[:, c] == 0))
    msg = (f"{label} [A, KKT]: problem {c}, variable {i}: x = {x[i, c]!r}, dual y = {y[i, c]:.4e}, max|r| = {scale[c]:.4e}: "
           f"violation {viol[i, c]:.3e} > bar {bar:.1e}; the device solution has {zeros} zeros of {x.shape[0]} there; "
           f"{int(np.sum(per > bar))} of {per.size} problems over the bar (all {per.size} checked){info}")
    return worst, msg, per


def values(label, g, r, x, xref, cols, bar, info="", record=True):
    """Check B on the problems `cols` (xref: k x len(cols)).  (worst, message or None).  |x - xref| relative to the largest
    entry of the problem's reference solution; a strictly active reference zero must be an exact zero of the device."""
    x = np.asarray(x, dtype=np.float64)[:, cols]
    nprob = r.shape[1]
    yref, scale = duals(g, r[:, cols], xref)
    top = xref.max(axis=0)
    with np.errstate(all="ignore"):
        dev = np.abs(x - xref) / np.where(top > 0, top, 1.0)
    dev = np.where((top == 0)[None, :] & (x != 0), np.inf, dev)
    strict = (xref == 0) & (yref > STRICT * scale[None, :])
    dev = np.where(strict & (x != 0), np.inf, dev)
    dev = np.where(np.isfinite(x), dev, np.inf)
    per = dev.max(axis=0) if dev.size else np.zeros(0)
    worst = float(per.max()) if per.size else 0.0
    if record:
        _record(label + " values", worst, bar)
    if worst <= bar:
        return worst, None
    j = int(np.argmax(per))
    i = int(np.argmax(dev[:, j]))
    zeros = int(np.sum(xref[:, j] == 0))
    why = " (a strictly active variable: must be exactly 0)" if strict[i, j] and x[i, j] != 0 else ""
    msg = (f"{label} [B, values]: problem {int(cols[j])}, variable {i}: dev {x[i, j]!r}, ref {xref[i, j]!r}{why}, largest entry of the "
           f"reference solution {top[j]:.4e}: deviation {dev[i, j]:.3e} > bar {bar:.1e}; the reference has {zeros} zeros of "
           f"{x.shape[0]} there (workspace {mc_of(x.shape[0])}); {int(np.sum(per > bar))} of {per.size} checked problems over the bar "
           f"({per.size} of {nprob} problems checked, {100.0 * per.size / nprob:.0f} %){info}")
    return worst, msg


def half_steps(v, w0, h0, runs, lw, lh):
    """[(label, F, B, lambda, X_dev as k x problems, X_prev as k x problems)] of runs {1: Run, 2: Run}: step 2 starts from
    the s = 1 run's pair."""
    out = []
    prev = (w0, h0)
    vt = np.ascontiguousarray(np.asarray(v).T)
    for s in sorted(runs):
        ws, hs = runs[s].w, runs[s].h
        out.append((f"W{s}", np.ascontiguousarray(prev[1].T), vt, lw, ws.T, prev[0].T))
        out.append((f"H{s}", ws, v, lh, hs, prev[1]))
        prev = (ws, hs)
    return out


def zero_counts(xref):
    return np.sum(xref == 0, axis=0)


def check_steps(v, w0, h0, runs, lw, lh, bar_x, kind="eu", tag="", cache=None, skip_vars=(), do_b=True):
    """Checks A and B of every half-step of runs {1: Run, 2: Run} and every recorded objective against the float64 objective of
    the device's iterates.  cache: {label: (F, cols, xref)} shared between runs whose half-step inputs are bit-identical (the
    second distance of a case; do_b = "cached": check B only where the cache holds the reference).  skip_vars: variables required to be exactly 0 and left out of B (the dead regime).
    Returns {label: {"kkt": worst, "values": worst, "zeros": reference zero counts, "cols": checked problems}}; raises
    AssertionError naming every failure."""
    fails, seen = [], {}
    cache = {} if cache is None else cache
    iterate = {0: (w0, h0)}
    for s in sorted(runs):
        iterate[s] = (runs[s].w, runs[s].h)
    for label, f, b, lam, x, _ in half_steps(v, w0, h0, runs, lw, lh):
        s = int(label[1:])
        run = runs[s]
        info = (f"; fall-backs of the {s}-step run (problems, half-steps) = {run.fallbacks}, (evicted, capped) = {run.diagnostics}")
        g, r = gram_rhs(f, b, lam)
        k, nprob = r.shape
        res = {}
        res["kkt"], msg, _ = kkt(tag + label, g, r, x, info=info)
        if msg:
            fails.append(msg)
        res["dev_zeros"] = np.sum(np.asarray(x) == 0, axis=0)
        for i in skip_vars:
            if np.any(x[i] != 0):
                fails.append(f"{tag}{label}: dead variable {i} is not exactly 0 in {int(np.sum(x[i] != 0))} problems{info}")
        hit = cache.get(label)
        if hit is not None and not np.array_equal(hit[0], f):
            hit = None
        if do_b is True or (do_b == "cached" and hit is not None):
            if hit is not None:
                cols, xref = hit[1], hit[2]
            else:
                cols = b_columns(nprob, k)
                xref = reference(f, b, lam, g, r, None if len(cols) == nprob else cols)
                cache[label] = (np.array(f, copy=True), cols, xref)
            res["values"], msg = values(tag + label, g, r, x, xref, cols, bar_x, info=info)
            if msg:
                fails.append(msg)
            res["zeros"], res["cols"] = zero_counts(xref), cols
        seen[label] = res
    vv = np.asarray(v, dtype=np.float64)
    scale = OBJ_FLOOR * (0.5 * float(np.sum(vv * vv)) if kind == "eu" else float(np.sum(vv)))
    for s, run in sorted(runs.items()):
        for i in range(s + 1):
            want = objective(kind, v, *iterate[i])
            got = float(run.objectives[i])
            rel = abs(got - want) / max(abs(want), scale)
            label = f"{tag}{kind} obj[{i}] of the {s}-step run"
            _record(label, rel, OBJ_RTOL)
            if not rel <= OBJ_RTOL:
                fails.append(f"{label}: recorded {got!r}, float64 of the iterate {want!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    if fails:
        raise AssertionError("\n".join(fails))
    return seen


# ---- cases and bars ---------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "regime m n k arith")


def case_id(c):
    return f"{c.regime}-{c.m}x{c.n}-k{c.k}-{c.arith}"


def lam_of(c):
    """(lambda_w, lambda_h): LAMS by k % 3; 0 in the dead regime.  Where k > min(m, n) a Gram matrix F^T F is singular and
    the minimiser of a lambda = 0 half-step is not unique (the float64 reference is ill-posed): both lambdas positive."""
    if c.regime == "dead":
        return (0.0, 0.0)
    rows = min(c.m, c.n) if c.regime != "mixed" else 2 * min(c.m, c.n) // 3      # (mixed: a third of them carry almost no weight)
    return (0.05, 0.02) if c.k > rows else LAMS[c.k % 3]


def _cases():
    out = []
    for k in (1, 2, 15, 16, 17, 28, 29, 32):                                   # ranks, kp 16 / 32: exact f32 only
        out += [Case(rg, 257, 200, k, "f32") for rg in ("cold", "zero")]
    for k in (33, 40, 63, 64, 65, 100, 127, 128):                              # ranks, kp 64 / 128
        out += [Case("mixed", 257, 200, k, a) for a in ("f32", "bf16")]
    for k in (129, 160, 257):                                                  # gx_nnls
        out += [Case("mixed", 130, 120, k, a) for a in ("bf16", "f32")]
    for k in (40, 64, 100, 128):                                               # regimes
        out += [Case(rg, 257, 200, k, "bf16") for rg in ("settled", "cold", "dead")]
    out += [Case("mixed", m, n, 4, "f32") for m, n in ((1, 257), (257, 1), (5, 4))]          # shapes
    for k in (33, 100):
        out += [Case("mixed", m, n, k, "bf16") for m, n in ((63, 129), (130, 64), (129, 257), (61, 127))]
    out += [Case("mixed", 3100, 70, 33, "bf16"), Case("mixed", 70, 3100, 33, "bf16"),        # grid-stride wraps
            Case("mixed", 600, 70, 128, "bf16"), Case("mixed", 70, 600, 128, "bf16"), Case("mixed", 1100, 140, 130, "bf16")]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()

# check B's bar per case: 10 x the largest deviation of the host emulation of the device arithmetic from the float64 reference
# on the case's own inputs (tests/test_anls_step_bars.py computes and verifies `floor`; it depends on the conditioning of G).
# The floor of the table is the emulated deviation with a quarter added for the BLAS's summation order, rounded up to two digits.
# The one device value above a third of its bar, 1.05e-5 at 5 x 4, is the kernels' feasibility slack (NMFX_NNLS_TOL: a passive
# variable within 1e-6 of the largest is not exchanged, then clamped): host_bpp(tol=1e-6) gives the same 1.053e-5 on that problem.
# case id: (emulated floor, bar_x = 10 x floor, largest deviation measured on an MI355X with NMFX_RECORD_BARS)
BARS = {
    "cold-257x200-k1-f32": (4.3e-07, 4.3e-06, 9.6e-07),
    "zero-257x200-k1-f32": (4.6e-07, 4.6e-06, 6.7e-07),
    "cold-257x200-k2-f32": (3.1e-05, 3.1e-04, 5.8e-06),
    "zero-257x200-k2-f32": (2.6e-05, 2.6e-04, 4.8e-06),
    "cold-257x200-k15-f32": (3.6e-05, 3.6e-04, 2.4e-05),
    "zero-257x200-k15-f32": (2.4e-05, 2.4e-04, 2.2e-05),
    "cold-257x200-k16-f32": (3.8e-05, 3.8e-04, 2.8e-05),
    "zero-257x200-k16-f32": (2.7e-05, 2.7e-04, 3.1e-05),
    "cold-257x200-k17-f32": (3.0e-05, 3.0e-04, 2.2e-05),
    "zero-257x200-k17-f32": (3.4e-05, 3.4e-04, 2.8e-05),
    "cold-257x200-k28-f32": (3.8e-05, 3.8e-04, 3.0e-05),
    "zero-257x200-k28-f32": (3.5e-05, 3.5e-04, 2.8e-05),
    "cold-257x200-k29-f32": (4.0e-05, 4.0e-04, 3.0e-05),
    "zero-257x200-k29-f32": (3.6e-05, 3.6e-04, 3.0e-05),
    "cold-257x200-k32-f32": (3.4e-05, 3.4e-04, 2.6e-05),
    "zero-257x200-k32-f32": (3.7e-05, 3.7e-04, 3.2e-05),
    "mixed-257x200-k33-f32": (3.5e-05, 3.5e-04, 2.3e-05),
    "mixed-257x200-k33-bf16": (4.1e-05, 4.1e-04, 2.7e-05),
    "mixed-257x200-k40-f32": (1.3e-04, 1.3e-03, 3.6e-05),
    "mixed-257x200-k40-bf16": (1.1e-04, 1.1e-03, 5.4e-05),
    "mixed-257x200-k63-f32": (8.4e-05, 8.4e-04, 4.2e-05),
    "mixed-257x200-k63-bf16": (7.0e-05, 7.0e-04, 5.3e-05),
    "mixed-257x200-k64-f32": (2.1e-04, 2.1e-03, 1.0e-04),
    "mixed-257x200-k64-bf16": (1.5e-04, 1.5e-03, 1.0e-04),
    "mixed-257x200-k65-f32": (7.7e-05, 7.7e-04, 6.5e-05),
    "mixed-257x200-k65-bf16": (7.2e-05, 7.2e-04, 9.9e-05),
    "mixed-257x200-k100-f32": (1.4e-03, 1.4e-02, 1.8e-04),
    "mixed-257x200-k100-bf16": (5.9e-04, 5.9e-03, 1.4e-03),
    "mixed-257x200-k127-f32": (4.3e-03, 4.3e-02, 1.5e-03),
    "mixed-257x200-k127-bf16": (1.8e-03, 1.8e-02, 1.9e-03),
    "mixed-257x200-k128-f32": (1.1e-03, 1.1e-02, 6.8e-04),
    "mixed-257x200-k128-bf16": (7.9e-04, 7.9e-03, 1.0e-03),
    "mixed-130x120-k129-bf16": (9.1e-05, 9.1e-04, 1.7e-04),
    "mixed-130x120-k129-f32": (1.4e-04, 1.4e-03, 4.2e-05),
    "mixed-130x120-k160-bf16": (9.2e-05, 9.2e-04, 2.5e-04),
    "mixed-130x120-k160-f32": (2.2e-04, 2.2e-03, 5.4e-05),
    "mixed-130x120-k257-bf16": (1.5e-04, 1.5e-03, 3.0e-04),
    "mixed-130x120-k257-f32": (2.4e-04, 2.4e-03, 8.4e-05),
    "settled-257x200-k40-bf16": (8.4e-05, 8.4e-04, 6.1e-05),
    "cold-257x200-k40-bf16": (2.7e-05, 2.7e-04, 2.9e-05),
    "dead-257x200-k40-bf16": (7.7e-05, 7.7e-04, 6.4e-05),
    "settled-257x200-k64-bf16": (2.1e-04, 2.1e-03, 1.3e-04),
    "cold-257x200-k64-bf16": (3.5e-05, 3.5e-04, 2.1e-05),
    "dead-257x200-k64-bf16": (1.7e-04, 1.7e-03, 1.1e-04),
    "settled-257x200-k100-bf16": (3.5e-04, 3.5e-03, 5.9e-04),
    "cold-257x200-k100-bf16": (3.3e-05, 3.3e-04, 3.8e-05),
    "dead-257x200-k100-bf16": (3.3e-04, 3.3e-03, 5.6e-04),
    "settled-257x200-k128-bf16": (8.1e-04, 8.1e-03, 1.1e-03),
    "cold-257x200-k128-bf16": (3.9e-05, 3.9e-04, 4.1e-05),
    "dead-257x200-k128-bf16": (6.6e-04, 6.6e-03, 9.6e-04),
    "mixed-1x257-k4-f32": (6.7e-07, 6.7e-06, 1.9e-06),
    "mixed-257x1-k4-f32": (2.3e-07, 2.3e-06, 1.0e-07),
    "mixed-5x4-k4-f32": (1.2e-06, 1.2e-05, 1.1e-05),
    "mixed-63x129-k33-bf16": (2.9e-04, 2.9e-03, 2.0e-04),
    "mixed-130x64-k33-bf16": (1.6e-04, 1.6e-03, 8.8e-05),
    "mixed-129x257-k33-bf16": (4.9e-05, 4.9e-04, 4.1e-05),
    "mixed-61x127-k33-bf16": (6.4e-04, 6.4e-03, 6.2e-04),
    "mixed-63x129-k100-bf16": (4.7e-05, 4.7e-04, 1.2e-04),
    "mixed-130x64-k100-bf16": (8.0e-05, 8.0e-04, 1.8e-04),
    "mixed-129x257-k100-bf16": (7.2e-05, 7.2e-04, 1.4e-04),
    "mixed-61x127-k100-bf16": (4.6e-05, 4.6e-04, 1.3e-04),
    "mixed-3100x70-k33-bf16": (1.4e-04, 1.4e-03, 7.4e-05),
    "mixed-70x3100-k33-bf16": (2.6e-04, 2.6e-03, 1.8e-04),
    "mixed-600x70-k128-bf16": (3.0e-04, 3.0e-03, 3.4e-04),
    "mixed-70x600-k128-bf16": (1.2e-04, 1.2e-03, 1.7e-04),
    "mixed-1100x140-k130-bf16": (4.2e-04, 4.2e-03, 2.7e-04),
}


def bar_of(c):
    return BARS[case_id(c)][1]


# ---- a fast float64 solver for the host tests -------------------------------------------------------------------------------
def host_bpp(g, r, passive=None, tol=1e-12):
    """Block principal pivoting (Kim & Park) on all problems at once in float64: the exchange rule of csrc/kernels_anls.hip,
    every problem's passive-set system solved in one batched np.linalg.solve (active rows and columns replaced by the
    identity).  It carries the host emulation from one half-step to the next and counts zeros on every problem in a fraction of
    Lawson-Hanson's time; tests/test_anls_step_bars.py pins it to the Lawson-Hanson reference on the problems check B covers.
    Variables with G_ii = 0 (dead) stay at zero."""
    k, n = r.shape
    live = np.diag(g) > 0
    p = (np.ones((k, n), bool) if passive is None else np.array(passive, dtype=bool)) & live[:, None]
    best = np.full(n, k + 1)
    spare = np.full(n, 3)
    eye = np.eye(k, dtype=bool)
    scale = np.abs(r).max(axis=0)
    x = np.zeros((k, n))
    todo = np.arange(n)
    for _ in range(8 * k + 64):
        pt = p[:, todo].T                                                # problems x k
        a = np.where(pt[:, :, None] & pt[:, None, :], g[None], 0.0) + (eye[None] & ~pt[:, :, None])
        xs = np.linalg.solve(a, np.where(pt, r[:, todo].T, 0.0)[:, :, None])[:, :, 0]
        xs = np.where(pt, xs, 0.0)
        y = np.where(pt, 0.0, xs @ g - r[:, todo].T)
        x[:, todo] = xs.T
        bad = (pt & (xs < -tol * np.abs(xs).max(axis=1, keepdims=True))) | (~pt & live[None] & (y < -tol * scale[todo, None]))
        ninf = bad.sum(axis=1)
        open_ = ninf > 0
        if not open_.any():
            break
        better = ninf < best[todo]
        full = better | (spare[todo] > 0)
        best[todo] = np.where(better, ninf, best[todo])
        spare[todo] = np.where(better, 3, np.maximum(spare[todo] - 1, 0))
        top = k - 1 - np.argmax(bad[:, ::-1], axis=1)                    # back-up rule: the largest infeasible index only
        single = np.zeros_like(bad)
        single[np.arange(len(todo)), top] = True
        flip = np.where(full[:, None], bad, bad & single)
        p[:, todo] ^= flip.T
        todo = todo[open_]
    else:
        raise RuntimeError("host_bpp: iteration cap")
    return np.maximum(x, 0.0)


# ---- one case on the device -------------------------------------------------------------------------------------------------
def final_workspace(k):
    """A problem whose solution has more zeros than this cannot have been solved by the complement kernels."""
    return mc_of(k, second=True)


def expects_both_paths(c):
    """Mixed cases whose launches hold problems for the complement kernels and for the elimination kernels (the host proves it
    from the reference alone: tests/test_anls_step_bars.py:test_regimes)."""
    return c.regime == "mixed" and 33 <= c.k <= 128 and min(c.m, c.n) >= 60


def run_case(c, kinds=("eu", "kl"), phases=False):
    """Run case c on the device for each distance, check every half-step (check B in full for the first distance, for the
    second where its half-step inputs are bit-identical) and the regime's counters.  Returns {kind: ({s: Run}, seen)} and, for
    phases, W_1 read after anls_phase_w alone under key "w_mid"."""
    v, w0, h0 = make_case(c.regime, c.m, c.n, c.k)
    lw, lh = lam_of(c)
    precision = c.arith if c.k <= 128 else None         # (beyond 128 components: NMFX_GX_ANLS_BF16, read once per process)
    cache, out, fails = {}, {}, []
    for kind in kinds:
        if phases:
            runs, arith, out["w_mid"] = run_phases(v, w0, h0, lw, lh, kind, precision)
        else:
            runs, arith = run_anls(v, w0, h0, lw, lh, kind, precision)
            if c.k > 128 or (c.arith == "bf16" and c.k > 32):
                assert arith == c.arith, f"{case_id(c)}: ran in {arith} arithmetic"
        try:
            seen = check_steps(v, w0, h0, runs, lw, lh, bar_of(c), kind=kind, cache=cache, tag=f"{case_id(c)} {kind} ",
                               skip_vars=DEAD_VARS if c.regime == "dead" else (), do_b=True if kind == kinds[0] else "cached")
        except AssertionError as e:
            fails.append(str(e))
            continue
        out[kind] = (runs, seen)
        fails += counter_failures(c, runs, seen, f"{case_id(c)} {kind}")
    if fails:
        raise AssertionError("\n".join(fails))
    return out


def counter_failures(c, runs, seen, tag):
    """What the fall-back counters of each run must show in the regime of c (kernels_anls.hip: which kernel solved what)."""
    fails = []
    for s, run in sorted(runs.items()):
        labels = [lb for lb in seen if int(lb[1:]) <= s]
        total = sum(len(seen[lb]["dev_zeros"]) for lb in labels)
        left, noinv = run.fallbacks
        evicted, capped = run.diagnostics
        say = f"{tag}, {s}-step run: fall-backs (problems, half-steps) = {run.fallbacks}, (evicted, capped) = {run.diagnostics}, {total} problems"
        if capped:
            fails.append(f"{say}: a solve reached the iteration cap")
        if c.k > 128:
            if (left, noinv) != (0, 0):
                fails.append(f"{say}: gx_nnls counts no fall-backs")
            continue
        if "NMFX_NNLS_CINV" in os.environ and os.environ["NMFX_NNLS_CINV"] == "0":
            if (left, noinv) != (0, 0):
                fails.append(f"{say}: the complement pass ran although NMFX_NNLS_CINV=0")
            continue
        over = sum(int(np.sum(seen[lb]["dev_zeros"] > final_workspace(c.k))) for lb in labels)
        if c.regime == "dead":
            if not (noinv == 2 * s and evicted > 0):
                fails.append(f"{say}: every half-step's inverse should have been refused, with evictions")
            continue
        if noinv:
            fails.append(f"{say}: an inverse was refused")
        if not over <= left <= total:
            fails.append(f"{say}: {over} solutions have more zeros than the complement workspace holds ({final_workspace(c.k)})")
        if c.regime == "settled" and left:
            fails.append(f"{say}: the complement pass should have solved everything")
        if c.regime == "cold" and c.k >= 64 and left < s * c.m:
            fails.append(f"{say}: every W problem ({s * c.m}) should have been left to the elimination kernels")
        if c.k <= 28 and left:
            fails.append(f"{say}: no complement of k <= 28 variables outgrows the workspace")
        if c.regime == "zero" and c.k > 28 and left < len(range(1, c.m, 5)) + len(range(1, c.n, 5)):
            fails.append(f"{say}: every empty passive set of k > 28 variables outgrows the workspace on its first exchange")
        if expects_both_paths(c):
            if not 0 < left < total:
                fails.append(f"{say}: both the complement and the elimination kernels should have solved problems")
    if expects_both_paths(c) and kp_of(c.k) == 128 and (c.m, c.n) == (257, 200) and 1 in runs and 2 in runs:
        # the second complement pass: in iteration 2, whose warm start is the settled support of iteration 1 (few exchanges, so
        # that a complement seldom outgrows the workspace on the way), fewer problems are left than end beyond the first
        # pass's 36 zeros.  (Not at the wrap shapes: a 70-row factor leaves every one of the 600 problems 58 zeros or more.)
        z2 = np.concatenate([seen[lb]["dev_zeros"] for lb in ("W2", "H2")])
        left2 = runs[2].fallbacks[0] - runs[1].fallbacks[0]
        if np.any((z2 > 36) & (z2 <= 52)) and not left2 < int(np.sum(z2 > 36)):
            fails.append(f"{tag}: iteration 2 left {left2} problems to the elimination kernel, {int(np.sum(z2 > 36))} solutions have more "
                         f"than 36 zeros, {int(np.sum((z2 > 36) & (z2 <= 52)))} of them at most 52: the second pass should have solved some")
    return fails
