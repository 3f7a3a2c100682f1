"""Problem-by-problem checks of single HALS half-steps (tests/test_gpu_hals_step.py, tests/test_hals_step_bars.py).

One HALS half-step makes `sweeps` projected Gauss-Seidel sweeps per row of W / column of H (nmf_amd/hals.py,
csrc/kernels_hals.hip) on the Gram matrix and right-hand sides of the ANLS half-step (tests/anls_step.py: a half-step is
(F, B, lambda), one problem per column of B, G = F^T F + 2 lambda I, r = F^T B):

    repeat `sweeps` times:  for j = 0 .. k-1:  if G[j, j] > 0:  x[j] = max(0, x[j] + (r[j] - G[j, :] @ x) / G[j, j])

The device runs s = 1 and s = 2 iterations from the same start; every half-step is compared with this sweep in float64 fed
the exact f32 values the device held before it (W_s from (V, H_{s-1}, W_{s-1}), H_s from (V, W_s, H_{s-1}), the device's
own W_s).  The reference is O(k^2) per problem and runs on all problems at once: every problem of every half-step is checked.

Inputs, regimes, lambdas and the padding rule are those of tests/anls_step.py."""
from collections import namedtuple

import numpy as np

import anls_step as A
from mur_step import NEVER, OBJ_FLOOR, OBJ_RTOL, _record, objective

STRICT = A.STRICT            # a reference zero clamped by more than STRICT * max|r_c| must be an exact zero of the device
WAVES = 8                    # problems per workgroup of hals_sweep_kernel (NMFX_HALS_WAVES)
BLOCKS_PER_CU = 2            # NMFX_HALS_BLOCKS_PER_CU


def wrap_stride(ncu=256):
    """Problems one round of the grid covers with `ncu` CUs: beyond it the blocks of hals_sweep_kernel loop."""
    return ncu * BLOCKS_PER_CU * WAVES


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def sweep(g, r, x, sweeps=1, dtype=np.float64, order=None, jacobi=False, clamp_off=None):
    """(x_new, numer) of `sweeps` sweeps on all problems at once (g: k x k, r and x: k x problems).  numer[j] is the unclamped
    value of variable j at its last update in the units of r, G_jj (x_j + step_j): where the clamp acts, x_j = 0 and -numer[j]
    is the dual (G x - r)_j at that moment.  The keyword faults are for tests/test_hals_step_bars.py: another order, all
    coordinates from the old x, no clamp on variable clamp_off."""
    g = np.asarray(g, dtype=dtype)
    r = np.asarray(r, dtype=dtype)
    x = np.array(x, dtype=dtype)
    numer = np.zeros_like(x)
    k = g.shape[0]
    for _ in range(sweeps):
        old = x.copy() if jacobi else x
        for j in (range(k) if order is None else order):
            if not g[j, j] > 0:
                continue
            u = x[j] + (r[j] - g[j] @ old) / g[j, j]
            numer[j] = u * g[j, j]
            x[j] = u if j == clamp_off else np.maximum(u, 0)
    return x, numer


# ---- device runner ------------------------------------------------------------------------------------------------------------
Run = namedtuple("Run", "w h objectives")


def run_hals(v, w0, h0, lw=0.0, lh=0.0, sweeps=1, kind="eu", precision=None, steps=(1, 2)):
    """The calls nmf_amd.hals.hals makes, with the stop rule off, on a fresh dense handle: ({s: Run}, arithmetic)."""
    from nmf_amd.engine import Engine
    m, n = v.shape
    k = w0.shape[1]
    out = {}
    with Engine(m, n, k) as eng:
        if precision is not None:
            eng.set_precision(precision)
        arith = A._arith(eng, k, precision)
        eng.upload_v(v)
        for s in steps:
            eng.set_factors(w0, h0)
            eng.anls_set_distance(A._dist(kind))
            eng.hals_run(lw, lh, sweeps, NEVER, 0, 0, 0, s)
            eng.aoadmm_finish(NEVER, 0, 0, s)
            w, h = eng.get_factors()
            out[s] = Run(w, h, eng.objectives(0, s + 1))
    return out, arith


# ---- comparator ---------------------------------------------------------------------------------------------------------------
def values(label, r, x, xref, numer, bar, record=True):
    """(worst, message or None, per-problem deviation).  |x - xref| relative to the largest entry of the problem's reference
    solution (1 where that solution is all zero); inf for a negative or non-finite device value, and for a non-zero device
    value where the reference clamped by more than STRICT * max|r_c|.  The message names the half-step (in `label`, behind the
    case), the problem and the variable."""
    x = np.asarray(x, dtype=np.float64)
    scale = np.abs(r).max(axis=0)
    top = xref.max(axis=0)
    with np.errstate(all="ignore"):
        dev = np.abs(x - xref) / np.where(top > 0, top, 1.0)
    strict = (xref == 0) & (numer < -STRICT * scale[None, :])
    dev = np.where(strict & (x != 0), np.inf, dev)
    dev = np.where(np.isfinite(x) & (x >= 0), dev, np.inf)
    per = dev.max(axis=0) if dev.size else np.zeros(0)
    worst = float(per.max()) if per.size else 0.0
    if record:
        _record(label + " values", worst, bar)
    if worst <= bar:
        return worst, None, per
    c = int(np.argmax(per))
    i = int(np.argmax(dev[:, c]))
    why = " (clamped beyond STRICT: must be exactly 0)" if strict[i, c] and x[i, c] != 0 else ""
    msg = (f"{label}: problem {c}, variable {i}: dev {x[i, c]!r}, ref {xref[i, c]!r}{why}, largest entry of the reference solution "
           f"{top[c]:.4e}: deviation {dev[i, c]:.3e} > bar {bar:.1e}; {int(np.sum(per > bar))} of {per.size} problems over the bar "
           f"(all {per.size} checked)")
    return worst, msg, per


def check_steps(v, w0, h0, runs, lw, lh, sweeps, bar, kind="eu", tag=""):
    """Every half-step of runs {1: Run, 2: Run} against the float64 sweep, and every recorded objective against the float64
    objective of the device's iterates.  Returns {label: worst}; raises AssertionError naming every failure."""
    fails, seen = [], {}
    iterate = {0: (w0, h0)}
    for s in sorted(runs):
        iterate[s] = (runs[s].w, runs[s].h)
    for label, f, b, lam, x, prev in A.half_steps(v, w0, h0, runs, lw, lh):
        g, r = A.gram_rhs(f, b, lam)
        xref, numer = sweep(g, r, prev, sweeps)
        seen[label], msg, _ = values(f"{tag}{label}", r, x, xref, numer, bar)
        if msg:
            fails.append(msg)
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


# ---- cases and bars -----------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "regime m n k arith sweeps")


def case_id(c):
    return f"{c.regime}-{c.m}x{c.n}-k{c.k}-{c.arith}" + (f"-s{c.sweeps}" if c.sweeps != 1 else "")


def lam_of(c):
    return A.lam_of(A.Case(*c[:5]))


def _cases():
    out = []
    for k in (1, 2, 15, 16, 17, 32):                                           # ranks, kp 16 / 32: exact f32 only
        out += [Case(rg, 257, 200, k, "f32", 1) for rg in ("cold", "zero")]
    for k in (33, 63, 64, 65, 100, 127, 128):                                  # ranks, kp 64 / 128
        out += [Case("mixed", 257, 200, k, a, 1) for a in ("f32", "bf16")]
    for k in (40, 128):                                                        # regimes
        out += [Case(rg, 257, 200, k, "bf16", 1) for rg in ("settled", "cold", "dead")]
    out += [Case("mixed", m, n, 4, "f32", 1) for m, n in ((1, 257), (257, 1), (5, 4))]       # shapes
    for k in (33, 100):
        out += [Case("mixed", m, n, k, "bf16", 1) for m, n in ((63, 129), (130, 64), (61, 127))]
    out += [Case("mixed", 4200, 70, 33, "bf16", 1), Case("mixed", 70, 4200, 33, "bf16", 1)]   # more problems than one round
    out += [Case("mixed", 257, 200, k, "bf16", 3) for k in (40, 128)]          # further sweeps reuse the residual
    return out


CASES = _cases()

# The bar per case: 10 x the largest deviation of the host emulation of the device arithmetic (tests/test_hals_step_bars.py: the
# products as the device forms them, the sweep in float32 on a kept residual, as the kernel runs it) from the float64 reference over the emulated two-iteration
# trajectory; the factor 10 is for the MFMA summation order, which the emulation does not reproduce.  The floor of the table is
# the emulated deviation with a quarter added for the BLAS's summation order, rounded up to two digits.
# case id: (emulated floor, bar = 10 x floor, largest deviation measured on an MI355X with NMFX_RECORD_BARS)
BARS = {
    "cold-257x200-k1-f32": (3.9e-07, 3.9e-06, 9.6e-07),
    "zero-257x200-k1-f32": (4.7e-07, 4.7e-06, 6.7e-07),
    "cold-257x200-k2-f32": (1.9e-06, 1.9e-05, 1.4e-06),
    "zero-257x200-k2-f32": (1.9e-06, 1.9e-05, 1.3e-06),
    "cold-257x200-k15-f32": (5.7e-06, 5.7e-05, 6.1e-06),
    "zero-257x200-k15-f32": (6.4e-06, 6.4e-05, 5.3e-06),
    "cold-257x200-k16-f32": (8.1e-06, 8.1e-05, 5.0e-06),
    "zero-257x200-k16-f32": (7.1e-06, 7.1e-05, 6.2e-06),
    "cold-257x200-k17-f32": (3.4e-04, 3.4e-03, 4.2e-04),
    "zero-257x200-k17-f32": (8.6e-05, 8.6e-04, 3.6e-05),
    "cold-257x200-k32-f32": (9.1e-05, 9.1e-04, 4.0e-05),
    "zero-257x200-k32-f32": (1.4e-03, 1.4e-02, 7.3e-04),
    "mixed-257x200-k33-f32": (1.7e-05, 1.7e-04, 1.0e-05),
    "mixed-257x200-k33-bf16": (4.0e-05, 4.0e-04, 4.0e-05),
    "mixed-257x200-k63-f32": (1.1e-04, 1.1e-03, 3.1e-05),
    "mixed-257x200-k63-bf16": (2.6e-04, 2.6e-03, 2.1e-04),
    "mixed-257x200-k64-f32": (3.8e-05, 3.8e-04, 1.9e-05),
    "mixed-257x200-k64-bf16": (1.1e-04, 1.1e-03, 1.1e-04),
    "mixed-257x200-k65-f32": (9.6e-05, 9.6e-04, 4.9e-05),
    "mixed-257x200-k65-bf16": (1.8e-04, 1.8e-03, 1.9e-04),
    "mixed-257x200-k100-f32": (4.0e-04, 4.0e-03, 1.5e-04),
    "mixed-257x200-k100-bf16": (3.4e-04, 3.4e-03, 4.4e-04),
    "mixed-257x200-k127-f32": (7.6e-05, 7.6e-04, 3.8e-05),
    "mixed-257x200-k127-bf16": (2.1e-04, 2.1e-03, 3.0e-04),
    "mixed-257x200-k128-f32": (9.3e-05, 9.3e-04, 6.5e-05),
    "mixed-257x200-k128-bf16": (8.2e-05, 8.2e-04, 1.5e-04),
    "settled-257x200-k40-bf16": (2.1e-05, 2.1e-04, 1.6e-05),
    "cold-257x200-k40-bf16": (3.4e-05, 3.4e-04, 6.8e-05),
    "dead-257x200-k40-bf16": (1.5e-04, 1.5e-03, 1.5e-04),
    "settled-257x200-k128-bf16": (9.4e-05, 9.4e-04, 9.2e-05),
    "cold-257x200-k128-bf16": (1.5e-04, 1.5e-03, 1.2e-04),
    "dead-257x200-k128-bf16": (6.0e-04, 6.0e-03, 7.0e-04),
    "mixed-1x257-k4-f32": (6.3e-04, 6.3e-03, 3.7e-04),
    "mixed-257x1-k4-f32": (9.9e-04, 9.9e-03, 7.9e-04),
    "mixed-5x4-k4-f32": (4.6e-07, 4.6e-06, 1.9e-07),
    "mixed-63x129-k33-bf16": (7.3e-05, 7.3e-04, 5.2e-05),
    "mixed-130x64-k33-bf16": (7.5e-05, 7.5e-04, 6.6e-05),
    "mixed-61x127-k33-bf16": (1.1e-04, 1.1e-03, 8.5e-05),
    "mixed-63x129-k100-bf16": (5.6e-05, 5.6e-04, 7.2e-05),
    "mixed-130x64-k100-bf16": (4.7e-05, 4.7e-04, 4.9e-05),
    "mixed-61x127-k100-bf16": (4.5e-05, 4.5e-04, 6.3e-05),
    "mixed-4200x70-k33-bf16": (3.2e-05, 3.2e-04, 2.3e-05),
    "mixed-70x4200-k33-bf16": (2.3e-04, 2.3e-03, 1.7e-04),
    "mixed-257x200-k40-bf16-s3": (3.9e-05, 3.9e-04, 3.4e-05),
    "mixed-257x200-k128-bf16-s3": (3.0e-04, 3.0e-03, 3.2e-04),
}


def bar_of(c):
    return BARS[case_id(c)][1]


def run_case(c, kinds=("eu", "kl")):
    """Run case c on the device for each reported objective and check every half-step.  Returns {kind: {s: Run}}."""
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = lam_of(c)
    out, fails = {}, []
    for kind in kinds:
        runs, arith = run_hals(v, w0, h0, lw, lh, c.sweeps, kind, c.arith)
        if c.arith == "bf16" and c.k > 32:
            assert arith == c.arith, f"{case_id(c)}: ran in {arith} arithmetic"
        try:
            check_steps(v, w0, h0, runs, lw, lh, c.sweeps, bar_of(c), kind=kind, tag=f"{case_id(c)} {kind} ")
        except AssertionError as e:
            fails.append(str(e))
        out[kind] = runs
    if fails:
        raise AssertionError("\n".join(fails))
    return out
