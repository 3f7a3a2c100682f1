"""Column-by-column checks of the dense HALS fold-in (tests/test_gpu_hals_transform_dense.py,
tests/test_hals_transform_dense_bars.py).

nmf_amd.hals.hals_transform_dense (csrc/kernels_hals.hip, hals_solve_kernel) solves, per column c of dense
x_new against a fixed W, the system all columns share the Gram matrix of,

    G = W^T W + 2 lambda I               r_c = W^T x_c

by the sweeps and under the stop rule of the sparse fold-in (tests/hals_transform_step.py): after sweep s, d_s is the largest
|delta_j| of that sweep and xmax_s the largest component after it; the column stops after the first s with d_s <= tol xmax_s,
or after max_sweeps; the kept float32 residual is formed anew before the sweeps 17, 33, ...  G and r are the products of the H
half-step of `hals`, formed once in the handle's arithmetic mode (exact f32, or split bf16 where k pads to 64 or 128).

Cases come from anls_step.make_case(regime, m, n, k) = (v, w0, h0) with x_new = v and the start h0.  W is the W after one
`hals` iteration from (w0, h0) -- its W half-step in the emulated device arithmetic of tests/test_hals_step_bars.py, so that
the CPU and the GPU tests share one float32-valued W per case -- and lambda_h is anls_step.lam_of's.  The float64 reference is
hals_transform_step.solve on G and r formed in float64 from the float32 values the device holds; the float32 emulation is
hals_transform_step.emu_solve on G and r as the device forms them (test_mur_step_bars.prod in the case's arithmetic mode).
A column is compared by its values with the comparator of tests/hals_step.py; no column is exempt."""
import functools
from collections import namedtuple

import numpy as np

import anls_step as A
import hals_step as HS
import hals_transform_step as T
from mur_step import _record

F = np.float32
OBJ_RTOL = T.OBJ_RTOL
LONG, STOP = T.LONG, T.STOP

Case = namedtuple("Case", "regime m n k arith")


def case_id(c):
    return f"{c.regime}-{c.m}x{c.n}-k{c.k}-{c.arith}"


def _cases():
    out = [Case("cold", 257, 200, k, "f32") for k in (1, 2, 15, 16, 17, 32)]                  # ranks, kp 16 and 32
    out += [Case("mixed", 257, 200, k, a) for k in (33, 64, 65, 128) for a in ("f32", "bf16")]     # ranks, kp 64 and 128
    out += [Case(rg, 257, 200, 40, "bf16") for rg in ("settled", "cold", "dead")]             # regimes
    out += [Case("mixed", m, n, 4, "f32") for m, n in ((1, 257), (257, 1), (5, 4))]           # edge shapes
    out += [Case("mixed", 61, 127, 33, "bf16")]                                                # odd shape
    out += [Case("mixed", 70, 4200, 33, "bf16")]                                               # more columns than one round of the grid
    return out


CASES = _cases()
IDS = [case_id(c) for c in CASES]


def lams_of(c):
    """(lambda_w of the iteration that gives W, lambda_h of the fold-in)."""
    return A.lam_of(A.Case(*c))


def terms_of(c):
    """The product emulation of the case's arithmetic mode (tests/test_hals_step_bars.py)."""
    return 4 if c.arith == "bf16" and c.k > 32 else "f32"


# ---- problems -----------------------------------------------------------------------------------------------------------------
Problem = namedtuple("Problem", "v w h0 lam g r")


@functools.lru_cache(maxsize=None)
def problem(c):
    """The case's fold-in: v m x n float32; w m x k and h0 k x n (float64 holding f32 values); lambda_h; the float64 system g
    (k x k) and r (k x n) of those values."""
    from test_hals_step_bars import emu_half_step
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = lams_of(c)
    w = emu_half_step(np.ascontiguousarray(h0.T), np.ascontiguousarray(v.T), lw, np.ascontiguousarray(w0.T), 1, terms_of(c))
    w = np.ascontiguousarray(w.T)
    g, r = A.gram_rhs(w, v, lh)
    return Problem(v, w, h0, lh, g, r)


def systems_f32(c, lam=None):
    """(g, r) as the device forms them, in float32: the products in the case's arithmetic mode, (float) 2 lambda added to the f32
    diagonal.  lam: another lambda (a planted fault)."""
    from test_mur_step_bars import prod
    p = problem(c)
    lam = p.lam if lam is None else lam
    wt = np.ascontiguousarray(np.asarray(p.w, F).T)
    g = (prod(wt, np.asarray(p.w, F), terms=terms_of(c)) + F(2 * lam) * np.eye(c.k, dtype=F)).astype(F)
    r = prod(wt, np.asarray(p.v, F), terms=terms_of(c)).astype(F)
    return g, r


def reference(c, run, counts=None):
    """The float64 Solved of a run ("long": 40 sweeps on every column; "stop": `counts` sweeps per column, or to the rule)."""
    p = problem(c)
    if run == "long":
        return _long_reference(c)
    return T.solve(p.g, p.r, p.h0, STOP["tol"], STOP["max_sweeps"], counts=counts)


@functools.lru_cache(maxsize=None)
def _long_reference(c):
    p = problem(c)
    return T.solve(p.g, p.r, p.h0, 0.0, LONG["max_sweeps"], counts=np.full(p.r.shape[1], LONG["max_sweeps"]))


# ---- comparators ----------------------------------------------------------------------------------------------------------------
def deviation(c, x, ref, bar, label="", record=False):
    """(worst, message or None) of a k x n result against the Solved reference through hals_step.values.  STRICT (a reference zero
    with a large dual must be an exact zero of the device) presumes that the device follows the reference closely: where the
    reference's unclamped value lies within bar x the column's largest entry of zero, the sign of the device's own is open and
    the zero is not strictly active (as in hals_transform_step.deviation)."""
    p = problem(c)
    diag = np.diag(p.g)[:, None]
    top = ref.x.max(axis=0)
    with np.errstate(all="ignore"):
        open_sign = -ref.numer <= bar * np.where(top > 0, top, 1.0)[None, :] * diag
    numer = np.where(open_sign, 0.0, ref.numer)
    worst, msg, _ = HS.values(label, p.r, x, ref.x, numer, bar, record=False)
    if record:
        _record(label + " values", worst, bar)
    return worst, msg


def stop_failures(c, counts, tol, cap, slack):
    """The stop rule of every column, checked on the float64 sweep run for the given counts: d_s <= tol xmax_s (1 + slack) at the
    last sweep or the count is the cap, and d_s >= tol xmax_s (1 - slack) at every earlier sweep.  Returns (messages, Solved)."""
    p = problem(c)
    counts = np.asarray(counts)
    fails = []
    if counts.shape != (p.r.shape[1],) or (counts < 1).any() or (counts > cap).any():
        return [f"counts outside 1 .. {cap}: {counts[(counts < 1) | (counts > cap)][:5]} ..."], None
    ref = T.solve(p.g, p.r, p.h0, tol, cap, counts=counts)
    idx = np.arange(counts.size)
    rd, rx = T.rule_history(p, ref)
    last_d, last_x = rd[counts - 1, idx], rx[counts - 1, idx]
    late = (counts < cap) & ~(last_d <= tol * last_x * (1 + slack))
    for q in np.nonzero(late)[0][:3]:
        fails.append(f"column {q}: stopped after {counts[q]} < {cap} sweeps with d = {last_d[q]:.6e} > tol xmax = {tol * last_x[q]:.6e}")
    for s in range(1, int(counts.max())):
        on = counts > s
        early = on & ~(rd[s - 1] >= tol * rx[s - 1] * (1 - slack))
        for q in np.nonzero(early)[0][:3]:
            fails.append(f"column {q}: went on to {counts[q]} sweeps although d_{s} = {rd[s - 1, q]:.6e} <= tol xmax_{s} = {tol * rx[s - 1, q]:.6e}")
    return fails, ref


def host_objective(c, h):
    """1/2 ||v - w h||^2 in float64 from the float32 values."""
    p = problem(c)
    res = np.asarray(p.v, dtype=np.float64) - p.w @ np.asarray(h, dtype=np.float64)
    return 0.5 * float(np.sum(res * res))


# ---- device runner ------------------------------------------------------------------------------------------------------------
Run = namedtuple("Run", "h sweeps objectives f64 arith")


def engine_for(c, k=None):
    """A fresh dense handle on the case's v in the case's arithmetic mode, k components (default: the case's)."""
    from nmf_amd.engine import Engine
    p = problem(c)
    eng = Engine(c.m, c.n, c.k if k is None else k)
    try:
        eng.set_precision(c.arith)
        eng.upload_v(p.v)
    except Exception:
        eng.close()
        raise
    return eng


def foldin(eng, w, h0, lam, tol, max_sweeps):
    """nmfx_hals_foldin_dense_run from (w, h0) on `eng`: Run, with Engine.objective_f64 of the start and of the result."""
    eng.set_factors(w, h0)
    f0 = eng.objective_f64()
    eng.hals_foldin_dense_run(lam, tol, max_sweeps)
    _, h = eng.get_factors()
    return Run(h, eng.hals_foldin_dense_sweeps(), eng.objectives(0, 2), (f0, eng.objective_f64()), eng.precision())


@functools.lru_cache(maxsize=None)
def run_foldin(c, tol, max_sweeps):
    p = problem(c)
    with engine_for(c) as eng:
        return foldin(eng, p.w, p.h0, p.lam, tol, max_sweeps)


# The bars per case, one for each run the device tests make: 10 x the largest deviation of emu_solve on the emulated products
# from the float64 reference (tests/test_hals_transform_dense_bars.py) in the run of 40 sweeps at tol = 0 ("long") and in the
# run at tol = 1e-3 capped at 8 ("stop": the reference run for the emulation's own counts); the rule and the margin of
# hals_step.BARS: the factor 10 is for the MFMA summation order of the products and the kernel's fused
# multiply-adds, which the emulation does not reproduce.  A floor of the table is the emulated deviation with a quarter added
# for the BLAS's summation order, rounded up to two digits.
# case id: (long floor, long bar = 10 x floor, stop floor, stop bar = 10 x floor,
#           largest long / stop deviation measured on an MI355X with NMFX_RECORD_BARS)
BARS = {
    "cold-257x200-k1-f32": (3.9e-07, 3.9e-06, 3.9e-07, 3.9e-06, 2.1e-07, 2.1e-07),
    "cold-257x200-k2-f32": (2.7e-06, 2.7e-05, 2.9e-06, 2.9e-05, 5.7e-07, 5.2e-07),
    "cold-257x200-k15-f32": (4.2e-06, 4.2e-05, 3.6e-06, 3.6e-05, 8.3e-07, 1.0e-06),
    "cold-257x200-k16-f32": (1.7e-05, 1.7e-04, 1.9e-05, 1.9e-04, 3.4e-06, 3.5e-06),
    "cold-257x200-k17-f32": (4.6e-06, 4.6e-05, 4.2e-06, 4.2e-05, 8.7e-07, 1.5e-06),
    "cold-257x200-k32-f32": (3.5e-06, 3.5e-05, 3.4e-06, 3.4e-05, 8.8e-07, 8.9e-07),
    "mixed-257x200-k33-f32": (4.0e-05, 4.0e-04, 3.1e-05, 3.1e-04, 1.3e-05, 1.4e-05),
    "mixed-257x200-k33-bf16": (5.8e-05, 5.8e-04, 5.5e-05, 5.5e-04, 4.1e-05, 4.9e-05),
    "mixed-257x200-k64-f32": (2.0e-04, 2.0e-03, 1.5e-04, 1.5e-03, 7.8e-05, 6.1e-05),
    "mixed-257x200-k64-bf16": (2.3e-04, 2.3e-03, 1.8e-04, 1.8e-03, 1.7e-04, 1.4e-04),
    "mixed-257x200-k65-f32": (9.1e-05, 9.1e-04, 6.1e-05, 6.1e-04, 4.5e-05, 3.0e-05),
    "mixed-257x200-k65-bf16": (6.4e-05, 6.4e-04, 4.9e-05, 4.9e-04, 1.0e-04, 8.3e-05),
    "mixed-257x200-k128-f32": (2.5e-04, 2.5e-03, 1.9e-04, 1.9e-03, 1.1e-04, 9.1e-05),
    "mixed-257x200-k128-bf16": (1.8e-04, 1.8e-03, 1.6e-04, 1.6e-03, 2.1e-04, 2.4e-04),
    "settled-257x200-k40-bf16": (1.1e-04, 1.1e-03, 7.4e-05, 7.4e-04, 7.7e-05, 5.5e-05),
    "cold-257x200-k40-bf16": (1.1e-04, 1.1e-03, 1.1e-04, 1.1e-03, 8.3e-05, 8.3e-05),
    "dead-257x200-k40-bf16": (1.2e-04, 1.2e-03, 6.9e-05, 6.9e-04, 8.1e-05, 5.9e-05),
    "mixed-1x257-k4-f32": (5.1e-04, 5.1e-03, 5.1e-04, 5.1e-03, 2.3e-04, 2.3e-04),
    "mixed-257x1-k4-f32": (8.5e-08, 8.5e-07, 1.1e-07, 1.1e-06, 1.2e-07, 1.2e-07),
    "mixed-5x4-k4-f32": (5.0e-07, 5.0e-06, 3.5e-07, 3.5e-06, 4.8e-07, 2.4e-07),
    "mixed-61x127-k33-bf16": (2.1e-04, 2.1e-03, 1.5e-04, 1.5e-03, 1.2e-04, 1.5e-04),
    "mixed-70x4200-k33-bf16": (2.5e-04, 2.5e-03, 2.0e-04, 2.0e-03, 1.9e-04, 1.9e-04),
}

# The slack of the stop rule: 10 x the largest relative difference between the emulation's d_s, xmax_s and the float64 ones over
# every case, sweep and column of the STOP run (tests/test_hals_transform_dense_bars.py::slack_of, the measure of
# tests/test_hals_transform_bars.py).  Measured: 3.87e-2, on mixed-1x257-k4-f32 (one row: W^T W has rank one and only 2 lambda I
# separates the components; settled-257x200-k40-bf16 4.96e-3, every other case below 3e-3); the floor is that with a quarter
# added, rounded up to two digits.
SLACK_FLOOR = 0.049
SLACK = 10 * SLACK_FLOOR


def bar_of(c, run):
    """run: "long" or "stop"."""
    return BARS[case_id(c)][{"long": 1, "stop": 3}[run]]
