"""Problem-by-problem checks of single sparse HALS half-steps (tests/test_gpu_hals_sparse_step.py,
tests/test_hals_sparse_step_bars.py).

A half-step of nmf_amd.hals.hals_sparse (csrc/kernels_sparse.hip, sp_hals_phase_kernel) is, per row of W / column of H,
`sweeps` projected Gauss-Seidel sweeps on G = F^T F + 2 lambda I and r = F^T b with r gathered from the non-zeros of X.  The
device runs s = 1 and s = 2 iterations from the same start with the stop rule off; every half-step is compared with
hals_step.sweep in float64 on (G, r) formed in float64 from the exact f32 values the device held before it, and every
recorded objective with nmf_amd.sparse.objective of the device's iterates.  Comparator, STRICT rule and messages are those of
tests/hals_step.py (the message names the half-step, the problem and the variable).

Matrices (all float32-valued, so that the device holds the caller's values):
    base    the 700 x 600 case of tests/test_gpu_sparse.py: dense row 3 and dense column 11 run the split path (pieces and
            fix-up), rows 0, 350 and columns 1, 599 are empty (nothing to gather: r = 0, the sweep still runs)
    rows    40 x 600 with rows of exactly 1, 255, 256, 257 and 513 non-zeros: the piece boundary and the four-step tail
    1x300, 300x1, 5x4      the edge shapes (1 x 300 is one long row)
    tall    20000 x 40 at 5 %: more units than one round of the phase grid (build_side: nblk = min(4 ncu, units / 8))
Regimes: scaled (the seeded uniform start times sqrt(alpha), alpha the least-squares scale: what hals_sparse starts from by
default), cold (the same start unscaled: far above X, most of W clamps in the first sweep), settled (five float64 iterations
from the scaled start first), dead (scaled, component 2 a zero column of W0 and row of H0, lambda = 0).  lambda: hals_step's
rule, by k % 3: (0, 0), (0.05, 0), (0, 0.02).

A problem with nothing to gather (an empty row or column: r = 0 exactly) has an exact answer that no arithmetic reaches: every
live variable ends at 0 (with G >= 0 and x >= 0 each step is x_j - (G_jj x_j + Sum_l G_jl x_l) / G_jj <= 0; the last one is
x_j - G_jj x_j / G_jj, rounding noise of either sign in float64 and in float32 alike), a variable with G_jj = 0 keeps its value.
`values` measures such a problem against that exact answer on the scale of the largest entry of its start; everything else
goes through hals_step.values unchanged."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import anls_step as A
import hals_step as HS
from mur_step import NEVER, OBJ_FLOOR, _record

OBJ_RTOL = 1e-9             # recorded objective vs nmf_amd.sparse.objective of the iterate (test_recorded_objective_is_f64_grade)
CHUNK = 256                 # SP_CHUNK: non-zeros per piece of a long row
DEAD = 2                    # the dead component of the dead regime
ROW_COUNTS = (1, 255, 256, 257, 513)


# ---- matrices -----------------------------------------------------------------------------------------------------------------
def sparse_case(m, n, density, seed, dense_row=None, dense_col=None, empty_rows=(), empty_cols=()):
    """tests/test_gpu_sparse.py::sparse_case."""
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


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "base":
        x = sparse_case(700, 600, 0.02, seed=16, dense_row=3, dense_col=11, empty_rows=(0, 350), empty_cols=(1, 599))
    elif name == "rows":
        rng = np.random.RandomState(3)
        x = sp.random(40, 600, density=0.02, format="lil", random_state=rng, data_rvs=lambda s: rng.uniform(0.1, 1.0, s))
        for r, cnt in enumerate(ROW_COUNTS):
            x[r, :] = 0
            cols = np.sort(rng.choice(600, cnt, replace=False))
            x[r, cols] = rng.uniform(0.1, 1.0, cnt)
        x = x.tocsr()
    elif name == "tall":
        x = sparse_case(20000, 40, 0.05, seed=7)
    else:
        m, n = (int(t) for t in name.split("x"))
        x = sparse_case(m, n, 0.9, seed=m + n)
    x = sp.csr_matrix(x, dtype=np.float32)
    x.sum_duplicates()
    x.eliminate_zeros()
    x.sort_indices()
    return x


Case = namedtuple("Case", "matrix k regime sweeps")


def case_id(c):
    return f"{c.matrix}-k{c.k}-{c.regime}" + (f"-s{c.sweeps}" if c.sweeps != 1 else "")


def lam_of(c):
    return (0.0, 0.0) if c.regime == "dead" else A.LAMS[c.k % 3]


def _cases():
    out = [Case("base", k, "scaled", 1) for k in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128)]     # every KP, both sides of each
    out += [Case("rows", k, "scaled", 1) for k in (8, 40)]
    out += [Case(name, 4, "scaled", 1) for name in ("1x300", "300x1", "5x4")]
    out += [Case("tall", 8, "scaled", 1)]
    out += [Case("base", 40, rg, 1) for rg in ("cold", "settled", "dead")]
    out += [Case("base", k, "scaled", 3) for k in (40, 128)]
    return out


CASES = _cases()


def start(c):
    """(W0, H0) float64 holding f32 values."""
    x = matrix(c.matrix)
    m, n = x.shape
    rng = np.random.RandomState(100 + c.k)
    w0, h0 = A.f32(rng.uniform(0.1, 1.0, (m, c.k))), A.f32(rng.uniform(0.1, 1.0, (c.k, n)))
    if c.regime == "dead":
        w0[:, DEAD] = 0
        h0[DEAD] = 0
    if c.regime != "cold":
        wh2 = float(np.sum((w0.T @ w0) * (h0 @ h0.T)))
        alpha = float(np.sum(x.multiply(w0 @ h0))) / wh2
        w0, h0 = A.f32(w0 * np.sqrt(alpha)), A.f32(h0 * np.sqrt(alpha))
    if c.regime == "settled":
        w, h, _ = host_hals(x, w0, h0, *lam_of(c), c.sweeps, 5)
        w0, h0 = A.f32(w), A.f32(h)
    return w0, h0


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def gram_rhs(f, b, lam):
    """G = F^T F + 2 lambda I and r = F^T B (k x problems) in float64; b: scipy.sparse, rows of F x problems."""
    f = np.asarray(f, dtype=np.float64)
    g = f.T @ f + 2 * lam * np.eye(f.shape[1])
    r = np.asarray((sp.csr_matrix(b, dtype=np.float64).T @ f).T)
    return g, np.ascontiguousarray(r)


def objective(x, w, h):
    from nmf_amd import sparse
    return sparse.objective(sp.csr_matrix(x, dtype=np.float64), w, h, "eu")


def host_hals(x, w, h, lw, lh, sweeps, iters):
    """The float64 loop of the definition on the non-zeros: (W, H, objective history of iters + 1 entries)."""
    xt = sp.csr_matrix(x.T)
    hist = [objective(x, w, h)]
    for _ in range(iters):
        g, r = gram_rhs(np.ascontiguousarray(h.T), xt, lw)
        w = HS.sweep(g, r, w.T, sweeps)[0].T
        g, r = gram_rhs(w, x, lh)
        h = HS.sweep(g, r, h, sweeps)[0]
        hist.append(objective(x, w, h))
    return w, h, np.array(hist)


def half_steps(x, w0, h0, runs, lw, lh):
    """tests/anls_step.py::half_steps with X sparse: [(label, F, B, lambda, X_dev k x problems, X_prev k x problems)]."""
    out = []
    prev = (w0, h0)
    xt = sp.csr_matrix(x.T)
    for s in sorted(runs):
        ws, hs = runs[s].w, runs[s].h
        out.append((f"W{s}", np.ascontiguousarray(prev[1].T), xt, lw, ws.T, prev[0].T))
        out.append((f"H{s}", ws, x, lh, hs, prev[1]))
        prev = (ws, hs)
    return out


# ---- device runner ------------------------------------------------------------------------------------------------------------
def run_hals_sparse(x, w0, h0, lw=0.0, lh=0.0, sweeps=1, steps=(1, 2)):
    """The calls nmf_amd.hals.hals_sparse makes, with the stop rule off, on a fresh sparse handle: {s: Run}."""
    from nmf_amd.engine import Engine
    out = {}
    with Engine.for_sparse(x, w0.shape[1]) as eng:
        for s in steps:
            eng.set_factors(w0, h0)
            eng.hals_sparse_run(lw, lh, sweeps, NEVER, 0, 0, 0, s)
            eng.hals_sparse_finish(NEVER, 0, 0, s)
            w, h = eng.get_factors()
            assert eng.state()[2] == s + 1
            out[s] = HS.Run(w, h, eng.objectives(0, s + 1))
    return out


# ---- comparator ---------------------------------------------------------------------------------------------------------------
def values(label, g, r, x, xref, numer, prev, bar, record=True):
    """hals_step.values, with the problems that gather nothing (r = 0) measured against their exact answer on the scale of
    their start (the module docstring): (worst, message or None, per-problem deviation)."""
    empty = np.abs(r).max(axis=0) == 0
    if empty.any():
        x, xref, numer = np.array(x, dtype=np.float64), np.array(xref), np.array(numer)
        top = np.abs(prev[:, empty]).max(axis=0)
        xref[:, empty] = np.where((np.diag(g) > 0)[:, None], 0.0, prev[:, empty])
        x[:, empty] = xref[:, empty] + (x[:, empty] - xref[:, empty]) / np.where(top > 0, top, 1.0)
        numer[:, empty] = 0
    return HS.values(label, r, x, xref, numer, bar, record=record)


def check_steps(x, w0, h0, runs, lw, lh, sweeps, bar, tag=""):
    """Every half-step of runs {1: Run, 2: Run} against the float64 sweep (hals_step.values: every problem checked, a failure
    names the problem and the variable) and every recorded objective against nmf_amd.sparse.objective of the device's
    iterates at OBJ_RTOL.  Returns {label: worst}; raises AssertionError naming every failure."""
    fails, seen = [], {}
    iterate = {0: (w0, h0)}
    for s in sorted(runs):
        iterate[s] = (runs[s].w, runs[s].h)
    k = w0.shape[1]
    for label, f, b, lam, xdev, prev in half_steps(x, w0, h0, runs, lw, lh):
        g, r = gram_rhs(f, b, lam)
        xref, numer = HS.sweep(g, r, prev, sweeps)
        seen[label], msg, _ = values(f"{tag}{label}", g, r, xdev, xref, numer, prev, bar)
        if msg:
            fails.append(msg)
        assert xdev.shape[0] == k
    # (relative to the objective, or to OBJ_FLOOR of 1/2 ||X||^2 where the fit is nearly exact, as hals_step.check_steps: a
    # 1 x n matrix is fitted exactly, and 1/2 [||X||^2 - 2 cross + <Grams>] is then float64 rounding of ||X||^2 on either side)
    scale = OBJ_FLOOR * 0.5 * float(np.sum(x.data.astype(np.float64) ** 2))
    for s, run in sorted(runs.items()):
        for i in range(s + 1):
            want = objective(x, *iterate[i])
            got = float(run.objectives[i])
            rel = abs(got - want) / max(abs(want), scale)
            label = f"{tag}obj[{i}] of the {s}-step run"
            _record(label, rel, OBJ_RTOL)
            if not rel <= OBJ_RTOL:
                fails.append(f"{label}: recorded {got!r}, float64 of the iterate {want!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    if fails:
        raise AssertionError("\n".join(fails))
    return seen


# The bar per case: 10 x the largest deviation of the host emulation of the device arithmetic from the float64 reference over
# the emulated two-iteration trajectory (tests/test_hals_sparse_step_bars.py: G rounded to f32 from float64 with 2 lambda added
# in f32, r summed in f32 on the W side and rounded from float64 on the H side, the sweep in float32 on a kept residual); the
# rule and the margin of hals_step.BARS.  The floor of the table is the emulated deviation with a quarter added, rounded up to
# two digits.
# case id: (emulated floor, bar = 10 x floor, largest deviation measured on an MI355X with NMFX_RECORD_BARS)
BARS = {
    "base-k1-scaled": (4.3e-07, 4.3e-06, 2.2e-07),
    "base-k3-scaled": (1.2e-06, 1.2e-05, 5.4e-07),
    "base-k4-scaled": (1.2e-06, 1.2e-05, 8.8e-07),
    "base-k5-scaled": (1.6e-06, 1.6e-05, 1.2e-06),
    "base-k8-scaled": (1.7e-06, 1.7e-05, 1.2e-06),
    "base-k9-scaled": (1.8e-06, 1.8e-05, 1.3e-06),
    "base-k16-scaled": (3.4e-06, 3.4e-05, 1.5e-06),
    "base-k17-scaled": (2.2e-06, 2.2e-05, 1.8e-06),
    "base-k32-scaled": (4.2e-06, 4.2e-05, 3.1e-06),
    "base-k33-scaled": (4.1e-06, 4.1e-05, 2.4e-06),
    "base-k64-scaled": (5.8e-06, 5.8e-05, 3.1e-06),
    "base-k65-scaled": (8.5e-06, 8.5e-05, 8.4e-06),
    "base-k100-scaled": (5.2e-06, 5.2e-05, 3.4e-06),
    "base-k128-scaled": (2.1e-05, 2.1e-04, 1.7e-05),
    "rows-k8-scaled": (1.2e-05, 1.2e-04, 7.5e-06),
    "rows-k40-scaled": (3.0e-05, 3.0e-04, 8.1e-05),
    "1x300-k4-scaled": (1.9e-06, 1.9e-05, 1.5e-06),
    "300x1-k4-scaled": (1.2e-06, 1.2e-05, 2.9e-07),
    "5x4-k4-scaled": (6.7e-07, 6.7e-06, 4.0e-07),
    "tall-k8-scaled": (7.9e-06, 7.9e-05, 4.9e-06),
    "base-k40-cold": (1.1e-03, 1.1e-02, 8.7e-04),
    "base-k40-settled": (1.1e-06, 1.1e-05, 4.7e-07),
    "base-k40-dead": (5.5e-06, 5.5e-05, 3.8e-06),
    "base-k40-scaled-s3": (5.7e-06, 5.7e-05, 3.5e-06),
    "base-k128-scaled-s3": (2.5e-05, 2.5e-04, 2.1e-05),
}


def bar_of(c):
    return BARS[case_id(c)][1]


def run_case(c):
    x = matrix(c.matrix)
    w0, h0 = start(c)
    lw, lh = lam_of(c)
    runs = run_hals_sparse(x, w0, h0, lw, lh, c.sweeps)
    check_steps(x, w0, h0, runs, lw, lh, c.sweeps, bar_of(c), tag=f"{case_id(c)} ")
    return runs
