"""Problem-by-problem checks of single masked HALS half-steps (tests/test_gpu_hals_masked_step.py,
tests/test_masked_hals_step_bars.py).

A half-step of nmf_amd.hals.hals_masked (csrc/kernels_sparse.hip, sp_mhals_phase_kernel) is, per row of W / column of H,
`sweeps` projected Gauss-Seidel sweeps on the row's OWN system over its observed set Omega,

    G = Sum_{e in Omega} f_e f_e^T + 2 lambda I        r = Sum_{e in Omega} v_e f_e

(f_e: the row of the other factor at entry e; an observed zero adds to G and not to r).  The device runs s = 1 and s = 2
iterations from the same start with the stop rule off; every half-step is compared with a batched float64 sweep, one G per
problem, on systems formed in float64 from the exact f32 values the device held before it, and every recorded objective with
nmf_amd.masked.objective of the device's iterates.  Comparator, STRICT rule and messages are those of tests/hals_step.py.

Matrices (float32-valued; x is dense with NaN outside the mask, about 10 % of the observed values are exact zeros):
    base    the 700 x 600 pattern of tests/sparse_hals_step.py as the mask: long row 3, long column 11, empty rows 0, 350 and
            columns 1, 599.  At k >= 16 most rows have fewer observed entries than k: their Grams are rank-deficient
    rows    40 x 600 with rows of exactly 1, 3, 4, 5, 255, 256, 257 and 513 observed entries: the four-entry tail of the MFMA
            step and the piece boundary
    1x300, 300x1, 5x4      the edge shapes
    tall    20000 x 40 at 5 %: more rows than one round of the phase grid
    full    64 x 48 with an all-ones mask: hals_step's shared-Gram reference applies too
Regimes and lambdas: those of tests/sparse_hals_step.py (scaled by the masked least-squares alpha, cold, settled, dead;
lambda by k % 3).

A problem whose right-hand side is exactly zero (no observed entry, or only observed zeros) has an exact answer that no
arithmetic reaches: every variable with G_jj > 0 ends at 0, every other keeps its value (tests/sparse_hals_step.py).
`values` measures such a problem against that answer on the scale of the largest entry of its start."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import anls_step as A
import hals_step as HS
import sparse_hals_step as SH
from mur_step import NEVER, _record

OBJ_RTOL = 1e-9             # recorded objective vs nmf_amd.masked.objective of the iterate
CHUNK = SH.CHUNK
DEAD = SH.DEAD
ROW_COUNTS = (1, 3, 4, 5, 255, 256, 257, 513)
ZERO_SHARE = 0.1            # of the observed values


# ---- matrices -----------------------------------------------------------------------------------------------------------------
def _pattern(name):
    if name == "rows":
        rng = np.random.RandomState(3)
        x = sp.random(40, 600, density=0.02, format="lil", random_state=rng, data_rvs=lambda s: rng.uniform(0.1, 1.0, s))
        for r, cnt in enumerate(ROW_COUNTS):
            x[r, :] = 0
            x[r, np.sort(rng.choice(600, cnt, replace=False))] = rng.uniform(0.1, 1.0, cnt)
        return sp.csr_matrix(x.tocsr(), dtype=np.float32)
    if name == "full":
        return sp.csr_matrix(np.random.RandomState(48).uniform(0.1, 1.0, (64, 48)).astype(np.float32))
    return SH.matrix(name)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """(x, mask): x float32 m x n with NaN outside the mask, mask bool.  Neither is ever written to."""
    p = sp.csr_matrix(_pattern(name), copy=True)
    p.eliminate_zeros()
    p.sort_indices()
    data = p.data.copy()
    rng = np.random.RandomState(1000 + p.shape[0] + p.shape[1])
    data[rng.rand(data.size) < ZERO_SHARE] = 0.0
    rows = np.repeat(np.arange(p.shape[0]), np.diff(p.indptr))
    x = np.full(p.shape, np.nan, dtype=np.float32)
    x[rows, p.indices] = data
    mask = np.zeros(p.shape, dtype=bool)
    mask[rows, p.indices] = True
    x.setflags(write=False)
    mask.setflags(write=False)
    return x, mask


Obs = namedtuple("Obs", "indptr indices data")        # the observed entries of one orientation, problem by problem (zeros kept)


@functools.lru_cache(maxsize=None)
def observed(name):
    """(by rows, by columns): the W half-step's problems gather rows of H^T, the H half-step's rows of W."""
    x, mask = matrix(name)
    out = []
    for xx, mm in ((x, mask), (x.T, mask.T)):
        r, c = np.nonzero(mm)
        indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=mm.shape[0]))])
        out.append(Obs(indptr, c, xx[r, c].astype(np.float64)))
    return tuple(out)


Case = SH.Case
case_id = SH.case_id
lam_of = SH.lam_of


def _cases():
    out = [Case("base", k, "scaled", 1) for k in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)]       # every KP, both sides of each
    out += [Case("rows", k, "scaled", 1) for k in (8, 40)]
    out += [Case(name, 4, "scaled", 1) for name in ("1x300", "300x1", "5x4")]
    out += [Case("tall", 8, "scaled", 1)]
    out += [Case("full", 8, "scaled", 1)]
    out += [Case("base", 40, rg, 1) for rg in ("cold", "settled", "dead")]
    out += [Case("base", k, "scaled", 3) for k in (40, 64)]
    return out


CASES = _cases()


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def systems(f, obs, lam, dtype=np.float64, shared=False, drop_zeros=False):
    """(G problems x k x k, r k x problems) of one half-step in `dtype` (float32: summed per row in f32, 2 lambda added in f32, as
    the bars' emulation wants it).  The keyword faults are for tests/test_masked_hals_step_bars.py: one shared Gram F^T F for
    every problem; the observed zeros left out of G."""
    f = np.asarray(f, dtype=dtype)
    k = f.shape[1]
    nprob = len(obs.indptr) - 1
    g = np.zeros((nprob, k, k), dtype=dtype)
    r = np.zeros((k, nprob), dtype=dtype)
    for p in range(nprob):
        lo, hi = obs.indptr[p], obs.indptr[p + 1]
        if lo == hi:
            continue
        fp, v = f[obs.indices[lo:hi]], obs.data[lo:hi].astype(dtype)
        r[:, p] = (fp * v[:, None]).sum(axis=0, dtype=dtype)
        if drop_zeros:
            fp = fp[v != 0]
        g[p] = fp.T @ fp
    if shared:
        g[:] = f.T @ f
    g[:, np.arange(k), np.arange(k)] += dtype(2 * lam)
    return g, r


def sweep(g, r, x, sweeps=1):
    """hals_step.sweep with one G per problem (g: problems x k x k; r and x: k x problems), in float64: (x_new, numer)."""
    g = np.asarray(g, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    x = np.array(x, dtype=np.float64)
    numer = np.zeros_like(x)
    k = g.shape[1]
    for _ in range(sweeps):
        for j in range(k):
            gjj = g[:, j, j]
            live = gjj > 0
            safe = np.where(live, gjj, 1.0)
            u = x[j] + (r[j] - np.einsum("pl,lp->p", g[:, j, :], x)) / safe
            numer[j] = np.where(live, u * gjj, numer[j])
            x[j] = np.where(live, np.maximum(u, 0), x[j])
    return x, numer


def objective(name, w, h):
    from nmf_amd import masked
    x, mask = matrix(name)
    return masked.objective(x, w, h, mask)


def host_hals(name, w, h, lw, lh, sweeps, iters):
    """The float64 loop of the definition: (W, H, objective history of iters + 1 entries)."""
    by_rows, by_cols = observed(name)
    hist = [objective(name, w, h)]
    for _ in range(iters):
        w = sweep(*systems(np.ascontiguousarray(h.T), by_rows, lw), w.T, sweeps)[0].T
        h = sweep(*systems(w, by_cols, lh), h, sweeps)[0]
        hist.append(objective(name, w, h))
    return w, h, np.array(hist)


def alpha_of(name, w0, h0):
    """<v, q>_Omega / Sum_Omega q^2, q = w0 h0, in float64."""
    by_rows, _ = observed(name)
    rows = np.repeat(np.arange(len(by_rows.indptr) - 1), np.diff(by_rows.indptr))
    q = np.einsum("ij,ji->i", np.asarray(w0, np.float64)[rows], np.asarray(h0, np.float64)[:, by_rows.indices])
    return float(by_rows.data @ q) / float(q @ q)


def start(c):
    """(W0, H0) float64 holding f32 values."""
    m, n = matrix(c.matrix)[0].shape
    rng = np.random.RandomState(100 + c.k)
    w0, h0 = A.f32(rng.uniform(0.1, 1.0, (m, c.k))), A.f32(rng.uniform(0.1, 1.0, (c.k, n)))
    if c.regime == "dead":
        w0[:, DEAD] = 0
        h0[DEAD] = 0
    if c.regime != "cold":
        alpha = alpha_of(c.matrix, w0, h0)
        w0, h0 = A.f32(w0 * np.sqrt(alpha)), A.f32(h0 * np.sqrt(alpha))
    if c.regime == "settled":
        w, h, _ = host_hals(c.matrix, w0, h0, *lam_of(c), c.sweeps, 5)
        w0, h0 = A.f32(w), A.f32(h)
    return w0, h0


def half_steps(name, w0, h0, runs, lw, lh):
    """[(label, F, observed entries problem by problem, lambda, X_dev k x problems, X_prev k x problems)]"""
    by_rows, by_cols = observed(name)
    out = []
    prev = (w0, h0)
    for s in sorted(runs):
        ws, hs = runs[s].w, runs[s].h
        out.append((f"W{s}", np.ascontiguousarray(prev[1].T), by_rows, lw, ws.T, prev[0].T))
        out.append((f"H{s}", ws, by_cols, lh, hs, prev[1]))
        prev = (ws, hs)
    return out


# ---- device runner ------------------------------------------------------------------------------------------------------------
def run_hals_masked(name, w0, h0, lw=0.0, lh=0.0, sweeps=1, steps=(1, 2)):
    """The calls nmf_amd.hals.hals_masked makes, with the stop rule off, on a fresh masked handle: {s: Run}."""
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    x, mask = matrix(name)
    k = w0.shape[1]
    out = {}
    with Engine.for_sparse(masked.observed(x, mask, k), k, masked=True) as eng:
        for s in steps:
            eng.set_factors(w0, h0)
            eng.hals_masked_run(lw, lh, sweeps, NEVER, 0, 0, 0, s)
            eng.hals_masked_finish(NEVER, 0, 0, s)
            w, h = eng.get_factors()
            assert eng.state()[2] == s + 1
            out[s] = HS.Run(w, h, eng.objectives(0, s + 1))
    return out


# ---- comparator ---------------------------------------------------------------------------------------------------------------
def values(label, g, r, x, xref, numer, prev, bar, record=True):
    """hals_step.values, with the problems whose right-hand side is exactly zero measured against their exact answer on the
    scale of their start (the module docstring): (worst, message or None, per-problem deviation)."""
    empty = np.abs(r).max(axis=0) == 0
    if empty.any():
        x, xref, numer = np.array(x, dtype=np.float64), np.array(xref), np.array(numer)
        diag = np.einsum("pjj->jp", g)[:, empty]
        top = np.abs(prev[:, empty]).max(axis=0)
        xref[:, empty] = np.where(diag > 0, 0.0, prev[:, empty])
        x[:, empty] = xref[:, empty] + (x[:, empty] - xref[:, empty]) / np.where(top > 0, top, 1.0)
        numer[:, empty] = 0
    return HS.values(label, r, x, xref, numer, bar, record=record)


def check_steps(name, w0, h0, runs, lw, lh, sweeps, bar, tag=""):
    """Every half-step of runs {1: Run, 2: Run} against the batched float64 sweep (every problem checked, a failure names the
    problem and the variable) and every recorded objective against nmf_amd.masked.objective of the device's iterates at
    OBJ_RTOL (a sum of squares per observed entry: no cancellation, so relative to itself).  Returns {label: worst}; raises
    AssertionError naming every failure."""
    fails, seen = [], {}
    iterate = {0: (w0, h0)}
    for s in sorted(runs):
        iterate[s] = (runs[s].w, runs[s].h)
    k = w0.shape[1]
    for label, f, obs, lam, xdev, prev in half_steps(name, w0, h0, runs, lw, lh):
        g, r = systems(f, obs, lam)
        xref, numer = sweep(g, r, prev, sweeps)
        seen[label], msg, _ = values(f"{tag}{label}", g, r, xdev, xref, numer, prev, bar)
        if msg:
            fails.append(msg)
        assert xdev.shape[0] == k
    for s, run in sorted(runs.items()):
        for i in range(s + 1):
            want = objective(name, *iterate[i])
            got = float(run.objectives[i])
            rel = abs(got - want) / abs(want) if want != 0 else abs(got)
            label = f"{tag}obj[{i}] of the {s}-step run"
            _record(label, rel, OBJ_RTOL)
            print(f"{label}: rel {rel:.3e}")
            if not rel <= OBJ_RTOL:
                fails.append(f"{label}: recorded {got!r}, float64 of the iterate {want!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    for label, worst in seen.items():
        print(f"{tag}{label}: worst deviation {worst:.3e} (bar {bar:.1e})")
    if fails:
        raise AssertionError("\n".join(fails))
    return seen


# The bar per case: 10 x the largest deviation of the host emulation of the device arithmetic from the float64 reference over
# the emulated two-iteration trajectory (tests/test_masked_hals_step_bars.py: every row's G and r summed in f32, 2 lambda added
# in f32, the sweep in float32 on a kept residual); the factor 10 is for the MFMA summation order and the fused multiply-adds,
# which the emulation does not reproduce: the rule and the margin of hals_step.BARS.  The floor of the table is the emulated
# deviation with a quarter added for the BLAS's summation order, rounded up to two digits.
# case id: (emulated floor, bar = 10 x floor, largest deviation measured on an MI355X with NMFX_RECORD_BARS)
BARS = {
    "base-k1-scaled": (3.4e-07, 3.4e-06, 3.0e-07),
    "base-k3-scaled": (1.9e-06, 1.9e-05, 5.9e-07),
    "base-k4-scaled": (2.4e-06, 2.4e-05, 6.9e-07),
    "base-k5-scaled": (2.6e-06, 2.6e-05, 7.7e-07),
    "base-k8-scaled": (2.4e-06, 2.4e-05, 1.4e-06),
    "base-k9-scaled": (3.5e-06, 3.5e-05, 1.3e-06),
    "base-k16-scaled": (1.3e-05, 1.3e-04, 2.1e-06),
    "base-k17-scaled": (9.1e-06, 9.1e-05, 2.2e-06),
    "base-k32-scaled": (1.4e-05, 1.4e-04, 4.0e-06),
    "base-k33-scaled": (2.4e-05, 2.4e-04, 9.4e-06),
    "base-k64-scaled": (1.7e-05, 1.7e-04, 1.3e-05),
    "rows-k8-scaled": (4.6e-06, 4.6e-05, 1.3e-06),
    "rows-k40-scaled": (9.5e-04, 9.5e-03, 1.7e-03),
    "1x300-k4-scaled": (1.4e-06, 1.4e-05, 8.2e-07),
    "300x1-k4-scaled": (4.1e-06, 4.1e-05, 2.1e-06),
    "5x4-k4-scaled": (6.4e-07, 6.4e-06, 4.6e-07),
    "tall-k8-scaled": (7.1e-04, 7.1e-03, 3.2e-04),
    "full-k8-scaled": (2.7e-06, 2.7e-05, 1.2e-06),
    "base-k40-cold": (1.3e-04, 1.3e-03, 4.9e-05),
    "base-k40-settled": (4.3e-06, 4.3e-05, 2.3e-06),
    "base-k40-dead": (9.5e-06, 9.5e-05, 6.9e-06),
    "base-k40-scaled-s3": (5.5e-05, 5.5e-04, 3.0e-05),
    "base-k64-scaled-s3": (5.9e-05, 5.9e-04, 1.3e-04),
}


def bar_of(c):
    return BARS[case_id(c)][1]


def run_case(c):
    w0, h0 = start(c)
    lw, lh = lam_of(c)
    runs = run_hals_masked(c.matrix, w0, h0, lw, lh, c.sweeps)
    check_steps(c.matrix, w0, h0, runs, lw, lh, c.sweeps, bar_of(c), tag=f"{case_id(c)} ")
    return runs
