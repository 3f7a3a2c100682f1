"""Problem-by-problem checks of stacked HALS (nmf_amd.hals.hals_stack, nmfx_hals_stack_*): helper of
tests/test_hals_stack_bars.py (CPU) and tests/test_gpu_hals_stack_step.py, tests/test_gpu_hals_stack.py (GPU).

A stack holds P problems side by side in the factor columns, W = [W_0 | W_1 | ...], H = [H_0; H_1; ...] (+ a tail of components
that belong to no problem on a handle with a larger k).  One half-step is the projected Gauss-Seidel sweep of tests/hals_step.py
over ALL components on the MASKED Gram matrix: G = F^T F of the stacked factor with every entry between two different problems,
or with the tail, set to zero, and 2 lambda_p on the diagonal of problem p's block.  The float64 reference is hals_step.sweep on
that G, fed the device's own previous stacked iterate (anls_step.half_steps / gram_rhs); the result is compared per problem.

All cases share one V per shape: planted rank 9 with little noise (anls_step.planted, the "settled" settings), so that a k = 9
problem started next to the planted pair is the near-exact-fit case of the recorded objective.  The other problems start from
uniform factors scaled by their least-squares alpha."""
import math
from collections import namedtuple

import numpy as np

import anls_step as A
import hals_step as HS
from mur_step import NEVER, OBJ_FLOOR, OBJ_RTOL, _record

NONE = -1                    # component -> problem: no problem (the tail)
PLANTED_K = 9

Case = namedtuple("Case", "name m n ks k_handle lams sweeps dead")


def _lams(ks, kind):
    if kind == "zero":
        return tuple((0.0, 0.0) for _ in ks)
    if kind == "by3":                                    # anls_step.LAMS by problem index
        return tuple(A.LAMS[p % 3] for p in range(len(ks)))
    if kind == "each":                                   # a different lambda for every problem, 0 next to 0.5
        vals = (0.0, 0.5, 0.2, 0.0, 0.15, 1.0, 0.1, 0.3)
        return tuple((vals[p % 8], vals[(p + 3) % 8]) for p in range(len(ks)))
    raise ValueError(kind)


def _case(name, m, n, ks, k_handle=None, lams="by3", sweeps=1, dead=None):
    return Case(name, m, n, tuple(ks), k_handle or sum(ks), _lams(ks, lams), sweeps, dead)


CASES = [
    _case("kp16", 257, 200, (1, 2, 5, 8)),
    _case("kp32", 257, 200, (3, 14, 15)),
    _case("kp64", 257, 200, (1, 2, 5, 9, 16, 31)),
    _case("kp128", 257, 200, (7, 50, 13, 40, 18)),
    _case("lane64", 257, 200, (60, 10, 58)),             # problem 1 across the lane-64 boundary of KP = 128
    _case("tail", 257, 200, (5, 6), k_handle=16),        # components 11 .. 15 belong to no problem
    _case("one", 257, 200, (3,)),                        # a stack of one (against hals_run on the same handle)
    _case("lambdas", 257, 200, (4, 9, 6, 3), lams="each"),
    _case("dead", 257, 200, (5, 9, 6), lams="zero", dead=(2, 1)),      # component 1 of problem 2: zero in W0 and H0, G_jj = 0
    _case("sweeps3", 257, 200, (9, 20, 11), sweeps=3),
    _case("row", 1, 257, (2, 2)),
    _case("col", 257, 1, (2, 2)),
    _case("tall", 4200, 70, (20, 13)),                   # more rows than one round of the sweep kernel's grid
    _case("wide", 70, 4200, (20, 13)),
]
BY_NAME = {c.name: c for c in CASES}


def case_id(c):
    return c.name


def arith_of(c):
    return "bf16" if c.k_handle > 32 else "f32"


def offsets(ks):
    return np.concatenate([[0], np.cumsum(ks)]).astype(int)


def comp2prob(ks, k_handle):
    c2p = np.full(k_handle, NONE)
    off = offsets(ks)
    for p in range(len(ks)):
        c2p[off[p]:off[p + 1]] = p
    return c2p


def mask_gram(g, ks, lams_side, k_handle=None):
    """The masked Gram matrix of a half-step: g (k x k, no lambda) with the entries between different problems and the tail
    zeroed, 2 lambda_p on problem p's diagonal."""
    k = g.shape[0]
    c2p = comp2prob(ks, k)
    same = (c2p[:, None] == c2p[None, :]) & (c2p[:, None] != NONE)
    out = np.where(same, g, 0).astype(g.dtype)
    lam = np.array([lams_side[p] if p != NONE else 0.0 for p in c2p])
    return out + np.diag((2 * lam).astype(g.dtype))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_v(m, n):
    return A.planted(m, n, PLANTED_K, 11 + 7 * m + 3 * n, noise=0.002, jitter=0.01, scale=3.0)


def make_case(c):
    """(V f32, [(W0_p, H0_p)] f32-valued float64)."""
    v, wp, hp = make_v(c.m, c.n)
    v64 = v.astype(np.float64)
    starts = []
    for p, k in enumerate(c.ks):
        if k == PLANTED_K:
            w0, h0 = wp.copy(), hp.copy()
        else:
            rng = np.random.default_rng(1000 + 31 * p + k)
            w0, h0 = rng.uniform(0.1, 1.0, (c.m, k)), rng.uniform(0.1, 1.0, (k, c.n))
            wh = w0 @ h0
            a = math.sqrt(float(np.vdot(v64, wh) / np.vdot(wh, wh)))
            w0, h0 = A.f32(w0 * a), A.f32(h0 * a)
        if c.dead and c.dead[0] == p:
            w0[:, c.dead[1]] = 0
            h0[c.dead[1]] = 0
        starts.append((w0, h0))
    return v, starts


def stack(starts, k_handle):
    m, n = starts[0][0].shape[0], starts[0][1].shape[1]
    w, h = np.zeros((m, k_handle)), np.zeros((k_handle, n))
    o = 0
    for w0, h0 in starts:
        k = w0.shape[1]
        w[:, o:o + k], h[o:o + k] = w0, h0
        o += k
    return w, h


# ---- device runner ------------------------------------------------------------------------------------------------------------
Run = namedtuple("Run", "w h objectives parts")      # stacked factors, objectives [s + 1][P], per problem (w_p, h_p)


def run_stack(v, ks, starts, lams, sweeps=1, k_handle=None, steps=(1, 2), stopped=None, eng=None):
    """The calls nmf_amd.hals.hals_stack makes, stop rule off, on a fresh dense handle: ({s: Run}, arithmetic)."""
    from nmf_amd.engine import Engine
    m, n = v.shape
    k_handle = k_handle or sum(ks)
    w0, h0 = stack(starts, k_handle)
    lws, lhs = [l[0] for l in lams], [l[1] for l in lams]
    out = {}
    with Engine(m, n, k_handle) as eng:
        arith = eng.precision()
        eng.upload_v(v)
        for s in steps:
            eng.set_factors(w0, h0)
            eng.hals_stack_set(ks)
            eng.hals_stack_run(lws, lhs, sweeps, NEVER, 0, 0, 0, s)
            eng.hals_stack_finish(NEVER, 0, 0, s)
            w, h = eng.get_factors()
            obj = np.stack([eng.hals_stack_objectives(p, 0, s + 1) for p in range(len(ks))], axis=1)
            out[s] = Run(w, h, obj, [eng.hals_stack_get_factors(p) for p in range(len(ks))])
    return out, arith


# ---- checks -------------------------------------------------------------------------------------------------------------------
def objective_parts(v, w, h, ks):
    """[float64 objective 1/2 ||V - W_p H_p||^2 per problem] of stacked factors."""
    v = np.asarray(v, dtype=np.float64)
    off = offsets(ks)
    return [0.5 * float(np.sum((v - w[:, off[p]:off[p + 1]] @ h[off[p]:off[p + 1]]) ** 2)) for p in range(len(ks))]


def check_steps(c, v, starts, runs, bar, tag=""):
    """Every half-step of runs {1: Run, 2: Run}, every problem, against the float64 masked sweep fed the device's previous
    stacked iterate; the tail stays zero; every recorded objective against the float64 objective of the device's iterate.
    Returns ({label: worst}, worst objective deviation); raises AssertionError naming every failure."""
    fails, seen = [], {}
    w0, h0 = stack(starts, c.k_handle)
    off = offsets(c.ks)
    for label, f, b, _, x, prev in A.half_steps(v, w0, h0, runs, 0.0, 0.0):
        side = 0 if label[0] == "W" else 1
        g, r = A.gram_rhs(f, b, 0.0)
        gm = mask_gram(g, c.ks, [l[side] for l in c.lams])
        xref, numer = HS.sweep(gm, r, prev, c.sweeps)
        for p in range(len(c.ks)):
            sl = slice(off[p], off[p + 1])
            seen[f"{label} p{p}"], msg, _ = HS.values(f"{tag}{label} problem {p} (k = {c.ks[p]})", r[sl], x[sl], xref[sl], numer[sl], bar)
            if msg:
                fails.append(msg)
        if np.asarray(x)[off[-1]:].any():
            fails.append(f"{tag}{label}: the components past the last problem hold non-zeros")
    scale = OBJ_FLOOR * 0.5 * float(np.sum(np.asarray(v, dtype=np.float64) ** 2))
    iterate = {0: (w0, h0)}
    for s in sorted(runs):
        iterate[s] = (runs[s].w, runs[s].h)
    want = {i: objective_parts(v, *iterate[i], c.ks) for i in iterate}
    worst_obj = 0.0
    obar = obj_bar_of(c)
    for s, run in sorted(runs.items()):
        for i in range(s + 1):
            for p in range(len(c.ks)):
                got = float(run.objectives[i, p])
                rel = abs(got - want[i][p]) / max(abs(want[i][p]), scale)
                worst_obj = max(worst_obj, rel)
                label = f"{tag}obj_{p}[{i}] of the {s}-step run"
                _record(label, rel, obar)
                if not rel <= obar:
                    fails.append(f"{label}: recorded {got!r}, float64 of the iterate {want[i][p]!r}: rel {rel:.3e} > {obar:.1e}")
    if fails:
        raise AssertionError("\n".join(fails))
    return seen, worst_obj


def run_case(c):
    v, starts = make_case(c)
    runs, arith = run_stack(v, c.ks, starts, c.lams, c.sweeps, c.k_handle)
    assert arith == arith_of(c), f"{c.name}: ran in {arith} arithmetic"
    seen, worst_obj = check_steps(c, v, starts, runs, bar_of(c), tag=f"{c.name} ")
    print(f"{c.name}: worst half-step deviation {max(seen.values()):.2e} (bar {bar_of(c):.1e}), worst objective deviation "
          f"{worst_obj:.2e} (bar {obj_bar_of(c):.1e})")
    return v, starts, runs


# ---- bars ---------------------------------------------------------------------------------------------------------------------
# Half-steps: as hals_step.BARS -- the floor is the largest deviation of the host emulation of the device arithmetic from the
# float64 masked sweep over the emulated two-iteration trajectory (tests/test_hals_stack_bars.py), rounded up to two digits with a
# quarter added for the BLAS's summation order; the bar is 10 x the floor.  Objective: the emulation of the decomposition
#     obj_p = 1/2 ||V||^2 - <W_p, A_p> + 1/2 <W_p^T W_p, H_p H_p^T>,  A = V H^T as the device forms it (f32 / four-term split bf16),
# everything else float64, against the float64 residual objective, relative to max(obj, OBJ_FLOOR 1/2 ||V||^2); bar = 10 x floor.
# case: (half-step floor, half-step bar, objective floor, objective bar, device maxima (half-step, objective) on an MI355X)
BARS = {
    "kp16": (8.1e-06, 8.1e-05, 2.0e-06, 2.0e-05, (5.1e-06, 2.3e-06)),
    "kp32": (1.3e-05, 1.3e-04, 2.0e-06, 2.0e-05, (7.8e-06, 1.0e-06)),
    "kp64": (1.8e-05, 1.8e-04, 6.4e-05, 6.4e-04, (1.4e-05, 3.8e-05)),
    "kp128": (3.7e-05, 3.7e-04, 2.8e-05, 2.8e-04, (4.8e-05, 1.7e-05)),
    "lane64": (4.4e-05, 4.4e-04, 1.8e-05, 1.8e-04, (4.7e-05, 6.4e-06)),
    "tail": (5.5e-06, 5.5e-05, 1.3e-06, 1.3e-05, (4.2e-06, 4.7e-07)),
    "one": (3.2e-06, 3.2e-05, 1.6e-07, 1.6e-06, (1.8e-06, 8.6e-07)),
    "lambdas": (6.8e-06, 6.8e-05, 3.8e-06, 3.8e-05, (4.9e-06, 3.1e-06)),
    "dead": (6.7e-06, 6.7e-05, 2.0e-06, 2.0e-05, (5.9e-06, 1.6e-06)),
    "sweeps3": (2.6e-05, 2.6e-04, 3.3e-05, 3.3e-04, (2.0e-05, 1.3e-05)),
    "row": (3.7e-07, 3.7e-06, 3.0e-05, 3.0e-04, (4.5e-07, 4.7e-05)),
    "col": (6.5e-07, 6.5e-06, 4.1e-07, 4.1e-06, (3.7e-07, 3.5e-07)),
    "tall": (2.0e-05, 2.0e-04, 4.3e-05, 4.3e-04, (1.5e-05, 1.3e-05)),
    "wide": (1.8e-05, 1.8e-04, 4.4e-06, 4.4e-05, (1.3e-05, 2.0e-06)),
}
# The objective bars above mur_step.OBJ_RTOL, the bar of the residual objective (DESIGN.md 4.11 says why): the decomposition
# subtracts <W_p, A_p>, a term of the size of ||V||^2 that carries the f32 rounding of the product A, from 1/2 ||V||^2; near an
# exact fit the difference is measured against OBJ_FLOOR 1/2 ||V||^2, 200 times less than what the rounding is relative to.
OBJ_BAR_ABOVE_RTOL = ("kp16", "kp32", "kp64", "kp128", "lane64", "tail", "lambdas", "dead", "sweeps3", "row", "tall", "wide")


def bar_of(c):
    return BARS[c.name][1]


def obj_bar_of(c):
    return BARS[c.name][3]
