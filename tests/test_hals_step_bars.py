"""The bars and the input regimes of the problem-by-problem HALS checks (tests/hals_step.py), proven on the CPU: a numpy
emulation of the device arithmetic defines each case's bar (10 x its own deviation from the float64 reference), the faults a
norm test cannot see are rejected and named, and the float64 reference alone shows what every input regime exercises.

Emulation of one half-step (F, B, lambda, X_prev): G = F^T F and r = F^T B through test_mur_step_bars.prod (exact-f32 products,
or the four-term split-bf16 products with f32 accumulation that the ANLS products run), 2 lambda added to the f32 diagonal,
then the sweep in float32 in the kernel's own form (sweep_kept_residual).  Not reproduced: the MFMA summation order of the
products and the fused multiply-adds of the kernel; the factor 10 between floor and bar is for those."""
import functools
import json
import os

import numpy as np
import pytest

import anls_step as A
import hals_step as HS
from test_mur_step_bars import prod

F = np.float32
IDS = [HS.case_id(c) for c in HS.CASES]


def terms_of(c):
    return 4 if c.arith == "bf16" and c.k > 32 else "f32"


def sweep_kept_residual(g, r, x, sweeps):
    """The sweep in float32 in the form the kernel runs it (csrc/kernels_hals.hip): the residual res = r - G x is formed once,
    column by column, and kept; step j takes d = max(-x_j, res_j / G_jj) (as a product with the reciprocal), x_j += d and
    res -= d G[:, j].  Algebraically the sweep of hals_step.sweep; in float32 the kept residual carries the rounding of every
    update since the mat-vec, which shows where one sweep moves x by orders of magnitude (the cold regime: 7e-5 of the largest
    entry at k = 32 where forming G[j, :] @ x anew in every step gives 2e-6)."""
    g, r, x = np.asarray(g, F), np.asarray(r, F), np.array(x, F)
    k = g.shape[0]
    live = np.diag(g) > 0
    inv = np.where(live, F(1) / np.where(live, np.diag(g), F(1)), F(0)).astype(F)
    res = r.copy()
    for l in range(k):
        res = (res - g[:, l:l + 1] * x[l:l + 1]).astype(F)
    for _ in range(sweeps):
        for j in range(k):
            if live[j]:
                d = np.maximum(-x[j], res[j] * inv[j]).astype(F)
                x[j] = x[j] + d
                res = (res - g[:, j:j + 1] * d[None, :]).astype(F)
    return x


def emu_half_step(f, b, lam, prev, sweeps, terms):
    k = f.shape[1]
    ft = np.ascontiguousarray(np.asarray(f, F).T)
    g = (prod(ft, np.asarray(f, F), terms=terms) + F(2 * lam) * np.eye(k, dtype=F)).astype(F)
    r = prod(ft, np.asarray(b, F), terms=terms).astype(F)
    return sweep_kept_residual(g, r, prev, sweeps).astype(np.float64)


@functools.lru_cache(maxsize=None)
def trajectory(c):
    """The emulated two-iteration run of a case: per half-step the float64 reference fed the emulation's previous f32 iterate,
    the emulation's own result and its deviation.  [(label, dict)]"""
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = HS.lam_of(c)
    out = []
    prev = (w0, h0)
    vt = np.ascontiguousarray(v.T)
    for s in (1, 2):
        for side in "WH":
            if side == "W":
                f, b, lam, x0 = np.ascontiguousarray(prev[1].T), vt, lw, np.ascontiguousarray(prev[0].T)
            else:
                f, b, lam, x0 = prev[0], v, lh, prev[1]
            g, r = A.gram_rhs(f, b, lam)
            xref, numer = HS.sweep(g, r, x0, c.sweeps)
            first, numer1 = HS.sweep(g, r, x0, 1)
            emu = emu_half_step(f, b, lam, x0, c.sweeps, terms_of(c))
            floor, _, _ = HS.values(f"{side}{s}", r, emu, xref, np.zeros_like(numer), np.inf, record=False)
            out.append((f"{side}{s}", dict(g=g, r=r, lam=lam, prev=x0, xref=xref, numer=numer, emu=emu, floor=floor,
                                           clamped=(numer1 < 0) & (np.diag(g) > 0)[:, None])))
            prev = (emu.T, prev[1]) if side == "W" else (prev[0], emu)
    return out


# ---- bars -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", HS.CASES, ids=IDS)
def test_emulation_defines_the_bar(c):
    """The emulation's largest deviation from the float64 reference is within the floor of the table, and the bar is 10 x that
    floor (NMFX_WRITE_HALS_BARS=<file>: append the figures instead, to rebuild the table)."""
    floor = max(h["floor"] for _, h in trajectory(c))
    path = os.environ.get("NMFX_WRITE_HALS_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": HS.case_id(c), "floor": floor}) + "\n")
        return
    table_floor, bar, _ = HS.BARS[HS.case_id(c)]
    assert bar == pytest.approx(10 * table_floor, rel=1e-12)
    assert floor <= table_floor, f"{HS.case_id(c)}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
    assert floor >= table_floor / 2, f"{HS.case_id(c)}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"


# ---- regimes: the reference alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in HS.CASES if (c.m, c.n) == (257, 200) and c.k >= 33 and c.sweeps == 1],
                         ids=lambda c: HS.case_id(c))
def test_regimes(c):
    """cold: more than half of W clamped in the first sweep; settled: no clamp in any half-step; dead: G_jj = 0 on variables 1
    and 3 in the first W half-step (they keep their start) and on variable 3 in the H half-step behind it, at lambda = 0;
    mixed: clamped and free entries in every workgroup's block of problems."""
    steps = dict(trajectory(c))
    if c.regime == "cold":
        share = steps["W1"]["clamped"].mean()
        assert share > 0.5, f"{HS.case_id(c)}: {share:.0%} of W clamped in the first sweep"
    elif c.regime == "settled":
        for label, h in steps.items():
            assert not h["clamped"].any(), f"{HS.case_id(c)} {label}: {int(h['clamped'].sum())} entries clamped"
    elif c.regime == "dead":
        assert HS.lam_of(c) == (0.0, 0.0)
        w1, h1 = steps["W1"], steps["H1"]
        assert np.diag(w1["g"])[list(A.DEAD_VARS)].tolist() == [0.0, 0.0] and (np.diag(w1["g"]) > 0).sum() == c.k - 2
        for i in A.DEAD_VARS:
            assert np.array_equal(w1["xref"][i], w1["prev"][i])
        assert (w1["xref"][1] > 0).all() and (w1["xref"][3] == 0).all()
        assert np.diag(h1["g"])[3] == 0 and np.diag(h1["g"])[1] > 0 and (h1["xref"][3] == 0).all()
    elif c.regime == "mixed":
        for label, h in steps.items():
            cl = h["clamped"]
            for a in range(0, cl.shape[1] - HS.WAVES + 1, HS.WAVES):       # (full blocks: 257 leaves a last block of one problem)
                blk = cl[:, a:a + HS.WAVES]
                assert blk.any() and not blk.all(), f"{HS.case_id(c)} {label}: problems {a} .. {a + blk.shape[1] - 1}"


def test_wrap_cases_wrap():
    big = [c for c in HS.CASES if max(c.m, c.n) > HS.wrap_stride()]
    assert {(c.m > c.n) for c in big} == {True, False}


# ---- planted faults -------------------------------------------------------------------------------------------------------------
FAULT_CASE = HS.Case("mixed", 257, 200, 64, "bf16", 1)
FAULT_CASE3 = HS.Case("mixed", 257, 200, 40, "bf16", 3)
FAULTS = ["jacobi", "reverse", "no_clamp", "neighbour", "stale", "lambda", "sweeps_skipped"]


def plant(fault, h, c, sweeps):
    """Column c of the half-step's result with `fault`."""
    g, r, lam, prev = h["g"], h["r"], h["lam"], h["prev"]
    k = g.shape[0]
    one = lambda **kw: HS.sweep(kw.pop("g", g), kw.pop("r", r[:, c:c + 1]), prev[:, c:c + 1], kw.pop("sweeps", sweeps), **kw)[0][:, 0]
    if fault == "jacobi":
        return one(jacobi=True)
    if fault == "reverse":
        return one(order=range(k - 1, -1, -1))
    if fault == "no_clamp":
        hit = np.nonzero(h["numer"][:, c] < 0)[0]
        return one(clamp_off=int(hit[0])) if len(hit) else h["xref"][:, c]
    if fault == "neighbour":
        return one(r=r[:, c + 1:c + 2])
    if fault == "stale":
        return prev[:, c].copy()
    if fault == "lambda":
        return one(g=g - 2 * lam * np.eye(k))
    if fault == "sweeps_skipped":
        return one(sweeps=1)
    raise ValueError(fault)


@pytest.mark.parametrize("fault", FAULTS)
def test_fault_in_one_problem_is_rejected_and_named(fault):
    """One fault in one problem of the W half-step of iteration 2 (lambda_w > 0, start: W_1), everything else the exact float64
    result: the comparator rejects it and names the problem.  The problem is the first one the fault moves by more than the bar."""
    case = FAULT_CASE3 if fault == "sweeps_skipped" else FAULT_CASE
    h = dict(trajectory(case))["W2"]
    assert h["lam"] > 0
    bar = HS.bar_of(case)
    top = h["xref"].max(axis=0)
    for prob in range(h["r"].shape[1] - 1):
        col = plant(fault, h, prob, case.sweeps)
        moved = np.abs(col - h["xref"][:, prob]).max() / top[prob]
        if moved > bar:
            break
    else:
        pytest.fail(f"{fault}: moves no problem by more than the bar {bar:.1e}")
    assert moved > bar
    x = h["xref"].copy()
    x[:, prob] = col
    _, msg, per = HS.values("W2", h["r"], x, h["xref"], h["numer"], bar, record=False)
    assert msg and f"problem {prob}," in msg and "1 of " in msg, msg
    assert (per > bar).sum() == 1


def test_exact_reference_passes():
    for case in (FAULT_CASE, FAULT_CASE3):
        for label, h in trajectory(case):
            assert HS.values(label, h["r"], h["xref"], h["xref"], h["numer"], 0.0, record=False)[1] is None


def test_non_finite_and_negative_values_never_pass():
    h = dict(trajectory(FAULT_CASE))["H2"]
    for bad in (np.nan, np.inf, -1e-30):
        x = h["xref"].copy()
        x[2, 5] = bad
        worst, msg, _ = HS.values("H2", h["r"], x, h["xref"], h["numer"], 1e30, record=False)
        assert worst == np.inf and "problem 5, variable 2" in msg


def test_a_strictly_clamped_zero_must_be_exact():
    h = dict(trajectory(FAULT_CASE))["W2"]
    strict = (h["xref"] == 0) & (h["numer"] < -HS.STRICT * np.abs(h["r"]).max(axis=0)[None, :])
    i, c = np.argwhere(strict)[0]
    x = h["xref"].copy()
    x[i, c] = 1e-30
    worst, msg, _ = HS.values("W2", h["r"], x, h["xref"], h["numer"], 1e30, record=False)
    assert worst == np.inf and f"problem {c}, variable {i}" in msg and "must be exactly 0" in msg


def test_reference_is_the_plain_loop():
    """The vectorised sweep against the definition written out per problem and per variable."""
    rng = np.random.default_rng(5)
    k, p = 7, 3
    f = rng.uniform(0, 1, (12, k))
    f[:, 2] = 0
    g, r = A.gram_rhs(f, rng.uniform(-1, 1, (12, p)), 0.0)
    x0 = rng.uniform(0, 1, (k, p))
    want = x0.copy()
    for c in range(p):
        for _ in range(2):
            for j in range(k):
                if g[j, j] > 0:
                    want[j, c] = max(0.0, want[j, c] + (r[j, c] - sum(g[j, l] * want[l, c] for l in range(k))) / g[j, j])
    got = HS.sweep(g, r, x0, 2)[0]
    assert np.allclose(got, want, rtol=1e-12, atol=1e-14) and np.array_equal(got[2], x0[2]) and (got == 0).any()
    kept = sweep_kept_residual(g, r, x0, 2)              # the kernel's form is the same sweep
    assert np.allclose(kept, want, rtol=1e-4, atol=1e-5) and np.array_equal(kept == 0, want == 0)
