"""The bars and the input regimes of the problem-by-problem checks of HALS beyond 128 components (tests/hals_wide_step.py),
proven on the CPU by the rule of tests/test_hals_step_bars.py: a numpy emulation of the device arithmetic defines each case's bar
(10 x its own deviation from the float64 reference), the faults a norm test cannot see are rejected and named -- first of all the
natural bug of a kernel that streams G in tiles, a block-Jacobi sweep -- and the float64 reference alone shows what every input
regime exercises.

Emulation of one half-step (F, B, lambda, X_prev), as the loop beyond 128 components forms it: G = F^T F in exact f32, r = F^T B
with the four split-bf16 terms (f32 accumulation) or in exact f32 (test_mur_step_bars.prod), 2 lambda added to the f32 diagonal,
then the sweep in float32 on a kept residual (test_hals_step_bars.sweep_kept_residual).  Not reproduced: the MFMA summation order
of the products and the fused multiply-adds of the kernel; the factor 10 between floor and bar is for those."""
import functools
import json
import os

import numpy as np
import pytest

import anls_step as A
import hals_step as HS
import hals_wide_step as HW
from test_hals_step_bars import sweep_kept_residual
from test_mur_step_bars import prod

F = np.float32
IDS = [HW.case_id(c) for c in HW.CASES]


def emu_half_step(f, b, lam, prev, sweeps, arith):
    k = f.shape[1]
    ft = np.ascontiguousarray(np.asarray(f, F).T)
    g = (prod(ft, np.asarray(f, F), terms="f32") + F(2 * lam) * np.eye(k, dtype=F)).astype(F)
    r = prod(ft, np.asarray(b, F), terms=4 if arith == "bf16" else "f32").astype(F)
    return sweep_kept_residual(g, r, prev, sweeps).astype(np.float64)


def sweep_block_jacobi(g, r, x, sweeps=1, block=64):
    """The planted fault of a tiled kernel: within a sweep every block of `block` components sees the other blocks' x from before
    the sweep (inside its own block the order is the definition's)."""
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    x = np.array(x, np.float64)
    k = g.shape[0]
    for _ in range(sweeps):
        old = x.copy()
        for a in range(0, k, block):
            xb = old.copy()
            for j in range(a, min(a + block, k)):
                if g[j, j] > 0:
                    xb[j] = np.maximum(xb[j] + (r[j] - g[j] @ xb) / g[j, j], 0)
            x[a:a + block] = xb[a:a + block]
    return x


@functools.lru_cache(maxsize=None)
def trajectory(c):
    """The emulated two-iteration run of a case: per half-step the float64 reference fed the emulation's previous f32 iterate,
    the emulation's own result and its deviation.  [(label, dict)]"""
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = HW.lam_of(c)
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
            first, numer1 = (xref, numer) if c.sweeps == 1 else HS.sweep(g, r, x0, 1)
            emu = emu_half_step(f, b, lam, x0, c.sweeps, c.arith)
            floor, _, _ = HS.values(f"{side}{s}", r, emu, xref, np.zeros_like(numer), np.inf, record=False)
            out.append((f"{side}{s}", dict(g=g, r=r, lam=lam, prev=x0, xref=xref, numer=numer, emu=emu, floor=floor,
                                           clamped=(numer1 < 0) & (np.diag(g) > 0)[:, None])))
            prev = (emu.T, prev[1]) if side == "W" else (prev[0], emu)
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def test_cases_stand_where_the_kernel_changes():
    """Every kp the kernel is instantiated for; a last tile and a last slot that are almost all padding; problem counts that leave
    waves of a block idle; both sides beyond one round of the grid (the kernel's own stride, as test_hals_step_bars.test_wrap_cases_wrap)."""
    assert {HW.kp_of(c.k) for c in HW.CASES} == set(range(256, 1025, 128))
    assert {HW.tile_rows(c.k) for c in HW.CASES} == {64, 32, 16}
    assert all(HW.MIN_K <= c.k <= HW.MAX_K for c in HW.CASES)
    ks = {c.k for c in HW.CASES}
    assert {129, 257, 1024} <= ks and 129 % 64 == 1 and 257 % 64 == 1
    assert any(c.m % HW.WAVES and c.n % HW.WAVES for c in HW.CASES) and {(1, 257), (257, 1)} <= {(c.m, c.n) for c in HW.CASES}
    big = [c for c in HW.CASES if max(c.m, c.n) > HW.wrap_stride()]
    assert {(c.m > c.n) for c in big} == {True, False}
    assert len(set(IDS)) == len(IDS) and set(IDS) == set(HW.BARS)


# ---- bars -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", HW.CASES, ids=IDS)
def test_emulation_defines_the_bar(c):
    """The emulation's largest deviation from the float64 reference is within the floor of the table, and the bar is 10 x that
    floor (NMFX_WRITE_HALS_BARS=<file>: append the figures instead, to rebuild the table)."""
    floor = max(h["floor"] for _, h in trajectory(c))
    path = os.environ.get("NMFX_WRITE_HALS_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": HW.case_id(c), "floor": floor}) + "\n")
        return
    table_floor, bar, _ = HW.BARS[HW.case_id(c)]
    assert bar == pytest.approx(10 * table_floor, rel=1e-12)
    assert floor <= table_floor, f"{HW.case_id(c)}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
    assert floor >= table_floor / 2, f"{HW.case_id(c)}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"


@pytest.mark.parametrize("c", HW.CASES, ids=IDS)
def test_emulation_passes_the_comparator(c):
    """The bar is measured with the comparator's rule for exact zeros switched off (as tests/test_hals_step_bars.py measures it).
    With the rule on, the emulated float32 sweep must pass at the floor itself on every half-step: a case on which float32
    cannot decide a clamp the float64 reference calls strict would fail on the device for no fault of the kernel."""
    if os.environ.get("NMFX_WRITE_HALS_BARS"):
        return
    for label, h in trajectory(c):
        worst, msg, _ = HS.values(f"{HW.case_id(c)} {label}", h["r"], h["emu"], h["xref"], h["numer"], HW.BARS[HW.case_id(c)][0], record=False)
        assert msg is None, msg


# ---- the bars of the public call (tests/test_gpu_hals_wide.py) --------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,sweeps", HW.PUBLIC_CASES, ids=[HW.public_id(*c) for c in HW.PUBLIC_CASES])
def test_emulated_public_trajectory_is_under_half_the_bars(m, n, k, sweeps):
    """Five emulated iterations (default arithmetic: split bf16) from the start the public call makes, against the float64 loop
    from the same start: the final product and the objective history stay under half of the bars the device is held to."""
    import math
    from test_gpu_hals import host_alpha, host_hals
    v = HW.public_v(m, n, k)
    lw, lh = HW.PUBLIC_LAMS
    w0, h0 = HW.public_start(m, n, k)
    a = host_alpha(v, w0, h0)
    w, h = A.f32(w0 * math.sqrt(a)), A.f32(h0 * math.sqrt(a))
    wr, hr, hist = host_hals(v, w, h, lw, lh, sweeps, HW.PUBLIC_ITERS)
    v64 = np.asarray(v, np.float64)
    vt = np.ascontiguousarray(v.T)
    emu_hist = [0.5 * np.sum((v64 - w @ h) ** 2)]
    for _ in range(HW.PUBLIC_ITERS):
        w = emu_half_step(np.ascontiguousarray(h.T), vt, lw, np.ascontiguousarray(w.T), sweeps, "bf16").T
        h = emu_half_step(w, v, lh, h, sweeps, "bf16")
        emu_hist.append(0.5 * np.sum((v64 - w @ h) ** 2))
    err = np.linalg.norm(w @ h - wr @ hr) / np.linalg.norm(v64)
    rel = float(np.max(np.abs(np.array(emu_hist) / hist - 1)))
    print(f"{HW.public_id(m, n, k, sweeps)}: emulated WH error {err:.2e} (bar {HW.PUBLIC_WH_BAR:.0e}), history {rel:.2e} (rtol {HW.PUBLIC_HIST_RTOL:.0e})")
    assert err < HW.PUBLIC_WH_BAR / 2 and rel < HW.PUBLIC_HIST_RTOL / 2


# ---- regimes: the reference alone -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in HW.CASES if c.regime != "mixed"], ids=lambda c: HW.case_id(c))
def test_regimes(c):
    """cold: more than half of W clamped in the first sweep; settled: no clamp in any half-step; dead: G_jj = 0 on variables 1
    and 3 in the first W half-step (they keep their start) and on variable 3 in the H half-step behind it, at lambda = 0."""
    steps = dict(trajectory(c))
    if c.regime == "cold":
        share = steps["W1"]["clamped"].mean()
        assert share > 0.5, f"{HW.case_id(c)}: {share:.0%} of W clamped in the first sweep"
    elif c.regime == "settled":
        for label, h in steps.items():
            assert not h["clamped"].any(), f"{HW.case_id(c)} {label}: {int(h['clamped'].sum())} entries clamped"
    elif c.regime == "dead":
        assert HW.lam_of(c) == (0.0, 0.0)
        w1, h1 = steps["W1"], steps["H1"]
        assert np.diag(w1["g"])[list(A.DEAD_VARS)].tolist() == [0.0, 0.0] and (np.diag(w1["g"]) > 0).sum() == c.k - 2
        for i in A.DEAD_VARS:
            assert np.array_equal(w1["xref"][i], w1["prev"][i])
        assert (w1["xref"][1] > 0).all() and (w1["xref"][3] == 0).all()
        assert np.diag(h1["g"])[3] == 0 and np.diag(h1["g"])[1] > 0 and (h1["xref"][3] == 0).all()


@pytest.mark.parametrize("c", [c for c in HW.CASES if c.regime == "mixed" and (c.m, c.n) == (257, 200) and c.sweeps == 1 and c.arith == "bf16"],
                         ids=lambda c: HW.case_id(c))
def test_mixed_clamps_and_frees_in_every_block(c):
    """mixed: clamped and free entries in every workgroup's block of problems, in every half-step."""
    for label, h in trajectory(c):
        cl = h["clamped"]
        for a in range(0, cl.shape[1] - HW.WAVES + 1, HW.WAVES):
            blk = cl[:, a:a + HW.WAVES]
            assert blk.any() and not blk.all(), f"{HW.case_id(c)} {label}: problems {a} .. {a + blk.shape[1] - 1}"


# ---- planted faults ---------------------------------------------------------------------------------------------------------------
def _reject(case, label, h, x_fault, what):
    """The comparator rejects x_fault at the case's bar and names the half-step, a problem and a variable."""
    bar = HW.bar_of(case)
    worst, msg, per = HS.values(f"{HW.case_id(case)} {label}", h["r"], x_fault, h["xref"], h["numer"], bar, record=False)
    assert msg is not None, f"{HW.case_id(case)} {label}: {what} passes: worst deviation {worst:.3e} <= bar {bar:.1e}"
    c = int(np.argmax(per))
    assert f"{label}: problem {c}, variable " in msg and "over the bar" in msg, msg
    return worst


@pytest.mark.parametrize("c", HW.CASES, ids=IDS)
def test_block_jacobi_is_rejected_on_every_case(c):
    """Each block of 64 components swept against the other blocks' x from before the sweep -- what a tiled kernel computes when a
    tile's steps do not reach the residual entries of the other slots.  The first W half-step, every problem: there it moves
    some problem by 0.2 (settled) to 14 (three sweeps) of its largest entry, 22 bars at 1 x 257 and 30 or more elsewhere.  (From
    the second iteration on the cold case at k = 300 and the single-row case have nothing left that it could move.)"""
    h = dict(trajectory(c))["W1"]
    x = sweep_block_jacobi(h["g"], h["r"], h["prev"], c.sweeps)
    _reject(c, "W1", h, x, "a block-Jacobi sweep")
    plain = HS.values("W1", h["r"], x, h["xref"], np.zeros_like(h["numer"]), np.inf, record=False)[0]
    print(f"{HW.case_id(c)}: block-Jacobi deviates by {plain:.3g} of a problem's largest entry, {plain / HW.bar_of(c):.0f} bars")
    assert plain > 5 * HW.bar_of(c)


FAULT_CASES = [HW.Case("mixed", 257, 200, 200, "bf16", 1), HW.Case("mixed", 257, 200, 384, "bf16", 3)]
FAULTS = ["block_jacobi", "block_jacobi_16", "jacobi", "reverse", "no_clamp", "sweeps_skipped"]


def plant(fault, h, c, sweeps):
    """Column c of the half-step's result with `fault`."""
    g, r, prev = h["g"], h["r"], h["prev"]
    k = g.shape[0]
    one = lambda **kw: HS.sweep(g, r[:, c:c + 1], prev[:, c:c + 1], kw.pop("sweeps", sweeps), **kw)[0][:, 0]
    if fault == "block_jacobi":
        return sweep_block_jacobi(g, r[:, c:c + 1], prev[:, c:c + 1], sweeps)[:, 0]
    if fault == "block_jacobi_16":                      # (the tile of the widest ranks)
        return sweep_block_jacobi(g, r[:, c:c + 1], prev[:, c:c + 1], sweeps, block=16)[:, 0]
    if fault == "jacobi":
        return one(jacobi=True)
    if fault == "reverse":
        return one(order=range(k - 1, -1, -1))
    if fault == "no_clamp":
        hit = np.nonzero(h["numer"][:, c] < 0)[0]
        return one(clamp_off=int(hit[0])) if len(hit) else h["xref"][:, c]
    if fault == "sweeps_skipped":
        return one(sweeps=1)
    raise ValueError(fault)


@pytest.mark.parametrize("fault", FAULTS)
def test_fault_in_one_problem_is_rejected_and_named(fault):
    """One fault in one problem of the W half-step of iteration 2 (lambda_w > 0, start: W_1), everything else the exact float64
    result: the comparator rejects it and names the problem.  The problem is the first one the fault moves by more than the bar."""
    case = FAULT_CASES[1] if fault == "sweeps_skipped" else FAULT_CASES[0]
    h = dict(trajectory(case))["W2"]
    assert h["lam"] > 0
    bar = HW.bar_of(case)
    top = h["xref"].max(axis=0)
    for prob in range(h["r"].shape[1] - 1):
        col = plant(fault, h, prob, case.sweeps)
        moved = np.abs(col - h["xref"][:, prob]).max() / top[prob]
        if moved > bar:
            break
    else:
        pytest.fail(f"{fault}: moves no problem by more than the bar {bar:.1e}")
    x = h["xref"].copy()
    x[:, prob] = col
    _, msg, per = HS.values("W2", h["r"], x, h["xref"], h["numer"], bar, record=False)
    assert msg and f"problem {prob}, variable " in msg and "1 of " in msg, msg
    assert (per > bar).sum() == 1


def test_exact_reference_passes():
    for case in FAULT_CASES:
        for label, h in trajectory(case):
            assert HS.values(label, h["r"], h["xref"], h["xref"], h["numer"], 0.0, record=False)[1] is None


def test_block_jacobi_with_one_block_is_the_sweep():
    """The planted fault is the definition wherever one block holds every component."""
    rng = np.random.default_rng(2)
    f = rng.uniform(0, 1, (90, 70))
    g, r = A.gram_rhs(f, rng.uniform(-1, 1, (90, 5)), 0.01)
    x0 = rng.uniform(0, 1, (70, 5))
    want = HS.sweep(g, r, x0, 2)[0]
    assert np.allclose(sweep_block_jacobi(g, r, x0, 2, block=128), want, rtol=1e-12, atol=1e-14)
    assert not np.allclose(sweep_block_jacobi(g, r, x0, 2, block=64), want, rtol=1e-3, atol=1e-6)
