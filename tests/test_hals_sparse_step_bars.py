"""The bars of the problem-by-problem sparse HALS checks (tests/sparse_hals_step.py), proven on the CPU: a numpy emulation of
the device arithmetic defines each case's bar (10 x its own deviation from the float64 reference over a two-iteration
trajectory, the rule and margin of tests/test_hals_step_bars.py), and the faults a norm test cannot see are rejected and
named by problem and variable.

Emulation of one half-step (F, B, lambda, X_prev): G = F^T F in float64 rounded to f32 (sp_stats_kernel sums in f64), 2 lambda
added to the f32 diagonal; r = F^T b summed in float32 over the non-zeros on the W side (the W phase accumulates in f32) and
in float64, rounded once, on the H side (the H phase accumulates in f64); then test_hals_step_bars.sweep_kept_residual in
float32, the form the kernel runs.  Not reproduced: the order in which a wave's groups and a long row's pieces are added, and
the fused multiply-adds; the factor 10 between floor and bar is for those."""
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import hals_step as HS
import sparse_hals_step as SH
from test_hals_step_bars import sweep_kept_residual

F = np.float32
IDS = [SH.case_id(c) for c in SH.CASES]


def emu_rhs(f, b, side):
    """r (k x problems) as the device rounds it."""
    if side == "W":
        return np.asarray((sp.csr_matrix(b, dtype=F).T @ np.asarray(f, F)).T, dtype=F)
    return np.asarray((sp.csr_matrix(b, dtype=np.float64).T @ np.asarray(f, np.float64)).T).astype(F)


def emu_half_step(f, b, lam, prev, sweeps, side, r=None):
    k = f.shape[1]
    f64 = np.asarray(f, np.float64)
    g = ((f64.T @ f64).astype(F) + F(2 * lam) * np.eye(k, dtype=F)).astype(F)
    if r is None:
        r = emu_rhs(f, b, side)
    return sweep_kept_residual(g, r, prev, sweeps).astype(np.float64)


@functools.lru_cache(maxsize=None)
def trajectory(c):
    """The emulated two-iteration run of a case: per half-step the float64 reference fed the emulation's previous f32 iterate,
    the emulation's own result and its deviation.  [(label, dict)]"""
    x = SH.matrix(c.matrix)
    xt = sp.csr_matrix(x.T)
    w0, h0 = SH.start(c)
    lw, lh = SH.lam_of(c)
    out = []
    prev = (w0, h0)
    for s in (1, 2):
        for side in "WH":
            if side == "W":
                f, b, lam, x0 = np.ascontiguousarray(prev[1].T), xt, lw, np.ascontiguousarray(prev[0].T)
            else:
                f, b, lam, x0 = prev[0], x, lh, prev[1]
            g, r = SH.gram_rhs(f, b, lam)
            xref, numer = HS.sweep(g, r, x0, c.sweeps)
            emu = emu_half_step(f, b, lam, x0, c.sweeps, side)
            floor, _, _ = SH.values(f"{side}{s}", g, r, emu, xref, np.zeros_like(numer), x0, np.inf, record=False)
            out.append((f"{side}{s}", dict(f=f, b=b, g=g, r=r, lam=lam, prev=x0, xref=xref, numer=numer, emu=emu, floor=floor, side=side)))
            prev = (emu.T, prev[1]) if side == "W" else (prev[0], emu)
    return out


# ---- bars -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SH.CASES, ids=IDS)
def test_emulation_defines_the_bar(c):
    """The emulation's largest deviation from the float64 reference is within the floor of the table, and the bar is 10 x that
    floor (NMFX_WRITE_HALS_BARS=<file>: append the figures instead, to rebuild the table)."""
    floor = max(h["floor"] for _, h in trajectory(c))
    path = os.environ.get("NMFX_WRITE_HALS_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": SH.case_id(c), "floor": floor}) + "\n")
        return
    table_floor, bar, _ = SH.BARS[SH.case_id(c)]
    assert bar == pytest.approx(10 * table_floor, rel=1e-12)
    assert floor <= table_floor, f"{SH.case_id(c)}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
    assert floor >= table_floor / 2, f"{SH.case_id(c)}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"


def test_the_table_has_every_case_and_no_other():
    assert sorted(SH.BARS) == sorted(IDS)


# ---- the matrices are what the cases say ----------------------------------------------------------------------------------------
def test_matrices():
    base = SH.matrix("base")
    counts = np.diff(base.indptr)
    ccounts = np.diff(base.tocsc().indptr)
    assert counts[3] == 599 - 1 and ccounts[11] == 700 - 2 and counts[3] > 2 * SH.CHUNK and ccounts[11] > 2 * SH.CHUNK      # (minus the empty columns / rows)
    assert counts[0] == counts[350] == 0 and ccounts[1] == ccounts[599] == 0
    rows = SH.matrix("rows")
    assert tuple(np.diff(rows.indptr)[:5]) == SH.ROW_COUNTS
    assert np.diff(SH.matrix("1x300").indptr)[0] > SH.CHUNK and np.diff(SH.matrix("300x1").tocsc().indptr)[0] > SH.CHUNK
    tall = SH.matrix("tall")
    assert tall.shape[0] / 8 > 4 * 256                 # more blocks of 8 waves than one round of the grid on 256 CUs
    for name in ("base", "rows", "tall", "1x300", "300x1", "5x4"):
        assert SH.matrix(name).dtype == np.float32 and (SH.matrix(name).data > 0).all()


def test_regimes():
    settled = dict(trajectory(SH.Case("base", 40, "settled", 1)))
    cold = dict(trajectory(SH.Case("base", 40, "cold", 1)))
    dead = dict(trajectory(SH.Case("base", 40, "dead", 1)))
    clamped = lambda h: float(((h["prev"] > 0) & (h["xref"] == 0)).mean())      # positive entries the half-step sets to zero
    assert clamped(cold["W1"]) > 0.5, clamped(cold["W1"])
    for label, h in settled.items():
        assert clamped(h) < 0.05, (label, clamped(h))
    assert SH.lam_of(SH.Case("base", 40, "dead", 1)) == (0.0, 0.0)
    for label in ("W1", "H1", "W2", "H2"):
        h = dead[label]
        assert np.diag(h["g"])[SH.DEAD] == 0 and (np.diag(h["g"]) > 0).sum() == 39
        assert np.array_equal(h["xref"][SH.DEAD], h["prev"][SH.DEAD]) and (h["xref"][SH.DEAD] == 0).all()
    lams = {SH.lam_of(c) for c in SH.CASES}
    assert any(lw > 0 for lw, _ in lams) and any(lh > 0 for _, lh in lams)


# ---- planted faults -------------------------------------------------------------------------------------------------------------
FAULT_CASE = SH.Case("base", 64, "scaled", 1)            # k % 3 = 1: lambda_w > 0
FAULTS = ["reverse", "jacobi", "no_clamp", "piece_dropped"]
LONG_ROW = 3                                           # the dense row of the base matrix: three pieces


def plant(fault, h, c):
    """Column c of the W half-step's result with `fault`."""
    g, r, prev = h["g"], h["r"], h["prev"]
    k = g.shape[0]
    one = lambda **kw: HS.sweep(g, kw.pop("r", r[:, c:c + 1]), prev[:, c:c + 1], 1, **kw)[0][:, 0]
    if fault == "reverse":
        return one(order=range(k - 1, -1, -1))
    if fault == "jacobi":
        return one(jacobi=True)
    if fault == "no_clamp":
        hit = np.nonzero(h["numer"][:, c] < 0)[0]
        return one(clamp_off=int(hit[0])) if len(hit) else h["xref"][:, c]
    if fault == "piece_dropped":                       # the second piece of the row's non-zeros never reaches r
        b = sp.csc_matrix(h["b"], dtype=np.float64)    # (W side: B = X^T, problem c is column c)
        lo, hi = b.indptr[c], b.indptr[c + 1]
        if hi - lo <= SH.CHUNK:
            return h["xref"][:, c]
        keep = np.ones(hi - lo, bool)
        keep[SH.CHUNK:2 * SH.CHUNK] = False
        rc = (np.asarray(h["f"], np.float64)[b.indices[lo:hi][keep]] * b.data[lo:hi][keep, None]).sum(axis=0)
        return one(r=rc[:, None])
    raise ValueError(fault)


@pytest.mark.parametrize("fault", FAULTS)
def test_fault_in_one_problem_is_rejected_and_named(fault):
    """One fault in one problem of the W half-step of iteration 2 (lambda_w > 0), everything else the exact float64 result: the
    comparator rejects it and names the problem and a variable.  The problem is the first one the fault moves by more than
    the bar; a dropped piece can only show in the long row."""
    h = dict(trajectory(FAULT_CASE))["W2"]
    assert h["lam"] > 0
    bar = SH.bar_of(FAULT_CASE)
    top = h["xref"].max(axis=0)
    for prob in range(h["r"].shape[1]):
        col = plant(fault, h, prob)
        moved = np.abs(col - h["xref"][:, prob]).max() / (top[prob] if top[prob] > 0 else 1.0)
        if moved > bar:
            break
    else:
        pytest.fail(f"{fault}: moves no problem by more than the bar {bar:.1e}")
    if fault == "piece_dropped":
        assert prob == LONG_ROW
    x = h["xref"].copy()
    x[:, prob] = col
    _, msg, per = HS.values("W2", h["r"], x, h["xref"], h["numer"], bar, record=False)
    assert msg and f"problem {prob}, variable " in msg and "1 of " in msg, msg
    assert (per > bar).sum() == 1


def test_exact_reference_passes():
    for label, h in trajectory(FAULT_CASE):
        assert HS.values(label, h["r"], h["xref"], h["xref"], h["numer"], 0.0, record=False)[1] is None


def test_host_loop_is_the_dense_definition():
    """The float64 loop on the non-zeros against tests/test_gpu_hals.py's loop on x.toarray()."""
    import anls_step as A
    c = SH.Case("5x4", 4, "scaled", 1)
    x = SH.matrix("5x4")
    w0, h0 = SH.start(c)
    w, h, hist = SH.host_hals(x, w0, h0, 0.05, 0.02, 2, 3)
    v = x.toarray().astype(np.float64)
    wd, hd = w0, h0
    for _ in range(3):
        g, r = A.gram_rhs(np.ascontiguousarray(hd.T), np.ascontiguousarray(v.T), 0.05)
        wd = HS.sweep(g, r, wd.T, 2)[0].T
        g, r = A.gram_rhs(wd, v, 0.02)
        hd = HS.sweep(g, r, hd, 2)[0]
    assert np.allclose(w, wd, rtol=1e-12, atol=1e-15) and np.allclose(h, hd, rtol=1e-12, atol=1e-15)
    assert hist[-1] == pytest.approx(0.5 * np.sum((v - wd @ hd) ** 2), rel=1e-12)
