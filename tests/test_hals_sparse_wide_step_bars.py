"""The bars of the problem-by-problem checks of sparse HALS with 129 .. 256 components (tests/sparse_hals_wide_step.py), proven
on the CPU: the numpy emulation of the device arithmetic of tests/test_hals_sparse_step_bars.py -- the arithmetic of a half-step
is the same at these ranks, only its route through the launches differs -- defines each case's bar (10 x its own deviation from
the float64 reference over a two-iteration trajectory), passes the comparator on every case, and the faults the new route could
have are rejected on named cases.

Emulation of one half-step (F, B, lambda, X_prev): G = F^T F in float64 rounded to f32, 2 lambda added to the f32 diagonal;
r = F^T b summed in float32 on the W side and in float64, rounded once, on the H side; the sweep in float32 on a kept residual.
The recorded objective is emulated as the device forms it: 1/2 [||X||^2 - 2 Sum_c <h_c, r_c> + <W^T W, H H^T>] in float64 with
r the H side's unrounded float64 sums."""
import functools
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp

import hals_step as HS
import sparse_hals_wide_step as SW
from test_hals_sparse_step_bars import emu_half_step

F = np.float32
IDS = [SW.case_id(c) for c in SW.CASES]


@functools.lru_cache(maxsize=None)
def trajectory(c):
    """The emulated two-iteration run of a case, as tests/test_hals_sparse_step_bars.py::trajectory.  [(label, dict)]"""
    x = SW.matrix(c.matrix)
    xt = sp.csr_matrix(x.T)
    w0, h0 = SW.start(c)
    lw, lh = SW.lam_of(c)
    out = []
    prev = (w0, h0)
    for s in (1, 2):
        for side in "WH":
            if side == "W":
                f, b, lam, x0 = np.ascontiguousarray(prev[1].T), xt, lw, np.ascontiguousarray(prev[0].T)
            else:
                f, b, lam, x0 = prev[0], x, lh, prev[1]
            g, r = SW.gram_rhs(f, b, lam)
            xref, numer = HS.sweep(g, r, x0, c.sweeps)
            emu = emu_half_step(f, b, lam, x0, c.sweeps, side)
            floor, msg, _ = SW.values(f"{side}{s}", g, r, emu, xref, np.zeros_like(numer), x0, np.inf, record=False)
            out.append((f"{side}{s}", dict(f=f, b=b, g=g, r=r, lam=lam, prev=x0, xref=xref, numer=numer, emu=emu, floor=floor, side=side)))
            prev = (emu.T, prev[1]) if side == "W" else (prev[0], emu)
    return out


# ---- bars -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SW.CASES, ids=IDS)
def test_emulation_defines_the_bar(c):
    """The emulation's largest deviation from the float64 reference is within the floor of the table, and the bar is 10 x that
    floor (NMFX_WRITE_HALS_BARS=<file>: append the figures instead, to rebuild the table)."""
    floor = max(h["floor"] for _, h in trajectory(c))
    path = os.environ.get("NMFX_WRITE_HALS_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": SW.case_id(c), "floor": floor}) + "\n")
        return
    table_floor, bar, _ = SW.BARS[SW.case_id(c)]
    assert bar == pytest.approx(10 * table_floor, rel=1e-12)
    assert floor <= table_floor, f"{SW.case_id(c)}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
    assert floor >= table_floor / 2, f"{SW.case_id(c)}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"


@pytest.mark.parametrize("c", SW.CASES, ids=IDS)
def test_emulation_passes_the_comparator(c):
    """Every half-step of the emulated trajectory passes the comparator at the case's bar, the exact-zero rule included: a case
    the float32 arithmetic itself cannot pass would ask the device for more than its number format."""
    bar = SW.bar_of(c)
    for label, h in trajectory(c):
        _, msg, _ = SW.values(label, h["g"], h["r"], h["emu"], h["xref"], h["numer"], h["prev"], bar, record=False)
        assert msg is None, msg


def test_the_table_has_every_case_and_no_other():
    assert sorted(SW.BARS) == sorted(IDS)


def test_cases_stand_where_the_route_changes():
    ks = {c.k for c in SW.CASES if c.matrix == "base"}
    assert {129, 200, 255, 256} <= ks and all(SW.MIN_K <= c.k <= SW.MAX_K for c in SW.CASES)
    assert 129 % SW.TILE == 1 and 256 % SW.TILE == 0            # a last tile with one live row, and a full one
    rows = SW.matrix("rows")
    assert np.diff(rows.indptr)[SW.LONG_ROW] == 2 * SW.CHUNK + 1
    tall = SW.matrix("tall")
    assert tall.shape[0] > 4 * 256 * 8 and tall.shape[0] > 2 * 256 * 8      # gather grid and sweep grid, 256 CUs
    assert {c.regime for c in SW.CASES} == {"scaled", "cold", "settled", "dead"} and any(c.sweeps == 3 for c in SW.CASES)
    lams = {SW.lam_of(c) for c in SW.CASES}
    assert any(lw > 0 for lw, _ in lams) and any(lh > 0 for _, lh in lams)


# ---- planted faults -------------------------------------------------------------------------------------------------------------
LAM_H_CASE = SW.Case("base", 200, "scaled", 1)           # k % 3 = 2: lambda_h > 0
LAM_W_CASE = SW.Case("base", 256, "scaled", 1)           # k % 3 = 1: lambda_w > 0
ROWS_CASE = SW.Case("rows", 129, "scaled", 1)


def rejected(label, h, x, bar):
    return SW.values(label, h["g"], h["r"], x, h["xref"], h["numer"], h["prev"], bar, record=False)[1]


@pytest.mark.parametrize("c,label", [(LAM_H_CASE, "H2"), (LAM_W_CASE, "W2")], ids=["lambda_h", "lambda_w"])
def test_gram_without_the_ridge_is_rejected(c, label):
    """G without 2 lambda I (the diagonal the sweep adds while it stages a tile), everything else exact."""
    h = dict(trajectory(c))[label]
    assert h["lam"] > 0
    k = h["g"].shape[0]
    x = HS.sweep(h["g"] - 2 * h["lam"] * np.eye(k), h["r"], h["prev"], c.sweeps)[0]
    msg = rejected(label, h, x, SW.bar_of(c))
    assert msg and "problem " in msg and "variable " in msg, msg


@pytest.mark.parametrize("label", ["W2", "H2"])
def test_a_jacobi_sweep_is_rejected(label):
    """Every step from the old x (a tile consumed without the steps before it): Gauss-Seidel is the definition."""
    h = dict(trajectory(LAM_H_CASE))[label]
    x = HS.sweep(h["g"], h["r"], h["prev"], 1, jacobi=True)[0]
    msg = rejected(label, h, x, SW.bar_of(LAM_H_CASE))
    assert msg and "problem " in msg, msg


@pytest.mark.parametrize("piece", [0, 1, 2])
def test_a_piece_dropped_from_the_long_row_is_rejected(piece):
    """One piece of the 513-non-zero row (256, 256 and 1 non-zeros) never reaches r: the comparator rejects that problem and no
    other."""
    h = dict(trajectory(ROWS_CASE))["W2"]
    bar = SW.bar_of(ROWS_CASE)
    b = sp.csc_matrix(h["b"], dtype=np.float64)        # (W side: B = X^T, problem c is column c)
    lo, hi = b.indptr[SW.LONG_ROW], b.indptr[SW.LONG_ROW + 1]
    assert hi - lo == 2 * SW.CHUNK + 1
    keep = np.ones(hi - lo, bool)
    keep[piece * SW.CHUNK:(piece + 1) * SW.CHUNK] = False
    rc = (np.asarray(h["f"], np.float64)[b.indices[lo:hi][keep]] * b.data[lo:hi][keep, None]).sum(axis=0)
    x = h["xref"].copy()
    x[:, SW.LONG_ROW] = HS.sweep(h["g"], rc[:, None], h["prev"][:, SW.LONG_ROW:SW.LONG_ROW + 1], 1)[0][:, 0]
    _, msg, per = SW.values("W2", h["g"], h["r"], x, h["xref"], h["numer"], h["prev"], bar, record=False)
    assert msg and f"problem {SW.LONG_ROW}, variable " in msg and "1 of " in msg, msg
    assert (per > bar).sum() == 1


def recorded_objective(x, w, h, r):
    """The objective as the device records it after an H half-step: the cross term from the H side's right-hand sides."""
    xd = x.data.astype(np.float64)
    cross = float(np.sum(np.asarray(h, np.float64) * np.asarray(r, np.float64)))
    return 0.5 * (float(np.dot(xd, xd)) - 2.0 * cross + float(np.sum((w.T @ w) * (h @ h.T))))


@pytest.mark.parametrize("c", [ROWS_CASE, SW.Case("300x1", 129, "scaled", 1)], ids=SW.case_id)
def test_rhs_rounded_before_the_cross_term_is_rejected(c):
    """The cross term <h_c, r_c> needs r as it was summed, in float64: with the float32 image the sweep reads, the recorded
    objective misses OBJ_RTOL; with the float64 sums it holds it.  The cases are the ones with a nearly exact fit, where the
    objective is a small difference of the three terms: the fault costs 9e-9 .. 4e-8 on rows and 1e-6 on 300x1 (against 1e-14
    with the float64 sums).  On the base matrix the 120000 roundings of one sign each average out to 3e-12 .. 2e-9 of a large
    objective, on either side of OBJ_RTOL: no case for this fault."""
    x = SW.matrix(c.matrix)
    traj = dict(trajectory(c))
    scale = SH_scale(x)
    for s in (1, 2):
        w, h, r = traj[f"H{s}"]["f"], traj[f"H{s}"]["emu"], traj[f"H{s}"]["r"]
        want = SW.objective(x, w, h)
        good = abs(recorded_objective(x, w, h, r) - want) / max(abs(want), scale)
        bad = abs(recorded_objective(x, w, h, r.astype(F)) - want) / max(abs(want), scale)
        assert good <= SW.OBJ_RTOL, (s, good)
        assert bad > SW.OBJ_RTOL, (s, bad)


def SH_scale(x):
    from mur_step import OBJ_FLOOR
    return OBJ_FLOOR * 0.5 * float(np.sum(x.data.astype(np.float64) ** 2))
