"""The bars of the problem-by-problem masked HALS checks (tests/masked_hals_step.py), proven on the CPU: a numpy emulation of the
device arithmetic defines each case's bar (10 x its own deviation from the float64 reference over a two-iteration trajectory,
the rule and margin of tests/test_hals_sparse_step_bars.py), the faults a norm test cannot see are rejected and named by
problem and variable, the matrices are what the cases say, and masked_start_scale is the float64 alpha.

Emulation of one half-step: every problem's G = Sum f f^T and r = Sum v f summed in float32 over its observed entries,
(float) 2 lambda added to the f32 diagonal, then test_hals_step_bars.sweep_kept_residual's sweep in float32 with one G per
problem, the form the kernel runs.  Not reproduced: the order in which the MFMA and a long row's waves add, and the fused
multiply-adds; the factor 10 between floor and bar is for those."""
import functools
import json
import os

import numpy as np
import pytest

import anls_step as A
import hals_step as HS
import masked_hals_step as MH

F = np.float32
IDS = [MH.case_id(c) for c in MH.CASES]


def sweep_kept_residual(g, r, x, sweeps):
    """test_hals_step_bars.sweep_kept_residual with one G per problem (g: problems x k x k)."""
    g, r, x = np.asarray(g, F), np.asarray(r, F), np.array(x, F)
    k = g.shape[1]
    diag = np.einsum("pjj->jp", g)
    live = diag > 0
    inv = np.where(live, F(1) / np.where(live, diag, F(1)), F(0)).astype(F)
    res = r.copy()
    for l in range(k):
        res = (res - g[:, :, l].T * x[l:l + 1]).astype(F)
    for _ in range(sweeps):
        for j in range(k):
            d = np.where(live[j], np.maximum(-x[j], res[j] * inv[j]), F(0)).astype(F)
            x[j] = x[j] + d
            res = (res - g[:, :, j].T * d[None, :]).astype(F)
    return x


def emu_half_step(f, obs, lam, prev, sweeps):
    g, r = MH.systems(f, obs, lam, dtype=F)
    return sweep_kept_residual(g, r, prev, sweeps).astype(np.float64)


@functools.lru_cache(maxsize=None)
def trajectory(c):
    """The emulated two-iteration run of a case: per half-step the float64 reference fed the emulation's previous f32 iterate,
    the emulation's own result and its deviation.  [(label, dict)]"""
    by_rows, by_cols = MH.observed(c.matrix)
    w0, h0 = MH.start(c)
    lw, lh = MH.lam_of(c)
    out = []
    prev = (w0, h0)
    for s in (1, 2):
        for side in "WH":
            if side == "W":
                f, obs, lam, x0 = np.ascontiguousarray(prev[1].T), by_rows, lw, np.ascontiguousarray(prev[0].T)
            else:
                f, obs, lam, x0 = prev[0], by_cols, lh, prev[1]
            g, r = MH.systems(f, obs, lam)
            xref, numer = MH.sweep(g, r, x0, c.sweeps)
            emu = emu_half_step(f, obs, lam, x0, c.sweeps)
            floor, _, _ = MH.values(f"{side}{s}", g, r, emu, xref, np.zeros_like(numer), x0, np.inf, record=False)
            out.append((f"{side}{s}", dict(f=f, obs=obs, g=g, r=r, lam=lam, prev=x0, xref=xref, numer=numer, emu=emu, floor=floor, side=side)))
            prev = (emu.T, prev[1]) if side == "W" else (prev[0], emu)
    return out


# ---- bars -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", MH.CASES, ids=IDS)
def test_emulation_defines_the_bar(c):
    """The emulation's largest deviation from the float64 reference is within the floor of the table, and the bar is 10 x that
    floor (NMFX_WRITE_HALS_BARS=<file>: append the figures instead, to rebuild the table)."""
    floor = max(h["floor"] for _, h in trajectory(c))
    path = os.environ.get("NMFX_WRITE_HALS_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": MH.case_id(c), "floor": floor}) + "\n")
        return
    table_floor, bar, _ = MH.BARS[MH.case_id(c)]
    assert bar == pytest.approx(10 * table_floor, rel=1e-12)
    assert floor <= table_floor, f"{MH.case_id(c)}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
    assert floor >= table_floor / 2, f"{MH.case_id(c)}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"


def test_the_table_has_every_case_and_no_other():
    assert sorted(MH.BARS) == sorted(IDS)
    assert all(measured <= bar for _, bar, measured in MH.BARS.values())


def test_the_cases_are_the_ones_the_checks_were_set_for():
    ids = set(IDS)
    assert {f"base-k{k}-scaled" for k in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)} <= ids
    assert {"rows-k8-scaled", "rows-k40-scaled", "1x300-k4-scaled", "300x1-k4-scaled", "5x4-k4-scaled", "tall-k8-scaled", "full-k8-scaled"} <= ids
    assert {"base-k40-cold", "base-k40-settled", "base-k40-dead", "base-k40-scaled-s3", "base-k64-scaled-s3"} <= ids
    assert all(MH.lam_of(c) == (0.0, 0.0) if c.regime == "dead" else MH.lam_of(c) == A.LAMS[c.k % 3] for c in MH.CASES)


# ---- the matrices are what the cases say ----------------------------------------------------------------------------------------
def test_matrices():
    for name in ("base", "rows", "tall", "1x300", "300x1", "5x4", "full"):
        x, mask = MH.matrix(name)
        assert x.dtype == np.float32 and mask.dtype == bool and x.shape == mask.shape
        assert np.isnan(x[~mask]).all() and np.isfinite(x[mask]).all() and (x[mask] >= 0).all()
        by_rows, by_cols = MH.observed(name)
        assert by_rows.indptr[-1] == by_cols.indptr[-1] == mask.sum()
        if mask.sum() >= 200:
            assert 0.05 < (x[mask] == 0).mean() < 0.15, name          # observed zeros: data
            assert (by_rows.data == 0).sum() == (by_cols.data == 0).sum() == (x[mask] == 0).sum()
    _, base = MH.matrix("base")
    counts, ccounts = base.sum(axis=1), base.sum(axis=0)
    assert base.shape == (700, 600) and counts[3] == 599 - 1 and ccounts[11] == 700 - 2 and counts[3] > 2 * MH.CHUNK and ccounts[11] > 2 * MH.CHUNK
    assert counts[0] == counts[350] == 0 and ccounts[1] == ccounts[599] == 0
    assert (counts < 16).mean() > 0.5 and (ccounts < 32).mean() > 0.5       # rank-deficient Grams at k >= 16 / 32
    _, rows = MH.matrix("rows")
    assert rows.shape == (40, 600) and tuple(rows.sum(axis=1)[:8]) == MH.ROW_COUNTS == (1, 3, 4, 5, 255, 256, 257, 513)
    assert MH.matrix("1x300")[1].sum() > MH.CHUNK and MH.matrix("300x1")[1].sum() > MH.CHUNK
    _, tall = MH.matrix("tall")
    assert tall.shape == (20000, 40) and tall.shape[0] / 8 > 4 * 256        # more blocks of 8 waves than one round of the grid on 256 CUs
    _, full = MH.matrix("full")
    assert full.shape == (64, 48) and full.all()


def test_regimes():
    settled = dict(trajectory(MH.Case("base", 40, "settled", 1)))
    cold = dict(trajectory(MH.Case("base", 40, "cold", 1)))
    dead = dict(trajectory(MH.Case("base", 40, "dead", 1)))
    clamped = lambda h: float(((h["prev"] > 0) & (h["xref"] == 0)).mean())      # positive entries the half-step sets to zero
    assert clamped(cold["W1"]) > 2 * max(clamped(h) for h in settled.values()), (clamped(cold["W1"]), [clamped(h) for h in settled.values()])
    for label in ("W1", "H1", "W2", "H2"):
        h = dead[label]
        assert (h["g"][:, MH.DEAD, MH.DEAD] == 0).all()
        assert np.array_equal(h["xref"][MH.DEAD], h["prev"][MH.DEAD]) and (h["xref"][MH.DEAD] == 0).all()
    lams = {MH.lam_of(c) for c in MH.CASES}
    assert any(lw > 0 for lw, _ in lams) and any(lh > 0 for _, lh in lams)


# ---- planted faults -------------------------------------------------------------------------------------------------------------
FAULT_CASE = MH.Case("base", 64, "scaled", 1)            # k % 3 = 1: lambda_w > 0
FAULTS = ["shared_gram", "zeros_dropped", "no_lambda", "stale_gram", "rhs_outside_mask"]


def planted(fault, h):
    """The W half-step's result (k x problems) with `fault` in every problem."""
    f, obs, lam, prev = h["f"], h["obs"], h["lam"], h["prev"]
    g, r = h["g"], h["r"]
    if fault == "shared_gram":                          # unmasked HALS's F^T F + 2 lambda I for every row
        g = MH.systems(f, obs, lam, shared=True)[0]
    elif fault == "zeros_dropped":                      # an observed zero treated as missing
        g = MH.systems(f, obs, lam, drop_zeros=True)[0]
    elif fault == "no_lambda":
        g = MH.systems(f, obs, 0.0)[0]
    elif fault == "stale_gram":                         # a row swept on the G the wave's LDS region held for the row before
        g = np.roll(g, 1, axis=0)
    elif fault == "rhs_outside_mask":                   # r over the whole row of a filled-in x (0.5 where nothing was observed)
        x, mask = MH.matrix(FAULT_CASE.matrix)
        filled = np.where(mask, x, np.float32(0.5)).astype(np.float64)
        r = np.asarray(f, np.float64).T @ filled.T
    else:
        raise ValueError(fault)
    return MH.sweep(g, r, prev, 1)[0]


@pytest.mark.parametrize("fault", FAULTS)
def test_fault_in_one_problem_is_rejected_and_named(fault):
    """One fault in one problem of the W half-step of iteration 2 (lambda_w > 0), everything else the exact float64 result: the
    comparator rejects it and names the problem and a variable.  The problem is the first one the fault moves by more than
    the bar."""
    h = dict(trajectory(FAULT_CASE))["W2"]
    assert h["lam"] > 0
    bar = MH.bar_of(FAULT_CASE)
    bad = planted(fault, h)
    top = h["xref"].max(axis=0)
    moved = np.abs(bad - h["xref"]).max(axis=0) / np.where(top > 0, top, 1.0)
    hit = np.nonzero(moved > bar)[0]
    assert len(hit), f"{fault}: moves no problem by more than the bar {bar:.1e}"
    prob = int(hit[0])
    x = h["xref"].copy()
    x[:, prob] = bad[:, prob]
    _, msg, per = HS.values("W2", h["r"], x, h["xref"], h["numer"], bar, record=False)
    assert msg and f"problem {prob}, variable " in msg and "1 of " in msg, msg
    assert (per > bar).sum() == 1


def test_exact_reference_passes():
    for label, h in trajectory(FAULT_CASE):
        assert HS.values(label, h["r"], h["xref"], h["xref"], h["numer"], 0.0, record=False)[1] is None


def test_all_ones_mask_is_the_shared_gram_sweep():
    """The `full` case: every problem's own system is hals_step's shared (G, r), and the batched sweep is hals_step.sweep."""
    c = MH.Case("full", 8, "scaled", 1)
    x, mask = MH.matrix("full")
    v = x.astype(np.float64)
    w0, h0 = MH.start(c)
    lw, lh = 0.05, 0.02
    w, h, hist = MH.host_hals("full", w0, h0, lw, lh, 2, 3)
    wd, hd = w0, h0
    for _ in range(3):
        g, r = A.gram_rhs(np.ascontiguousarray(hd.T), np.ascontiguousarray(v.T), lw)
        wd = HS.sweep(g, r, wd.T, 2)[0].T
        g, r = A.gram_rhs(wd, v, lh)
        hd = HS.sweep(g, r, hd, 2)[0]
    assert np.allclose(w, wd, rtol=1e-10, atol=1e-14) and np.allclose(h, hd, rtol=1e-10, atol=1e-14)
    assert hist[-1] == pytest.approx(0.5 * np.sum((v - wd @ hd) ** 2), rel=1e-12)
    for _, hs in trajectory(c):
        gs, rs = (A.gram_rhs(hs["f"], v.T if hs["side"] == "W" else v, hs["lam"]))
        assert np.allclose(hs["g"], gs[None], rtol=1e-12, atol=1e-15) and np.allclose(hs["r"], rs, rtol=1e-12, atol=1e-15)


# ---- the start scale ------------------------------------------------------------------------------------------------------------
class FakeEngine:
    """An engine whose objective_f64 is nmf_amd.masked.objective of the factors last set."""

    def __init__(self, name):
        self.name, self.sets = name, []

    def set_factors(self, w, h):
        self.sets.append((np.array(w, dtype=np.float64), np.array(h, dtype=np.float64)))

    def objective_f64(self):
        return MH.objective(self.name, *self.sets[-1])


@pytest.mark.parametrize("regime", ["scaled", "cold"])
def test_masked_start_scale_is_the_float64_alpha(regime):
    from nmf_amd.hals import masked_start_scale, scaled_start
    c = MH.Case("base", 8, regime, 1)
    w0, h0 = MH.start(c)
    eng = FakeEngine("base")
    alpha = masked_start_scale(eng, w0, h0)
    want = MH.alpha_of("base", w0, h0)
    assert abs(alpha - want) <= 1e-9 * abs(want), (alpha, want)
    if regime == "scaled":
        assert abs(alpha - 1) < 1e-5                      # (the start was scaled by its own alpha, rounded to f32)
    else:
        assert alpha < 0.5
    assert len(eng.sets) == 3 and np.array_equal(eng.sets[-1][0], w0) and np.array_equal(eng.sets[-1][1], h0)      # (w0, h0) left set
    ws, hs = scaled_start(alpha, w0, h0)
    assert np.allclose(ws, w0 * np.sqrt(want)) and np.allclose(hs, h0 * np.sqrt(want))


def test_masked_start_scale_of_a_zero_start_is_none():
    from nmf_amd.hals import masked_start_scale, scaled_start
    w0, h0 = np.zeros((700, 8)), np.zeros((8, 600))
    eng = FakeEngine("base")
    assert masked_start_scale(eng, w0, h0) is None
    ws, hs = scaled_start(None, w0, h0)
    assert ws is w0 and hs is h0
