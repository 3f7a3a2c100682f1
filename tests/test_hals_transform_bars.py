"""The bars of the HALS fold-in checks (tests/hals_transform_step.py), proven on the CPU: a float32 emulation of the kernel's
form (kept residual, refresh every 16 sweeps, the stop rule in f32) defines each case's value bar and the slack of the stop
rule, planted faults are caught, and the stop-rule cases are not vacuous."""
import functools
import json
import os

import numpy as np
import pytest

import hals_transform_step as T

LONG, STOP = T.LONG, T.STOP


@functools.lru_cache(maxsize=None)
def emulated(c):
    """The emulation's two runs of a case with the float64 reference of each (the STOP reference run for the emulation's own
    counts): {'long': (emu, ref), 'stop': (emu, ref)}."""
    p = T.problem(c)
    g32, r32 = T.systems_f32(c)
    out = {}
    emu = T.emu_solve(g32, r32, p.h0, **LONG)
    out["long"] = (emu, T.solve(p.g, p.r, p.h0, 0.0, LONG["max_sweeps"], counts=np.full(p.r.shape[1], LONG["max_sweeps"])))
    emu = T.emu_solve(g32, r32, p.h0, **STOP)
    out["stop"] = (emu, T.solve(p.g, p.r, p.h0, STOP["tol"], STOP["max_sweeps"], counts=emu.counts))
    return out


def floor_of(c, run):
    emu, ref = emulated(c)[run]
    return T.deviation(c, emu.x, ref, np.inf)[0]


def slack_of(c):
    """The largest difference between the emulation's and the float64 d_s, on the scale at which the rule decides --
    max(d_s, tol xmax_s) of the reference: a difference far below the threshold cannot change a decision -- and between the
    xmax_s, relative to the reference's."""
    emu, ref = emulated(c)["stop"]
    tol = STOP["tol"]
    p = T.problem(c)
    some = (np.abs(p.r).max(axis=0) > 0)[None, :]      # (a zero right-hand side: checked against its exact trajectory, no slack needed)
    with np.errstate(all="ignore"):
        dd = np.abs(emu.d - ref.d) / np.maximum(ref.d, tol * ref.xmax)
        dx = np.abs(emu.xmax - ref.xmax) / ref.xmax
    dd, dx = dd[some & np.isfinite(dd)], dx[some & np.isfinite(dx)]
    return float(max(np.max(dd, initial=0.0), np.max(dx, initial=0.0)))


@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_emulation_defines_the_bar(c):
    """In either run the emulation's largest deviation from the float64 reference is within the floor of the table and the bar
    is 10 x that floor, and the case's stop-rule difference is within the slack's floor (NMFX_WRITE_HALS_BARS=<file>: append
    the figures instead, to rebuild the table)."""
    floors, slack = {run: floor_of(c, run) for run in ("long", "stop")}, slack_of(c)
    path = os.environ.get("NMFX_WRITE_HALS_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": T.case_id(c), "long": floors["long"], "stop": floors["stop"], "slack": slack}) + "\n")
        return
    row = T.BARS[T.case_id(c)]
    for run, table_floor, bar in (("long", row[0], row[1]), ("stop", row[2], row[3])):
        floor = floors[run]
        assert bar == pytest.approx(10 * table_floor, rel=1e-12) and bar == T.bar_of(c, run)
        assert floor <= table_floor, f"{T.case_id(c)} {run}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
        assert floor >= table_floor / 2, f"{T.case_id(c)} {run}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"
    assert slack <= T.SLACK_FLOOR, f"{T.case_id(c)}: stop-rule difference {slack:.3e} above the slack's floor {T.SLACK_FLOOR:.3e}"


def test_the_slack_is_ten_times_the_largest_difference():
    worst = max(slack_of(c) for c in T.CASES)
    assert T.SLACK == pytest.approx(10 * T.SLACK_FLOOR, rel=1e-12)
    assert T.SLACK_FLOOR / 2 <= worst <= T.SLACK_FLOOR, (worst, T.SLACK_FLOOR)
    assert T.SLACK < 0.5


def test_the_table_has_every_case_and_no_other():
    assert sorted(T.BARS) == sorted(T.IDS)


def test_the_cases_are_the_ones_the_issue_sets():
    ids = set(T.IDS)
    for kind in ("sparse", "masked"):
        assert {f"{kind}-base-k{k}-scaled" for k in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64)} <= ids
        assert {f"{kind}-rowsT-k8-scaled", f"{kind}-rowsT-k40-scaled", f"{kind}-1x300-k4-scaled", f"{kind}-300x1-k4-scaled",
                f"{kind}-5x4-k4-scaled", f"{kind}-tallT-k8-scaled"} <= ids
        assert {f"{kind}-base-k40-{rg}" for rg in ("cold", "settled", "dead")} <= ids
    assert {"sparse-base-k65-scaled", "sparse-base-k128-scaled", "masked-full-k8-scaled"} <= ids
    lams = {T.lam_of(c) for c in T.CASES}
    assert 0.0 in lams and any(l > 0 for l in lams)
    counts = T.problem(T.Case("masked", "rowsT", 8, "scaled")).nobs
    assert tuple(counts[:8]) == (1, 3, 4, 5, 255, 256, 257, 513)            # the transposed rows are the columns' problems
    assert tuple(T.problem(T.Case("sparse", "rowsT", 8, "scaled")).nobs[:5]) == (1, 255, 256, 257, 513)
    assert T.problem(T.Case("sparse", "tallT", 8, "scaled")).r.shape[1] == 20000
    p = T.problem(T.Case("masked", "base", 16, "scaled"))
    assert p.lam == 0 and p.deficient.mean() > 0.5                             # no unique minimiser: compared by objective
    assert not T.problem(T.Case("masked", "base", 17, "scaled")).deficient.any()      # lambda_h > 0


def test_exact_reference_passes():
    for c in (T.Case("masked", "base", 16, "scaled"), T.Case("sparse", "base", 8, "scaled")):
        ref = emulated(c)["long"][1]
        assert T.deviation(c, ref.x, ref, 0.0) == (0.0, None)


# ---- the stop-rule cases are not vacuous ----------------------------------------------------------------------------------------
def test_stop_rule_cases_are_not_vacuous():
    """On the float64 reference alone: at tol = 1e-3 and a cap of 8, columns stop at 1, between 2 and 7, and at the cap."""
    at1 = mid = cap = 0
    for c in T.CASES:
        p = T.problem(c)
        counts = T.solve(p.g, p.r, p.h0, **STOP).counts
        at1 += int((counts == 1).sum()); mid += int(((counts >= 2) & (counts <= 7)).sum()); cap += int((counts == STOP["max_sweeps"]).sum())
        print(f"{T.case_id(c)}: sweeps 1..8 -> {np.bincount(counts, minlength=9)[1:].tolist()}")
    assert at1 > 0 and mid > 0 and cap > 0, (at1, mid, cap)
    for kind in ("sparse", "masked"):                     # ... and within single cases of either kind
        p = T.problem(T.Case(kind, "base", 40, "settled"))
        counts = T.solve(p.g, p.r, p.h0, **STOP).counts
        assert ((counts >= 2) & (counts <= 7)).any() and ((counts == 1).any() or (counts == 8).any()), np.bincount(counts)


def test_the_float64_stop_rule_passes_its_own_check():
    for c in (T.Case("sparse", "base", 40, "settled"), T.Case("masked", "base", 40, "cold")):
        p = T.problem(c)
        counts = T.solve(p.g, p.r, p.h0, **STOP).counts
        assert T.stop_failures(c, counts, STOP["tol"], STOP["max_sweeps"], 0.0)[0] == []


# ---- planted faults -------------------------------------------------------------------------------------------------------------
def test_fault_shared_gram_on_a_masked_case():
    c = T.Case("masked", "base", 8, "scaled")
    p = T.problem(c)
    bad = T.solve(T.systems_f32(c, shared=True)[0].astype(np.float64), p.r, p.h0, **LONG)
    worst, msg = T.deviation(c, bad.x, emulated(c)["long"][1], T.bar_of(c, "long"), "shared")
    assert msg and "problem " in msg and worst > T.bar_of(c, "long")


@pytest.mark.parametrize("c", [T.Case("masked", "base", 8, "scaled"), T.Case("sparse", "base", 8, "scaled")], ids=T.case_id)
def test_fault_two_lambda_left_out(c):
    p = T.problem(c)
    assert p.lam > 0
    g = p.g - 2 * p.lam * np.eye(c.k)
    bad = T.solve(g, p.r, p.h0, **LONG)
    worst, msg = T.deviation(c, bad.x, emulated(c)["long"][1], T.bar_of(c, "long"), "no lambda")
    assert msg and worst > T.bar_of(c, "long")


@pytest.mark.parametrize("c", [T.Case("masked", "base", 40, "settled"), T.Case("sparse", "base", 40, "settled")], ids=T.case_id)
def test_fault_stop_rule_on_the_first_sweeps_step(c):
    p = T.problem(c)
    bad = T.solve(p.g, p.r, p.h0, first_step=True, **STOP)
    fails, _ = T.stop_failures(c, bad.counts, STOP["tol"], STOP["max_sweeps"], T.SLACK)
    assert fails and "went on to" in fails[0]


@pytest.mark.parametrize("off", [1, -1])
def test_fault_count_off_by_one(off):
    c = T.Case("sparse", "base", 40, "settled")
    p = T.problem(c)
    good = T.solve(p.g, p.r, p.h0, **STOP).counts
    bad = np.clip(good + off, 1, STOP["max_sweeps"])
    assert (bad != good).any()
    fails, _ = T.stop_failures(c, bad, STOP["tol"], STOP["max_sweeps"], T.SLACK)
    assert fails


def test_fault_residual_never_refreshed():
    """40 sweeps in the cold regime on the residual of the start: on the unmasked case the drift of the kept residual is over
    the bar (emulated: 9.7e-3 never refreshed, 5.3e-4 refreshed every 16 sweeps, bar 6.7e-3).  On the masked cold case the
    drift is measurable but within the bar (3.8e-4 never refreshed, 6.2e-5 refreshed, bar 7.8e-4): a value bar of ten times the
    emulation does not see a missing refresh there, and this test says so rather than claim it."""
    c = T.Case("sparse", "base", 40, "cold")
    p = T.problem(c)
    bar = T.bar_of(c, "long")
    bad = T.emu_solve(*T.systems_f32(c), p.h0, refresh=None, **LONG)
    worst, msg = T.deviation(c, bad.x, emulated(c)["long"][1], bar, "never refreshed")
    print(f"{T.case_id(c)}: never refreshed {worst:.3e}, bar {bar:.1e}")
    assert msg and worst > bar
    c = T.Case("masked", "base", 40, "cold")
    p = T.problem(c)
    bad = T.emu_solve(*T.systems_f32(c), p.h0, refresh=None, **LONG)
    drift = T.deviation(c, bad.x, emulated(c)["long"][1], np.inf)[0]
    print(f"{T.case_id(c)}: never refreshed {drift:.3e}, refreshed {floor_of(c, 'long'):.3e}, bar {T.bar_of(c, 'long'):.1e}")
    assert drift > 3 * floor_of(c, "long")
