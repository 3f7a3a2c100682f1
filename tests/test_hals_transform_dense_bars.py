"""The bars of the dense HALS fold-in checks (tests/hals_transform_dense_step.py), proven on the CPU: the float32 emulation of
the kernel's form (kept residual, refresh every 16 sweeps, the stop rule in f32) on the products as the device forms them
defines each case's value bars and the slack of the stop rule, planted faults are caught, and the cases are the ones the checks
are meant to have."""
import functools
import json
import os

import numpy as np
import pytest

import hals_step as HS
import hals_transform_dense_step as D
import hals_transform_step as T

LONG, STOP = D.LONG, D.STOP


@functools.lru_cache(maxsize=None)
def emulated(c):
    """The emulation's two runs of a case with the float64 reference of each (the STOP reference run for the emulation's own
    counts): {'long': (emu, ref), 'stop': (emu, ref)}."""
    p = D.problem(c)
    g32, r32 = D.systems_f32(c)
    out = {"long": (T.emu_solve(g32, r32, p.h0, **LONG), D.reference(c, "long"))}
    emu = T.emu_solve(g32, r32, p.h0, **STOP)
    out["stop"] = (emu, D.reference(c, "stop", counts=emu.counts))
    return out


def floor_of(c, run):
    emu, ref = emulated(c)[run]
    return D.deviation(c, emu.x, ref, np.inf)[0]


def slack_of(c):
    """The largest difference between the emulation's and the float64 d_s, on the scale at which the rule decides --
    max(d_s, tol xmax_s) of the reference -- and between the xmax_s, relative to the reference's
    (tests/test_hals_transform_bars.py::slack_of)."""
    emu, ref = emulated(c)["stop"]
    tol = STOP["tol"]
    with np.errstate(all="ignore"):
        dd = np.abs(emu.d - ref.d) / np.maximum(ref.d, tol * ref.xmax)
        dx = np.abs(emu.xmax - ref.xmax) / ref.xmax
    dd, dx = dd[np.isfinite(dd)], dx[np.isfinite(dx)]
    return float(max(np.max(dd, initial=0.0), np.max(dx, initial=0.0)))


@pytest.mark.parametrize("c", D.CASES, ids=D.IDS)
def test_emulation_defines_the_bar(c):
    """In either run the emulation's largest deviation from the float64 reference is within the floor of the table and the bar
    is 10 x that floor, and the case's stop-rule difference is within the slack's floor (NMFX_WRITE_HALS_BARS=<file>: append
    the figures instead, to rebuild the table)."""
    floors, slack = {run: floor_of(c, run) for run in ("long", "stop")}, slack_of(c)
    path = os.environ.get("NMFX_WRITE_HALS_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": D.case_id(c), "long": floors["long"], "stop": floors["stop"], "slack": slack}) + "\n")
        return
    row = D.BARS[D.case_id(c)]
    for run, table_floor, bar in (("long", row[0], row[1]), ("stop", row[2], row[3])):
        floor = floors[run]
        assert bar == pytest.approx(10 * table_floor, rel=1e-12) and bar == D.bar_of(c, run)
        assert floor <= table_floor, f"{D.case_id(c)} {run}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
        assert floor >= table_floor / 2, f"{D.case_id(c)} {run}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"
    assert slack <= D.SLACK_FLOOR, f"{D.case_id(c)}: stop-rule difference {slack:.3e} above the slack's floor {D.SLACK_FLOOR:.3e}"


def test_the_slack_is_ten_times_the_largest_difference():
    worst = max(slack_of(c) for c in D.CASES)
    assert D.SLACK == pytest.approx(10 * D.SLACK_FLOOR, rel=1e-12)
    assert D.SLACK_FLOOR / 2 <= worst <= D.SLACK_FLOOR, (worst, D.SLACK_FLOOR)
    assert D.SLACK < 0.5


def test_the_table_has_every_case_and_no_other():
    assert sorted(D.BARS) == sorted(D.IDS)


def test_the_cases_are_the_ones_the_issue_sets():
    ids = set(D.IDS)
    assert {f"cold-257x200-k{k}-f32" for k in (1, 2, 15, 16, 17, 32)} <= ids
    assert {f"mixed-257x200-k{k}-{a}" for k in (33, 64, 65, 128) for a in ("f32", "bf16")} <= ids
    assert {f"{rg}-257x200-k40-bf16" for rg in ("settled", "cold", "dead")} <= ids
    assert {"mixed-1x257-k4-f32", "mixed-257x1-k4-f32", "mixed-5x4-k4-f32", "mixed-61x127-k33-bf16", "mixed-70x4200-k33-bf16"} <= ids
    assert len(ids) == 22
    assert max(c.n for c in D.CASES) > HS.wrap_stride()                           # more columns than one round of the grid
    lams = {D.problem(c).lam for c in D.CASES}
    assert 0.0 in lams and any(l > 0 for l in lams)
    for c in D.CASES:                                                              # w and h0 are what the device will hold
        p = D.problem(c)
        assert np.array_equal(p.w, p.w.astype(np.float32).astype(np.float64)) and (p.w >= 0).all() and np.isfinite(p.w).all()
        assert np.array_equal(p.h0, p.h0.astype(np.float32).astype(np.float64)) and p.w.shape == (c.m, c.k) and p.h0.shape == (c.k, c.n)
        assert (np.abs(p.r).max(axis=0) > 0).all()                                # no column with a zero right-hand side
    dead = D.problem(D.Case("dead", 257, 200, 40, "bf16"))
    assert dead.lam == 0 and np.diag(dead.g)[3] == 0 and (np.diag(dead.g) > 0).sum() == 39      # G_33 = 0: a dead component


def test_exact_reference_passes():
    for c in (D.Case("mixed", 257, 200, 64, "bf16"), D.Case("cold", 257, 200, 17, "f32")):
        ref = emulated(c)["long"][1]
        assert D.deviation(c, ref.x, ref, 0.0) == (0.0, None)


def test_strictly_clamped_zeros_exist_and_must_be_exact():
    """The mixed and the cold cases hold reference zeros with a dual beyond STRICT; one of them at 1e-30 is an infinite deviation."""
    for c in (D.Case("mixed", 257, 200, 64, "bf16"), D.Case("cold", 257, 200, 40, "bf16")):
        p = D.problem(c)
        ref = emulated(c)["long"][1]
        strict = (ref.x == 0) & (ref.numer < -HS.STRICT * np.abs(p.r).max(axis=0)[None, :])
        assert strict.sum() > 50, (D.case_id(c), int(strict.sum()))
        big = (ref.x == 0) & (-ref.numer > 100 * D.bar_of(c, "long") * ref.x.max(axis=0)[None, :] * np.diag(p.g)[:, None]) & strict
        i, q = np.argwhere(big)[0]
        x = ref.x.copy()
        x[i, q] = 1e-30
        worst, msg = D.deviation(c, x, ref, D.bar_of(c, "long"), "strict")
        assert worst == np.inf and f"problem {q}, variable {i}" in msg and "must be exactly 0" in msg


# ---- the stop-rule cases are not vacuous ----------------------------------------------------------------------------------------
def test_stop_rule_cases_are_not_vacuous():
    """On the float64 reference alone: at tol = 1e-3 and a cap of 8, columns stop early (after 2 or 3 sweeps; from these starts
    no column stops after its first), between 4 and 7, and at the cap -- and so within single cases."""
    early = mid = cap = 0
    for c in D.CASES:
        counts = D.reference(c, "stop").counts
        early += int((counts <= 3).sum()); mid += int(((counts >= 4) & (counts <= 7)).sum()); cap += int((counts == STOP["max_sweeps"]).sum())
        print(f"{D.case_id(c)}: sweeps 1..8 -> {np.bincount(counts, minlength=9)[1:].tolist()}")
    assert early > 0 and mid > 0 and cap > 0, (early, mid, cap)
    for c in (D.Case("settled", 257, 200, 40, "bf16"), D.Case("mixed", 70, 4200, 33, "bf16")):
        counts = D.reference(c, "stop").counts
        assert (counts <= 3).any() and ((counts >= 4) & (counts <= 7)).any() and (counts == 8).any(), np.bincount(counts)


def test_the_float64_stop_rule_passes_its_own_check():
    for c in (D.Case("settled", 257, 200, 40, "bf16"), D.Case("cold", 257, 200, 40, "bf16")):
        counts = D.reference(c, "stop").counts
        assert D.stop_failures(c, counts, STOP["tol"], STOP["max_sweeps"], 0.0)[0] == []


# ---- planted faults -------------------------------------------------------------------------------------------------------------
LAMBDA_CASES = [c for c in D.CASES if D.problem(c).lam > 0 and (c.m, c.n) == (257, 200)]


def test_fault_two_lambda_left_out():
    """The sweep on G without 2 lambda I: over the long bar on every 257 x 200 case with lambda_h > 0 but those this test names."""
    assert len(LAMBDA_CASES) >= 3
    seen, blind = [], []
    for c in LAMBDA_CASES:
        p = D.problem(c)
        bad = T.solve(p.g - 2 * p.lam * np.eye(c.k), p.r, p.h0, 0.0, LONG["max_sweeps"], counts=np.full(c.n, LONG["max_sweeps"]))
        bar = D.bar_of(c, "long")
        worst, msg = D.deviation(c, bad.x, emulated(c)["long"][1], bar, "no lambda")
        print(f"{D.case_id(c)}: 2 lambda left out {worst:.3e}, bar {bar:.1e}")
        (seen if msg and worst > bar else blind).append(D.case_id(c))
    assert seen and not blind, f"the long bar does not see a missing 2 lambda on {blind}"


STOP_FAULT_CASES = [D.Case("cold", 257, 200, 40, "bf16"), D.Case("mixed", 70, 4200, 33, "bf16")]


@pytest.mark.parametrize("c", STOP_FAULT_CASES + [D.Case("settled", 257, 200, 40, "bf16")], ids=D.case_id)
def test_fault_stop_rule_on_the_first_sweeps_step(c):
    p = D.problem(c)
    bad = T.solve(p.g, p.r, p.h0, first_step=True, **STOP)
    fails, _ = D.stop_failures(c, bad.counts, STOP["tol"], STOP["max_sweeps"], D.SLACK)
    assert fails and "went on to" in fails[0]


@pytest.mark.parametrize("off", [1, -1])
@pytest.mark.parametrize("c", STOP_FAULT_CASES, ids=D.case_id)
def test_fault_count_off_by_one(c, off):
    good = D.reference(c, "stop").counts
    bad = np.clip(good + off, 1, STOP["max_sweeps"])
    assert (bad != good).any()
    fails, _ = D.stop_failures(c, bad, STOP["tol"], STOP["max_sweeps"], D.SLACK)
    assert any(("went on to" if off > 0 else "stopped after") in f for f in fails), fails


def test_a_count_one_too_many_is_not_seen_where_the_sweeps_contract_slowly():
    """The slack of 0.49 lets a column run one sweep too many as long as the sweep that should have been its last moved it by
    more than 0.51 tol xmax.  In the settled regime a sweep shrinks the step by less than that on every column that stops
    before the cap, so counts that are all one too high pass there: the rule sees that fault on the cold and the mixed cases
    above, not here, and this test says so rather than claim it.  One too few is seen here too."""
    c = D.Case("settled", 257, 200, 40, "bf16")
    good = D.reference(c, "stop").counts
    assert (good < STOP["max_sweeps"]).sum() > 100
    assert D.stop_failures(c, np.clip(good + 1, 1, STOP["max_sweeps"]), STOP["tol"], STOP["max_sweeps"], D.SLACK)[0] == []
    assert D.stop_failures(c, np.clip(good - 1, 1, STOP["max_sweeps"]), STOP["tol"], STOP["max_sweeps"], D.SLACK)[0]


@pytest.mark.parametrize("c", [D.Case("mixed", 257, 200, 33, "bf16"), D.Case("mixed", 70, 4200, 33, "bf16"),
                               D.Case("cold", 257, 200, 16, "f32")], ids=D.case_id)
def test_fault_rhs_of_the_neighbouring_column(c):
    """Every column solved on the right-hand side of the next one (a stride fault): rejected, and the message names a column."""
    p = D.problem(c)
    bad = T.solve(p.g, np.roll(p.r, -1, axis=1), p.h0, 0.0, LONG["max_sweeps"], counts=np.full(c.n, LONG["max_sweeps"]))
    bar = D.bar_of(c, "long")
    worst, msg = D.deviation(c, bad.x, emulated(c)["long"][1], bar, "neighbour")
    assert msg and "problem " in msg and worst > bar


def test_fault_residual_never_refreshed_is_not_seen_by_a_value_bar():
    """40 sweeps on the residual of the start, never formed anew, in the cold regime (and on every other case).  On the sparse
    fold-in's cold case this drift is over the bar (tests/test_hals_transform_bars.py).  On the dense cases it is not even
    distinguishable from the refreshed emulation (cold-257x200-k40-bf16: 8.11e-5 never refreshed, 8.03e-5 refreshed, bar
    1.1e-3): these solves contract, the steps shrink sweep by sweep and the kept residual stops gathering rounding long before
    sweep 16.  A value bar does not see a missing refresh here, and this test says so rather than claim it; that the refresh
    runs at all (r reloaded from the right column, the mat-vec redone) is what the 40-sweep device run checks, since a refresh
    from a wrong right-hand side is the stride fault above."""
    seen = []
    for c in D.CASES:
        p = D.problem(c)
        bar = D.bar_of(c, "long")
        bad = T.emu_solve(*D.systems_f32(c), p.h0, refresh=None, **LONG)
        drift, msg = D.deviation(c, bad.x, emulated(c)["long"][1], bar, "never refreshed")
        print(f"{D.case_id(c)}: never refreshed {drift:.3e}, refreshed {floor_of(c, 'long'):.3e}, bar {bar:.1e}")
        if msg:
            seen.append(D.case_id(c))
        assert drift <= 2 * floor_of(c, "long")
    assert seen == []
