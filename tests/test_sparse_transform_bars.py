"""The bars of the sparse MUR fold-in checks (tests/sparse_transform_step.py), proven on the CPU: a float32 emulation of the
kernels' form defines each case's value bars and the slack of the count check, the emulation's own counts stay within half the
share of columns that may differ from the float64 count, and planted faults are caught -- or, where one is not, the test says so."""
import functools
import json
import os

import numpy as np
import pytest

import sparse_transform_step as T

STOP = T.STOP
NEAR = (0.5, 2.0)            # "near 1": the float64 ratios delta / (tol xmax) that a rounding difference could carry across 1


@functools.lru_cache(maxsize=None)
def emulated(c):
    """The emulation's runs of a case with the float64 run of each: {1: (emu, ref), 3: ..., 25: ..., 'stop': (emu, ref at the
    emulation's own counts)}."""
    out = {}
    for steps in T.FIXED_STEPS:
        out[steps] = (T.emu_solve(c, 0.0, steps), T.solve(c, 0.0, steps, counts=np.full(T.N, steps)))
    emu = T.emu_solve(c, **STOP)
    out["stop"] = (emu, T.solve(c, STOP["tol"], STOP["max_iter"], counts=emu.counts))
    return out


@functools.lru_cache(maxsize=None)
def reference(c):
    return T.solve(c, **STOP)


def floor_of(c, run):
    runs = T.FIXED_STEPS if run == "fixed" else ("stop",)
    return max(float(T.deviation(emulated(c)[r][0].h, emulated(c)[r][1].h).max()) for r in runs)


def slack_of(c):
    """The largest relative difference between the emulation's and the float64 delta_u / (tol xmax_u) where the float64 ratio is
    near 1, over the steps both trajectories have."""
    emu, ref = emulated(c)["stop"]
    re_, rr = T.ratios(emu, STOP["tol"]), T.ratios(ref, STOP["tol"])
    with np.errstate(all="ignore"):
        near = (rr >= NEAR[0]) & (rr <= NEAR[1]) & np.isfinite(re_)
        diff = np.abs(re_ - rr) / rr
    return float(np.max(diff[near], initial=0.0))


@pytest.mark.parametrize("c", T.CASES, ids=T.IDS)
def test_emulation_defines_the_bars(c):
    """The emulation's largest deviation from the float64 definition is within the floor of the table and the bar is 10 x that
    floor, for the runs at tol = 0 and for the run to the stop rule; the case's ratio difference is within the slack's floor; and
    the emulation's counts differ from the float64 counts in at most half of the columns that may (NMFX_WRITE_SPT_BARS=<file>:
    append the figures instead, to rebuild the table)."""
    floors, slack = {run: floor_of(c, run) for run in ("fixed", "stop")}, slack_of(c)
    off = int((emulated(c)["stop"][0].counts != reference(c).counts).sum())
    path = os.environ.get("NMFX_WRITE_SPT_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": T.case_id(c), "fixed": floors["fixed"], "stop": floors["stop"], "slack": slack, "off": off,
                                 "counts": reference(c).counts.tolist()}) + "\n")
        return
    row = T.BARS[T.case_id(c)]
    for run, table_floor, bar in (("fixed", row[0], row[1]), ("stop", row[2], row[3])):
        floor = floors[run]
        assert bar == pytest.approx(10 * table_floor, rel=1e-12) and bar == T.bar_of(c, run)
        assert floor <= table_floor, f"{T.case_id(c)} {run}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
        assert floor >= table_floor / 2, f"{T.case_id(c)} {run}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"
    assert slack <= T.SLACK_FLOOR, f"{T.case_id(c)}: ratio difference {slack:.3e} above the slack's floor {T.SLACK_FLOOR:.3e}"
    assert 2 * off <= T.limit(T.N), f"{T.case_id(c)}: the emulation alone differs from the float64 count in {off} columns"
    emu, at = emulated(c)["stop"]
    fails, _ = T.count_failures(c, emu.counts, STOP["tol"], STOP["max_iter"], T.SLACK, ref=reference(c), at=at)
    assert not fails, "\n".join(fails)


def test_the_slack_is_ten_times_the_largest_difference():
    worst = max(slack_of(c) for c in T.CASES)
    assert T.SLACK == pytest.approx(10 * T.SLACK_FLOOR, rel=1e-12)
    assert T.SLACK_FLOOR / 2 <= worst <= T.SLACK_FLOOR, (worst, T.SLACK_FLOOR)
    assert T.SLACK < 0.5


def test_the_table_has_every_case_and_no_other():
    assert sorted(T.BARS) == sorted(T.IDS)


def test_the_cases_are_the_ones_the_issue_sets():
    assert {(c.handle, c.loss) for c in T.CASES} == set(T.PAIRS) and len(T.PAIRS) == 5
    for pair in T.PAIRS:
        mine = [c for c in T.CASES if (c.handle, c.loss) == pair]
        assert sorted(c.k for c in mine) == [1, 3, 5, 16, 17, 40, 64, 100, 130]
        assert {T.kp_of(c.k) for c in mine} == {4, 8, 16, 32, 64, 128, 256}
        assert {c.lam for c in mine} == {0.0, 0.5} and {c.fmt for c in mine} == {"f64", "f32", "alt"}
    for c in T.CASES:
        p = T.problem(c)
        shape = p.x.shape
        assert shape[0] <= 600 and shape[1] <= 24
        assert tuple(p.lens[:5]) == (0, 1, 256, 257, 520)
        assert not p.w[T.ZERO_ROW].any() and all(T.ZERO_ROW in p.rows[j, :p.lens[j]] for j in (2, 3, 4))
        if c.handle == "masked" and c.loss != "is":
            assert (p.xv[5, :p.lens[5]] == 0).sum() == 1                      # the observed zero is an entry
        if c.loss == "is":
            assert (p.xv[p.ok] > 0).all()


def test_stop_rule_cases_are_not_vacuous():
    """On the float64 definition alone: columns stop after few steps, after many, and at the cap."""
    few = many = cap = 0
    for c in T.CASES:
        counts = reference(c).counts
        few += int((counts <= 10).sum()); many += int(((counts > 50) & (counts < STOP["max_iter"])).sum()); cap += int((counts == STOP["max_iter"]).sum())
        print(f"{T.case_id(c)}: steps min {counts.min()} mean {counts.mean():.0f} max {counts.max()}")
    assert few > 0 and many > 0 and cap > 0, (few, many, cap)


def test_the_float64_run_passes_its_own_checks():
    for c in (T.CASES[4], T.CASES[22], T.CASES[40]):
        ref = reference(c)
        assert T.count_failures(c, ref.counts, STOP["tol"], STOP["max_iter"], 0.0, ref=ref)[0] == []
        assert T.value_failures(c, ref.h, ref.h, 0.0, "itself") == (0.0, [])


def test_an_empty_column_goes_to_zero_in_two_steps():
    """The definition on a column without entries: a = 0, so step 1 takes every component to 0 (delta_1 > 0 = tol xmax_1) and step
    2 moves nothing: the count is 2, or 1 under a cap of 1."""
    for c in (T.CASES[3], T.CASES[14], T.CASES[21], T.CASES[30], T.CASES[41]):
        ref = reference(c)
        assert T.problem(c).lens[0] == 0 and ref.counts[0] == 2 and not ref.h[:, 0].any()
        assert T.solve(c, 0.0, 1).counts[0] == 1
        emu = emulated(c)["stop"][0]
        assert emu.counts[0] == 2 and not emu.h[:, 0].any()


# ---- planted faults -------------------------------------------------------------------------------------------------------------
def _values_caught(c, fault, run="fixed"):
    """(worst deviation of the faulty float64 run of 25 steps, the case's bar)."""
    bad = T.solve(c, 0.0, 25, counts=np.full(T.N, 25), fault=fault)
    worst, msgs = T.value_failures(c, bad.h, emulated(c)[25][1].h, T.bar_of(c, run), fault)
    return worst, T.bar_of(c, run), msgs


def _case(handle, loss, k):
    return next(c for c in T.CASES if (c.handle, c.loss, c.k) == (handle, loss, k))


@pytest.mark.parametrize("loss", ["eu", "kl"])
def test_fault_unmasked_statistics_on_a_masked_case(loss):
    worst, bar, msgs = _values_caught(_case("masked", loss, 16), "unmasked_stats")
    assert msgs and worst > bar


@pytest.mark.parametrize("pair", T.PAIRS, ids="-".join)
def test_fault_lambda_left_out(pair):
    c = next(c for c in T.CASES if (c.handle, c.loss) == pair and c.lam > 0 and c.k >= 16)
    worst, bar, msgs = _values_caught(c, "no_lambda")
    assert msgs and worst > bar


@pytest.mark.parametrize("pair", T.PAIRS, ids="-".join)
def test_fault_last_piece_dropped(pair):
    c = next(c for c in T.CASES if (c.handle, c.loss) == pair and c.k == 40)
    bad = T.solve(c, 0.0, 25, counts=np.full(T.N, 25), fault="drop_last_piece")
    dev = T.deviation(bad.h, emulated(c)[25][1].h)
    hit = np.nonzero(dev > T.bar_of(c, "fixed"))[0].tolist()
    if pair == ("sparse", "eu") or pair == ("sparse", "kl"):
        assert 4 in hit or 3 in hit, (hit, dev[[3, 4]])
    assert set(hit) <= {3, 4} and hit, (hit, dev[[3, 4]])                     # (the 257- and the 520-entry column lose 1 and 8 entries)


@pytest.mark.parametrize("pair", [("masked", "eu"), ("masked", "is"), ("sparse", "kl"), ("masked", "kl")], ids="-".join)
def test_fault_fixed_sum_hoisted_from_h0(pair):
    """The q-dependent sums formed once, from h0, and kept."""
    c = next(c for c in T.CASES if (c.handle, c.loss) == pair and c.k == 17)
    worst, bar, msgs = _values_caught(c, "hoist_from_h0")
    assert msgs and worst > bar


def _count_fault(c, bad_counts):
    fails, _ = T.count_failures(c, bad_counts, STOP["tol"], STOP["max_iter"], T.SLACK, ref=reference(c))
    return fails


def test_fault_stop_rule_on_the_previous_delta():
    """Testing step t against delta_{t-1} stops every column one step late.  The ratio delta / (tol xmax) of a multiplicative
    update falls slowly, by less than the slack per step on many columns, so the per-column condition cannot see one step there:
    the case is caught by the share of columns whose count differs from the float64 count, and the test prints how many columns
    the per-column condition caught."""
    caught_by_ratio = 0
    for c in (_case("sparse", "kl", 16), _case("masked", "eu", 40), _case("masked", "is", 17)):
        bad = T.solve(c, fault="previous_delta", **STOP)
        ref = reference(c)
        moved = bad.counts != ref.counts
        assert moved.sum() > T.limit(T.N)
        fails = _count_fault(c, bad.counts)
        assert fails and any("another count than the float64 run" in f for f in fails)
        n = sum("went on to" in f for f in fails)
        caught_by_ratio += n
        print(f"{T.case_id(c)}: {int(moved.sum())} columns one step late; the ratio condition names {n} of them (slack {T.SLACK:.3f})")
    print(f"per-column ratio condition: {caught_by_ratio} messages in all")


@pytest.mark.parametrize("off", [1, -1])
def test_fault_count_off_by_one(off):
    """As above: every column off by one is over the share that may differ; whether the ratio condition also names a column
    depends on how fast its ratio falls, and is printed."""
    for c in (_case("sparse", "kl", 16), _case("masked", "kl", 40)):
        ref = reference(c)
        bad = np.clip(ref.counts + off, 1, STOP["max_iter"])
        assert (bad != ref.counts).sum() > T.limit(T.N)
        fails = _count_fault(c, bad)
        assert fails and any("another count than the float64 run" in f for f in fails)
        word = "went on to" if off > 0 else "stopped after"
        print(f"{T.case_id(c)} off by {off:+d}: the ratio condition names {sum(word in f for f in fails)} columns (slack {T.SLACK:.3f})")
    # a single column off by one: caught only where its ratio moves by more than the slack in one step
    c = _case("sparse", "eu", 1)
    ref = reference(c)
    bad = ref.counts.copy()
    bad[1] += off
    if 1 <= bad[1] <= STOP["max_iter"]:
        fails = _count_fault(c, bad)
        print(f"{T.case_id(c)} column 1 alone off by {off:+d}: {'caught' if fails else 'NOT caught at this slack'}")
        assert fails                                                          # (k = 1 converges in one step: the ratio jumps)
