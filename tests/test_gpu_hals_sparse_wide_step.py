"""Every half-step of sparse HALS with 129 .. 256 components on the device, problem by problem, against the float64 sweep, and
every recorded objective against nmf_amd.sparse.objective of the device's iterates (tests/sparse_hals_wide_step.py has the cases
and the bars; tests/test_hals_sparse_wide_step_bars.py proves them on the CPU)."""
import numpy as np
import pytest

import sparse_hals_wide_step as SW

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", SW.CASES, ids=[SW.case_id(c) for c in SW.CASES])
def test_every_half_step_and_objective(c):
    """1 and 2 iterations with the stop rule off from the case's start: W1, H1, W2, H2 within the case's bar on every problem,
    obj[0 .. s] within 1e-9 of the float64 objective of the iterates, padded components and clamps exact."""
    runs = SW.run_case(c)
    for s, run in runs.items():
        assert run.w.shape == (SW.matrix(c.matrix).shape[0], c.k) and (run.w >= 0).all() and (run.h >= 0).all()
        assert len(run.objectives) == s + 1
    if c.regime == "dead":
        for run in runs.values():
            assert (run.w[:, SW.DEAD] == 0).all() and (run.h[SW.DEAD] == 0).all()


def _run(eng, w0, h0, calls, lams=(0.05, 0.02)):
    eng.set_factors(w0, h0)
    done = 0
    for n in calls:
        eng.hals_sparse_wide_run(*lams, 1, SW.NEVER, 0, 0, done, n)
        done += n
    eng.hals_sparse_wide_finish(SW.NEVER, 0, 0, done)
    return (*eng.get_factors(), eng.objectives(0, done + 1))


def test_two_runs_give_the_same_bits():
    """The long row, the long column and every block partial are summed in a fixed order: no atomics anywhere."""
    from nmf_amd.engine import Engine
    c = SW.Case("base", 200, "scaled", 1)
    w0, h0 = SW.start(c)
    out = []
    for _ in range(2):
        with Engine.for_sparse(SW.matrix(c.matrix), c.k) as eng:
            out.append(_run(eng, w0, h0, (2,)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_a_continued_run_is_the_run_in_one_call():
    """first = 0, count = 1 and then first = 1, count = 1 give the bits of count = 2 (the Grams of the stats launches carry
    over; obj[0] is recorded by the first call only)."""
    from nmf_amd.engine import Engine
    c = SW.Case("base", 200, "scaled", 1)
    w0, h0 = SW.start(c)
    with Engine.for_sparse(SW.matrix(c.matrix), c.k) as eng:
        out = [_run(eng, w0, h0, calls) for calls in ((2,), (1, 1))]
    for a, b in zip(*out):
        assert np.array_equal(a, b)
