"""Every half-step of sparse HALS on the device, problem by problem, against the float64 sweep, and every recorded objective
against nmf_amd.sparse.objective of the device's iterates (tests/sparse_hals_step.py has the cases, the comparator and the
bars; tests/test_hals_sparse_step_bars.py proves them on the CPU)."""
import numpy as np
import pytest

import sparse_hals_step as SH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", SH.CASES, ids=[SH.case_id(c) for c in SH.CASES])
def test_every_half_step_and_objective(c):
    """1 and 2 iterations with the stop rule off from the case's start: W1, H1, W2, H2 within the case's bar on every problem,
    obj[0 .. s] within 1e-9 of the float64 objective of the iterates, padded components and clamps exact."""
    runs = SH.run_case(c)
    for s, run in runs.items():
        assert run.w.shape == (SH.matrix(c.matrix).shape[0], c.k) and (run.w >= 0).all() and (run.h >= 0).all()
        assert len(run.objectives) == s + 1
    if c.regime == "dead":
        for run in runs.values():
            assert (run.w[:, SH.DEAD] == 0).all() and (run.h[SH.DEAD] == 0).all()


def test_a_continued_run_is_the_run_in_one_call():
    """Iterations 0 and 1 in two calls give the bits of one call of two (the Grams of the stats launches carry over)."""
    from nmf_amd.engine import Engine
    c = SH.Case("base", 40, "scaled", 1)
    x = SH.matrix(c.matrix)
    w0, h0 = SH.start(c)
    out = []
    with Engine.for_sparse(x, c.k) as eng:
        for calls in ((2,), (1, 1)):
            eng.set_factors(w0, h0)
            done = 0
            for n in calls:
                eng.hals_sparse_run(0.05, 0.02, 1, SH.NEVER, 0, 0, done, n)
                done += n
            eng.hals_sparse_finish(SH.NEVER, 0, 0, done)
            out.append((*eng.get_factors(), eng.objectives(0, 3)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
