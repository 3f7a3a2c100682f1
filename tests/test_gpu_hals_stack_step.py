"""Every half-step of stacked HALS on the device, problem by problem, against the float64 masked sweep, and every recorded
objective against the float64 objective of the device's iterate of that problem (tests/hals_stack_step.py).

The shapes are the smallest at which the stacked form of hals_sweep_kernel and the objective kernels (csrc/kernels_hals.hip) can
go wrong: one stack at each padded width, a problem across the lane-64 boundary of KP = 128, components that belong to no
problem, a stack of one, a different lambda for every problem, a dead component inside a problem, three sweeps on the kept
residual, a single row and a single column, more problems than one round of the grid."""
import numpy as np
import pytest

import hals_stack_step as ST
from mur_step import NEVER

pytestmark = pytest.mark.gpu


def cases(*names):
    return pytest.mark.parametrize("c", [ST.BY_NAME[n] for n in names], ids=list(names))


@cases("kp16", "kp32", "kp64", "kp128", "lane64", "lambdas", "sweeps3", "row", "col", "tall", "wide")
def test_half_steps_and_objectives(c):
    ST.run_case(c)


@cases("tail")
def test_unowned_tail_components_stay_zero(c):
    _, _, runs = ST.run_case(c)
    for s, run in runs.items():
        assert not run.w[:, sum(c.ks):].any() and not run.h[sum(c.ks):].any(), f"{s}-step run"


@cases("dead")
def test_dead_component_keeps_its_zeros(c):
    _, _, runs = ST.run_case(c)
    p, j = c.dead
    for s, run in runs.items():
        w, h = run.parts[p]
        assert not w[:, j].any() and not h[j].any(), f"{s}-step run"
        assert w[:, j - 1].any() and h[j - 1].any()


@cases("one")
def test_stack_of_one_against_hals_run(c):
    """The same handle, the same start: nmfx_hals_run and a stack of one.  Within the bar; bit-identity is reported."""
    from nmf_amd.engine import Engine
    v, starts, runs = ST.run_case(c)
    (lw, lh), = c.lams
    with Engine(c.m, c.n, c.k_handle) as eng:
        eng.upload_v(v)
        eng.set_factors(*starts[0])
        eng.hals_run(lw, lh, c.sweeps, NEVER, 0, 0, 0, 2)
        w, h = eng.get_factors()
    same = np.array_equal(w, runs[2].w) and np.array_equal(h, runs[2].h)
    print(f"stack of one against hals_run: factors bit-identical: {same}")
    for name, a, b in (("W", w, runs[2].w), ("H", h, runs[2].h)):
        assert np.abs(a - b).max() <= ST.bar_of(c) * max(a.max(), 1e-30), name


def test_get_factors_slices_the_stack():
    c = ST.BY_NAME["kp32"]
    v, starts = ST.make_case(c)
    runs, _ = ST.run_stack(v, c.ks, starts, c.lams, steps=(1,))
    off = ST.offsets(c.ks)
    for p, (w, h) in enumerate(runs[1].parts):
        assert np.array_equal(w, runs[1].w[:, off[p]:off[p + 1]]) and np.array_equal(h, runs[1].h[off[p]:off[p + 1]])
