"""Every half-step of masked HALS on the device, problem by problem, against the batched float64 sweep (one Gram matrix per
problem), and every recorded objective against nmf_amd.masked.objective of the device's iterates (tests/masked_hals_step.py
has the cases, the comparator and the bars; tests/test_masked_hals_step_bars.py proves them on the CPU)."""
import numpy as np
import pytest

import anls_step as A
import hals_step as HS
import masked_hals_step as MH

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", MH.CASES, ids=[MH.case_id(c) for c in MH.CASES])
def test_every_half_step_and_objective(c):
    """1 and 2 iterations with the stop rule off from the case's start: W1, H1, W2, H2 within the case's bar on every problem,
    obj[0 .. s] within 1e-9 of the float64 objective of the iterates, dead components and clamps exact."""
    runs = MH.run_case(c)
    x, _ = MH.matrix(c.matrix)
    for s, run in runs.items():
        assert run.w.shape == (x.shape[0], c.k) and run.h.shape == (c.k, x.shape[1]) and (run.w >= 0).all() and (run.h >= 0).all()
        assert len(run.objectives) == s + 1
    if c.regime == "dead":
        for run in runs.values():
            assert (run.w[:, MH.DEAD] == 0).all() and (run.h[MH.DEAD] == 0).all()


@pytest.mark.parametrize("k", [3, 40])
def test_padded_components_are_exact_zeros(k):
    """get_factors returns the k components only, so the padding (kp = 4 / 64) is checked through what it would do: a run with k
    components equals, bit for bit, a run of the padded width whose extra components start at zero -- and those, dead
    components with lambda = 0, are exact zeros after two iterations."""
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    c = MH.Case("base", k, "scaled", 1)
    x, mask = MH.matrix("base")
    w0, h0 = MH.start(c)
    kp = 4 if k <= 4 else 64
    out = []
    for kk in (k, kp):
        wp, hp = np.zeros((w0.shape[0], kk)), np.zeros((kk, h0.shape[1]))
        wp[:, :k], hp[:k] = w0, h0
        with Engine.for_sparse(masked.observed(x, mask, kk), kk, masked=True) as eng:
            eng.set_factors(wp, hp)
            eng.hals_masked_run(0.0, 0.0, 1, MH.NEVER, 0, 0, 0, 2)
            w, h = eng.get_factors()
            out.append((w, h, eng.objectives(0, 3)))
    (w, h, obj), (wp, hp, objp) = out
    assert (wp[:, k:] == 0).all() and (hp[k:] == 0).all()
    assert np.array_equal(w, wp[:, :k]) and np.array_equal(h, hp[:k]) and np.array_equal(obj, objp)


def test_all_ones_mask_is_unmasked_hals():
    """The `full` case against hals_step's shared-Gram float64 reference, at the same bar."""
    c = MH.Case("full", 8, "scaled", 1)
    x, _ = MH.matrix("full")
    v = x.astype(np.float64)
    w0, h0 = MH.start(c)
    lw, lh = MH.lam_of(c)
    runs = MH.run_hals_masked("full", w0, h0, lw, lh, 1)
    fails = []
    for label, f, b, lam, xdev, prev in A.half_steps(v, w0, h0, runs, lw, lh):
        g, r = A.gram_rhs(f, b, lam)
        xref, numer = HS.sweep(g, r, prev, 1)
        worst, msg, _ = HS.values(f"full-shared {label}", r, xdev, xref, numer, MH.bar_of(c))
        print(f"{label}: worst deviation from the shared-Gram sweep {worst:.3e}")
        if msg:
            fails.append(msg)
    assert not fails, "\n".join(fails)


def test_a_continued_run_is_the_run_in_one_call():
    """Iterations 0 and 1 in two calls give the bits of one call of two."""
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    c = MH.Case("base", 40, "scaled", 1)
    x, mask = MH.matrix(c.matrix)
    w0, h0 = MH.start(c)
    out = []
    with Engine.for_sparse(masked.observed(x, mask, c.k), c.k, masked=True) as eng:
        for calls in ((2,), (1, 1)):
            eng.set_factors(w0, h0)
            done = 0
            for n in calls:
                eng.hals_masked_run(0.05, 0.02, 1, MH.NEVER, 0, 0, done, n)
                done += n
            eng.hals_masked_finish(MH.NEVER, 0, 0, done)
            out.append((*eng.get_factors(), eng.objectives(0, 3)))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
