"""Every HALS half-step of the device beyond 128 components, problem by problem, against the float64 sweep
(tests/hals_wide_step.py; nmfx_hals_wide_run, hals_wide_sweep_kernel in csrc/kernels_hals.hip).

W_1, H_1, W_2, H_2 are each checked against the float64 projected Gauss-Seidel sweep fed the device's own previous iterate, on
every problem, and every recorded objective against the float64 objective of the device's iterates.  The kernel streams G through
LDS in row tiles: the ranks stand at every kp it is instantiated for, with a last tile (129) and a last slot (257) that are almost
all padding; the shapes leave waves of a block without a problem (1, 64 and 8 q + 1 problems) and take the blocks through a
second trip; three sweeps stream G again on the kept residual."""
import numpy as np
import pytest

import anls_step as A
import hals_step as HS
import hals_wide_step as HW

pytestmark = pytest.mark.gpu


def cases(pred):
    sel = [c for c in HW.CASES if pred(c)]
    return pytest.mark.parametrize("c", sel, ids=[HW.case_id(c) for c in sel])


def plain(c):
    return c.sweeps == 1 and (c.m, c.n) == (257, 200)


# ---- ranks: every kp, every tile height -------------------------------------------------------------------------------------------
@cases(lambda c: plain(c) and c.regime == "mixed")
def test_ranks(c):
    HW.run_case(c)


# ---- regimes ----------------------------------------------------------------------------------------------------------------------
@cases(lambda c: plain(c) and c.regime in ("settled", "cold", "dead"))
def test_regimes(c):
    out = HW.run_case(c)
    if c.regime == "dead":                               # G_33 = 0 in every half-step: the component keeps its zeros
        for s, run in out["eu"].items():
            assert not run.w[:, 3].any() and not run.h[3].any(), f"{HW.case_id(c)}: dead variable 3 moved in the {s}-step run"


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
@cases(lambda c: c.sweeps == 1 and (c.m, c.n) != (257, 200) and max(c.m, c.n) <= HW.wrap_stride())
def test_shapes(c):
    HW.run_case(c)


# ---- more problems than one round of the grid ----------------------------------------------------------------------------------------
@cases(lambda c: max(c.m, c.n) > 600)
def test_grid_wraps(c):
    assert max(c.m, c.n) > HW.wrap_stride()              # (256 CUs: the blocks of the long side take a second trip, most waves idle in it)
    HW.run_case(c, kinds=("eu",))


# ---- further sweeps on the kept residual ---------------------------------------------------------------------------------------------
@cases(lambda c: c.sweeps == 3)
def test_three_sweeps(c):
    HW.run_case(c, kinds=("eu",))


# ---- determinism: no atomics ---------------------------------------------------------------------------------------------------------
@cases(lambda c: plain(c) and c.regime == "mixed" and c.k in (200, 640) and c.arith == "bf16")
def test_two_runs_bit_identical(c):
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = HW.lam_of(c)
    a, _ = HW.run_hals_wide(v, w0, h0, lw, lh, steps=(2,))
    b, _ = HW.run_hals_wide(v, w0, h0, lw, lh, steps=(2,))
    for x, y, name in zip(a[2], b[2], ("W2", "H2", "objective history")):
        assert np.array_equal(x, y), f"{name}: {int(np.sum(x != y))} elements differ between two identical runs"


# ---- the entry guard: HALS's family ----------------------------------------------------------------------------------------------------
T = (HS.NEVER, 1e-3, 1e-3)


def _handle(k=200, regime="cold"):
    from nmf_amd.engine import Engine
    v, w0, h0 = A.make_case(regime, 257, 200, k)
    eng = Engine(257, 200, k)
    eng.upload_v(v)
    eng.set_factors(w0, h0)
    return eng


@pytest.mark.parametrize("k", [200, 384])
def test_two_calls_equal_one(k):
    with _handle(k) as a:
        a.hals_wide_run(0.0, 0.01, 1, *T, 0, 1)
        a.hals_wide_run(0.0, 0.01, 1, *T, 1, 1)
        got = a.get_factors()
    with _handle(k) as b:
        b.hals_wide_run(0.0, 0.01, 1, *T, 0, 2)
        want = b.get_factors()
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)


def test_anls_and_hals_wide_do_not_continue_each_other():
    """As every other pair of solver families (tests/test_gpu_hals_step.py): refused until the factors are read back and set again."""
    from nmf_amd._lib import NmfxError
    with _handle() as e:
        e.hals_wide_run(0.0, 0.0, 1, *T, 0, 1)
        with pytest.raises(NmfxError, match="another solver"):
            e.anls_run(0.0, 0.0, *T, 1, 1)
        e.hals_wide_run(0.0, 0.0, 1, *T, 1, 1)           # (the refusal changed nothing the run depends on)
        w, h = e.get_factors()
        e.set_factors(w, h)
        e.anls_run(0.0, 0.0, *T, 0, 1)
        with pytest.raises(NmfxError, match="another solver"):
            e.hals_wide_run(0.0, 0.0, 1, *T, 1, 1)
    with _handle() as ref:
        ref.hals_wide_run(0.0, 0.0, 1, *T, 0, 2)
        np.testing.assert_array_equal(ref.get_factors()[0], w)


def test_a_fired_stop_rule_keeps_the_iterate():
    """st->flag set: the sweep returns at once, in front of its first barrier, and the pair stays."""
    with _handle(200, "settled") as e:
        e.hals_wide_run(0.0, 0.0, 1, 0, 1e30, 1e30, 0, 3)       # (tol1 = 1e30: the rule fires at the first index past min_iter = 0)
        flag, stop_i, _ = e.state()[:3]
        assert flag != 0, "the stop rule did not fire"
        kept = e.get_factors()
        e.hals_wide_run(0.0, 0.0, 1, 0, 1e30, 1e30, 3, 2)
        for x, y in zip(kept, e.get_factors()):
            np.testing.assert_array_equal(x, y)


def test_c_abi_refusals():
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    lib = L.load()
    assert lib.nmfx_version() >= 396
    with _handle() as e:
        for args, word in (((0.0, 0.0, 0) + T + (0, 1), b"sweeps"), ((0.0, 0.0, 17) + T + (0, 1), b"sweeps"),
                           ((-1.0, 0.0, 1) + T + (0, 1), b"lambda"), ((0.0, -1.0, 1) + T + (0, 1), b"lambda"),
                           ((0.0, 0.0, 1) + T + (-1, 1), b"range"), ((0.0, 0.0, 1) + T + (0, -1), b"range")):
            assert lib.nmfx_hals_wide_run(e.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(e.h), args
            assert b"nmfx_hals_wide_run" in lib.nmfx_last_error(e.h)
        before = e.get_factors()
        # nmfx_hals_run keeps its own refusal and wording beyond 128 components
        assert lib.nmfx_hals_run(e.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG
        assert lib.nmfx_last_error(e.h) == b"nmfx_hals_run: not available with more than 128 components in this build"
        for x, y in zip(before, e.get_factors()):        # (nothing was launched)
            np.testing.assert_array_equal(x, y)
        e.hals_wide_run(0.0, 0.0, 1, *T, 0, 1)           # (a refused call joins no family and leaves the handle usable)
    with _handle(40) as e:                               # (weights exist up to 128 components only: their refusal stands in front of the rank's)
        e.upload_weights(np.ones((257, 200), dtype=np.float32))
        assert lib.nmfx_hals_wide_run(e.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"weights" in lib.nmfx_last_error(e.h)
        e.clear_weights()
        assert lib.nmfx_hals_wide_run(e.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"nmfx_hals_run" in lib.nmfx_last_error(e.h)
    rng = np.random.default_rng(0)
    for k, word in ((128, b"nmfx_hals_run"), (40, b"nmfx_hals_run"), (1025, b"1024")):
        with Engine(40, 30, k) as eng:
            eng.upload_v(rng.uniform(0.1, 1, (40, 30)).astype(np.float32))
            w0, h0 = rng.uniform(0.1, 1, (40, k)), rng.uniform(0.1, 1, (k, 30))
            eng.set_factors(w0, h0)
            assert lib.nmfx_hals_wide_run(eng.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and word in lib.nmfx_last_error(eng.h), k
            w, h = eng.get_factors()
            assert np.array_equal(w, A.f32(w0)) and np.array_equal(h, A.f32(h0))
    import scipy.sparse as sp
    from nmf_amd import sparse
    xs = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 200)
    with Engine.for_sparse(xs, 200) as se:
        assert lib.nmfx_hals_wide_run(se.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(se.h)
