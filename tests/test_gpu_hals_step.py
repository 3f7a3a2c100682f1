"""Every HALS half-step of the device, problem by problem, against the float64 sweep (tests/hals_step.py).

W_1, H_1, W_2, H_2 are each checked against the float64 projected Gauss-Seidel sweep fed the device's own previous iterate, on
every problem, and every recorded objective against the float64 objective of the device's iterates.  The shapes are the
smallest at which hals_sweep_kernel (csrc/kernels_hals.hip) can go wrong: every padding edge of k (16, 32, 64, 128, the second
variable per lane from 65 on), problem counts of 8 q + 1, single rows and columns, more problems than one round of the grid,
more than one sweep on the kept residual."""
import numpy as np
import pytest

import anls_step as A
import hals_step as HS

pytestmark = pytest.mark.gpu


def cases(pred):
    sel = [c for c in HS.CASES if pred(c)]
    return pytest.mark.parametrize("c", sel, ids=[HS.case_id(c) for c in sel])


def plain(c):
    return c.sweeps == 1 and (c.m, c.n) == (257, 200)


# ---- ranks at every padding edge ------------------------------------------------------------------------------------------------
@cases(lambda c: plain(c) and c.k <= 32)
def test_ranks_kp16_kp32(c):
    HS.run_case(c)


@cases(lambda c: plain(c) and c.regime == "mixed")
def test_ranks_kp64_kp128(c):
    HS.run_case(c)


# ---- regimes ----------------------------------------------------------------------------------------------------------------------
@cases(lambda c: plain(c) and c.k >= 40 and c.regime in ("settled", "cold", "dead"))
def test_regimes(c):
    out = HS.run_case(c)
    if c.regime == "dead":                               # G_33 = 0 in every half-step: the component keeps its zeros
        for s, run in out["eu"].items():
            assert not run.w[:, 3].any() and not run.h[3].any(), f"{HS.case_id(c)}: dead variable 3 moved in the {s}-step run"


# ---- shapes -------------------------------------------------------------------------------------------------------------------------
@cases(lambda c: c.sweeps == 1 and (c.m, c.n) != (257, 200) and max(c.m, c.n) <= HS.wrap_stride())
def test_shapes(c):
    HS.run_case(c)


# ---- more problems than one round of the grid ----------------------------------------------------------------------------------------
@cases(lambda c: max(c.m, c.n) > 600)
def test_grid_wraps(c):
    assert max(c.m, c.n) > HS.wrap_stride()              # (256 CUs: the blocks of the long side take a second round)
    HS.run_case(c, kinds=("eu",))


# ---- further sweeps on the kept residual ---------------------------------------------------------------------------------------------
@cases(lambda c: c.sweeps == 3)
def test_three_sweeps(c):
    HS.run_case(c, kinds=("eu",))


# ---- determinism: no atomics ---------------------------------------------------------------------------------------------------------
@cases(lambda c: plain(c) and c.regime == "mixed" and c.k in (64, 128) and c.arith == "bf16")
def test_two_runs_bit_identical(c):
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = HS.lam_of(c)
    a, _ = HS.run_hals(v, w0, h0, lw, lh, steps=(2,))
    b, _ = HS.run_hals(v, w0, h0, lw, lh, steps=(2,))
    for x, y, name in zip(a[2], b[2], ("W2", "H2", "objective history")):
        assert np.array_equal(x, y), f"{name}: {int(np.sum(x != y))} elements differ between two identical runs"


# ---- the entry guard: a solver family of its own -------------------------------------------------------------------------------------
T = (HS.NEVER, 1e-3, 1e-3)


def _handle(k=40):
    from nmf_amd.engine import Engine
    v, w0, h0 = A.make_case("cold", 257, 200, k)
    eng = Engine(257, 200, k)
    eng.upload_v(v)
    eng.set_factors(w0, h0)
    return eng


@pytest.mark.parametrize("k", [40, 100])
def test_two_calls_equal_one(k):
    with _handle(k) as a:
        a.hals_run(0.0, 0.01, 1, *T, 0, 2)
        a.hals_run(0.0, 0.01, 1, *T, 2, 3)
        got = a.get_factors()
    with _handle(k) as b:
        b.hals_run(0.0, 0.01, 1, *T, 0, 5)
        want = b.get_factors()
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)


def test_anls_and_hals_do_not_continue_each_other():
    """As every other pair of solver families (tests/test_gpu_mur.py): refused until the factors are read back and set again."""
    from nmf_amd._lib import NmfxError
    with _handle() as e:
        e.hals_run(0.0, 0.0, 1, *T, 0, 1)
        with pytest.raises(NmfxError, match="another solver"):
            e.anls_run(0.0, 0.0, *T, 1, 1)
        with pytest.raises(NmfxError, match="another solver"):
            e.mur_run(0, 0.0, 0.0, *T, 1, 1)
        e.hals_run(0.0, 0.0, 1, *T, 1, 1)                # (the refusals changed nothing the run depends on)
        w, h = e.get_factors()
        e.set_factors(w, h)
        e.anls_run(0.0, 0.0, *T, 0, 1)
        with pytest.raises(NmfxError, match="another solver"):
            e.hals_run(0.0, 0.0, 1, *T, 1, 1)
    with _handle() as ref:
        ref.hals_run(0.0, 0.0, 1, *T, 0, 2)
        np.testing.assert_array_equal(ref.get_factors()[0], w)


def test_c_abi_refusals():
    from nmf_amd import _lib as L
    lib = L.load()
    with _handle() as e:
        for args, word in (((0.0, 0.0, 0) + T + (0, 1), b"sweeps"), ((0.0, 0.0, 17) + T + (0, 1), b"sweeps"),
                           ((-1.0, 0.0, 1) + T + (0, 1), b"lambda"), ((0.0, -1.0, 1) + T + (0, 1), b"lambda"),
                           ((0.0, 0.0, 1) + T + (-1, 1), b"range"), ((0.0, 0.0, 1) + T + (0, -1), b"range")):
            assert lib.nmfx_hals_run(e.h, *args) == L.NMFX_E_ARG and word in lib.nmfx_last_error(e.h), args
        e.hals_run(0.0, 0.0, 1, *T, 0, 1)                # (a refused call joins no family and leaves the handle usable)
        e.upload_weights(np.ones((257, 200), dtype=np.float32))
        assert lib.nmfx_hals_run(e.h, 0.0, 0.0, 1, *T, 1, 1) == L.NMFX_E_ARG and b"weights" in lib.nmfx_last_error(e.h)
    from nmf_amd.engine import Engine
    rng = np.random.default_rng(0)
    with Engine(40, 30, 130) as big:                     # beyond 128 components: no generic path
        big.upload_v(rng.uniform(0.1, 1, (40, 30)).astype(np.float32))
        big.set_factors(rng.uniform(0.1, 1, (40, 130)), rng.uniform(0.1, 1, (130, 30)))
        assert lib.nmfx_hals_run(big.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"128" in lib.nmfx_last_error(big.h)
    import scipy.sparse as sp
    from nmf_amd import sparse
    xs = sparse.normalise(sp.random(64, 48, density=0.2, format="csr", random_state=0), 4)
    with Engine.for_sparse(xs, 4) as se:
        assert lib.nmfx_hals_run(se.h, 0.0, 0.0, 1, *T, 0, 1) == L.NMFX_E_ARG and b"sparse" in lib.nmfx_last_error(se.h)
