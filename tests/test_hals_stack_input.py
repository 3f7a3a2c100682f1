"""The input rules of nmf_amd.hals.hals_stack and of factorize_grid(..., 'hals'): every refusal is raised before any device work
(these tests run without a GPU: a call that got as far as the device would raise `no HIP device`) and before any draw from the
global generator, with its type and the start of its message, and leaves the caller's array as it was."""
import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd import grid
from nmf_amd.hals import hals_stack


def data():
    return np.random.default_rng(3).uniform(0.1, 1.0, (12, 9))


P = [dict(k=3), dict(k=2, lambda_w=0.1)]
REFUSALS = [
    (dict(problems=[]), ValueError, "hals_stack: problems is empty"),
    (dict(problems=()), ValueError, "hals_stack: problems is empty"),
    (dict(problems=5), ValueError, "hals_stack: problems must be a non-empty sequence of dicts"),
    (dict(problems=[3]), ValueError, "hals_stack: problem 0 is not a dict"),
    (dict(problems=[dict(k=3), dict(lambda_w=0.1)]), ValueError, "hals_stack: problem 1 has no k"),
    (dict(problems=[dict(k=2.5)]), ValueError, "hals_stack: problem 0 needs an integer k >= 1"),
    (dict(problems=[dict(k=True)]), ValueError, "hals_stack: problem 0 needs an integer k >= 1"),
    (dict(problems=[dict(k="3")]), ValueError, "hals_stack: problem 0 needs an integer k >= 1"),
    (dict(problems=[dict(k=3), dict(k=0)]), ValueError, "hals_stack: problem 1 needs an integer k >= 1"),
    (dict(problems=[dict(k=-2)]), ValueError, "hals_stack: problem 0 needs an integer k >= 1"),
    (dict(problems=[dict(k=64), dict(k=64), dict(k=1)]), ValueError, "hals_stack: the problems hold 129 components together"),
    (dict(problems=[dict(k=129)]), ValueError, "hals_stack: the problems hold 129 components together"),
    (dict(problems=[dict(k=3, lambda_w=-0.1)]), ValueError, "hals_stack: problem 0: lambda_w must be non-negative"),
    (dict(problems=[dict(k=3), dict(k=3, lambda_h=float("nan"))]), ValueError, "hals_stack: problem 1: lambda_h must be non-negative"),
    (dict(problems=[dict(k=3, lambda_h=None)]), ValueError, "hals_stack: problem 0: lambda_h must be non-negative"),
    (dict(problems=[dict(k=3, rho=1.0)]), ValueError, "hals_stack: problem 0 has the unknown key 'rho'"),
    (dict(problems=[dict(k=3, distance_type="eu")]), ValueError, "hals_stack: problem 0 has the unknown key 'distance_type'"),
    (dict(sweeps=0), ValueError, "hals_stack: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=17), ValueError, "hals_stack: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=1.5), ValueError, "hals_stack: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=True), ValueError, "hals_stack: sweeps must be an integer between 1 and 16"),
    (dict(distance_type="kl"), TypeError, "hals_stack() got an unexpected keyword argument 'distance_type'"),
]


@pytest.mark.parametrize("kw,exc,start", REFUSALS, ids=[f"{i}-{next(iter(r[0]))}" for i, r in enumerate(REFUSALS)])
def test_refusals(kw, exc, start):
    x = data()
    keep = x.copy()
    args = dict(problems=P, nndsvd_init=(False, "zero"))
    args.update(kw)
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(exc) as e:
        hals_stack(x, **args)
    assert str(e.value).startswith(start), str(e.value)
    assert "no HIP device" not in str(e.value)
    assert np.array_equal(x, keep)
    assert np.array_equal(np.random.rand(4), want), "a refused call drew from the global generator"


@pytest.mark.parametrize("fmt", ["csr_matrix", "csc_matrix", "coo_matrix"])
def test_sparse_input_is_refused(fmt):
    x = getattr(sp, fmt)(data())
    with pytest.raises(TypeError) as e:
        hals_stack(x, P)
    assert "hals_stack" in str(e.value) and "no HIP device" not in str(e.value)


def test_abi_table():
    names = ["nmfx_hals_stack_set", "nmfx_hals_stack_terms", "nmfx_hals_stack_run", "nmfx_hals_stack_finish", "nmfx_hals_stack_get_state",
             "nmfx_hals_stack_get_objectives", "nmfx_hals_stack_get_factors"]
    assert all(n in L.SIGNATURES for n in names)
    lib = L.load()
    assert lib.nmfx_version() >= 390 and all(hasattr(lib, n) for n in names)


# ---- factorize_grid(v, 'hals', ...) up to the first device call ---------------------------------------------------------------
class Reached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    made = []

    def engine(m, n, k, device=0):
        made.append((m, n, k))
        raise Reached()
    monkeypatch.setattr(grid, "Engine", engine)
    return made


GRID_REFUSALS = [
    (dict(features=(3, 129)), ValueError, "hals: supports 1 <= k <= 128 components"),
    (dict(features=(3,), sweeps=0), ValueError, "hals: sweeps must be an integer between 1 and 16"),
    (dict(features=(3,), lambda_w=(0.0, -1.0)), ValueError, "hals: lambda_w must be non-negative"),
    (dict(features=(3,), distance_type="is"), ValueError, "hals: distance_type='is'"),
    (dict(features=(3,), distance_type="beta"), ValueError, "hals: distance_type='beta'"),
    (dict(features=(3,), mask=np.ones((12, 9), bool)), TypeError, "factorize_grid: mask= is not supported"),
]


@pytest.mark.parametrize("kw,exc,start", GRID_REFUSALS, ids=[str(i) for i in range(len(GRID_REFUSALS))])
def test_grid_refusals_come_before_any_engine(kw, exc, start, no_device):
    x = data()
    keep = x.copy()
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(exc) as e:
        grid.factorize_grid(x, "hals", **kw)
    assert str(e.value).startswith(start), str(e.value)
    assert no_device == [] and np.array_equal(x, keep) and np.array_equal(np.random.rand(4), want)


def test_grid_keeps_one_k128_engine_for_the_stacks(no_device):
    with pytest.raises(Reached):
        grid.factorize_grid(data(), "hals", features=(3, 5), lambda_h=(0, 0.1), nndsvd_init=(False, "zero"))
    assert no_device == [(12, 9, 128)]


@pytest.mark.parametrize("kw", [dict(distance_type="kl"), dict()], ids=["kl", "NMFX_GRID_PAIR=0"])
def test_grid_without_stacking_runs_each_combination_on_its_own_engine(kw, no_device, monkeypatch):
    if not kw:
        monkeypatch.setenv("NMFX_GRID_PAIR", "0")
    with pytest.raises(Reached):
        grid.factorize_grid(data(), "hals", features=(3, 5), lambda_h=(0, 0.1), nndsvd_init=(False, "zero"), **kw)
    assert no_device == [(12, 9, 3)]


def test_stacks_are_packed_greedily_in_the_legacy_order():
    combos = [(k, lw, lh) for k in (60, 50, 30) for lw in (0,) for lh in (0, 0.1)]
    assert grid._hals_stacks(combos, 128) == [[0, 1], [2, 3], [4, 5]]
    combos = [(k, 0, 0) for k in range(2, 16)]
    assert sum(k for k, _, _ in combos) == 119 and grid._hals_stacks(combos, 128) == [list(range(14))]
    assert grid._hals_stacks([(128, 0, 0), (1, 0, 0), (127, 0, 0), (2, 0, 0)], 128) == [[0], [1, 2], [3]]
