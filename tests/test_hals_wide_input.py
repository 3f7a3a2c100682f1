"""The input rules of nmf_amd.hals.hals_wide: every refusal is raised before any device work (these tests run without a GPU: a
call that got as far as the device would raise `no HIP device`) and before any RNG draw, with its type and the start of its
message, and leaves the caller's array as it was.  `hals` itself keeps its own rules."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd import hals as H
from nmf_amd.hals import hals, hals_wide
from nmf_amd.nmf import NMF

RANGE = "hals_wide: supports 129 <= k <= 1024 components"


def data():
    return np.random.default_rng(3).uniform(0.1, 1.0, (12, 9))


REFUSALS = [
    (dict(distance_type="is"), ValueError, "hals_wide: distance_type='is'"),
    (dict(distance_type="beta"), ValueError, "hals_wide: distance_type='beta'"),
    (dict(distance_type="xx"), KeyError, "'Distance type unknown"),
    (dict(k=0), ValueError, RANGE),
    (dict(k=-3), ValueError, RANGE),
    (dict(k=1025), ValueError, RANGE),
    (dict(k=4096), ValueError, RANGE),
    (dict(k=200.0), ValueError, RANGE),
    (dict(k=True), ValueError, RANGE),
    (dict(k=None), ValueError, RANGE),
    (dict(sweeps=0), ValueError, "hals_wide: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=17), ValueError, "hals_wide: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=1.5), ValueError, "hals_wide: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=True), ValueError, "hals_wide: sweeps must be an integer between 1 and 16"),
    (dict(lambda_w=-0.1), ValueError, "hals_wide: lambda_w must be non-negative"),
    (dict(lambda_h=-1e-9), ValueError, "hals_wide: lambda_h must be non-negative"),
    (dict(lambda_h=float("nan")), ValueError, "hals_wide: lambda_h must be non-negative"),
    (dict(mask=np.ones((12, 9), bool)), TypeError, "hals_wide() got an unexpected keyword argument 'mask'"),
    (dict(weights=np.ones((12, 9))), TypeError, "hals_wide() got an unexpected keyword argument 'weights'"),
]


@pytest.mark.parametrize("kw,exc,start", REFUSALS, ids=[f"{i}-{next(iter(r[0]))}" for i, r in enumerate(REFUSALS)])
def test_refusals(kw, exc, start):
    x = data()
    keep = x.copy()
    args = dict(k=200)
    args.update(kw)
    with pytest.raises(exc) as e:
        hals_wide(x, **args)
    assert str(e.value).startswith(start), str(e.value)
    assert "no HIP device" not in str(e.value)
    assert np.array_equal(x, keep)


@pytest.mark.parametrize("k", [1, 64, 128])
def test_a_rank_of_hals_names_hals(k):
    with pytest.raises(ValueError) as e:
        hals_wide(data(), k)
    assert str(e.value).startswith(RANGE) and f"(got k = {k})" in str(e.value) and "hals runs 1 <= k <= 128" in str(e.value)
    with pytest.raises(ValueError) as e:
        hals_wide(data(), 1025)
    assert "hals runs" not in str(e.value)


@pytest.mark.parametrize("fmt", ["csr_matrix", "csc_matrix", "coo_matrix"])
def test_sparse_input_is_refused(fmt):
    x = getattr(sp, fmt)(data())
    with pytest.raises(TypeError) as e:
        hals_wide(x, 200)
    assert str(e.value).startswith("hals_wide: takes dense data only") and "hals_sparse" in str(e.value)
    with pytest.raises(TypeError):                       # (the type of the data comes before the rank)
        hals_wide(x, 3)


@pytest.mark.parametrize("kw", [dict(k=128), dict(k=1025), dict(sweeps=0), dict(lambda_w=-1), dict(distance_type="is")])
def test_refusals_come_before_the_random_start(kw):
    """A refused call draws nothing from the global generator: the next seeded start is the one the caller expects."""
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    args = dict(k=200, nndsvd_init=(False, "zero"))
    args.update(kw)
    with pytest.raises(ValueError):
        hals_wide(data(), **args)
    assert np.array_equal(np.random.rand(4), want)
    np.random.seed(11)
    with pytest.raises(TypeError):
        hals_wide(sp.csr_matrix(data()), 200, nndsvd_init=(False, "zero"))
    assert np.array_equal(np.random.rand(4), want)


def test_hals_keeps_its_own_range():
    with pytest.raises(ValueError) as e:
        hals(data(), 129)
    assert str(e.value).startswith("hals: supports 1 <= k <= 128 components (got k = 129)")
    assert H.MAX_K == 128 and H.MAX_K_WIDE == 1024 and H.MAX_SWEEPS == 16


def test_signature_is_that_of_hals():
    a, b = inspect.signature(hals), inspect.signature(hals_wide)
    assert list(a.parameters) == list(b.parameters)
    assert all(a.parameters[p].default == b.parameters[p].default and a.parameters[p].kind == b.parameters[p].kind for p in a.parameters)


def test_nmf_factorize_routes_by_rank():
    """Dense, unmasked data: k > 128 goes to hals_wide (its wording), k <= 128 stays with hals; masks and sparse data stay where
    they were, whatever the rank."""
    with pytest.raises(ValueError, match="^hals_wide: sweeps"):
        NMF(data(), 200).factorize("hals", sweeps=0)
    with pytest.raises(ValueError, match="^hals_wide: supports 129 <= k <= 1024"):
        NMF(data(), 2000).factorize("hals")
    with pytest.raises(ValueError, match="^hals: sweeps"):
        NMF(data(), 128).factorize("hals", sweeps=0)
    with pytest.raises(ValueError, match="^hals: supports 1 <= k <= 128"):
        NMF(data(), 0).factorize("hals")
    with pytest.raises(ValueError, match="^hals_sparse: supports 1 <= k <= 128"):
        NMF(sp.csr_matrix(data()), 200).factorize("hals")
    with pytest.raises(ValueError, match="^hals_masked: "):
        NMF(data(), 200).factorize("hals", mask=np.ones((12, 9), bool))


def test_abi_table():
    assert L.SIGNATURES["nmfx_hals_wide_run"] == L.SIGNATURES["nmfx_hals_run"]
    lib = L.load()
    assert lib.nmfx_version() >= 396 and hasattr(lib, "nmfx_hals_wide_run")
    from nmf_amd.engine import Engine
    assert callable(Engine.hals_wide_run)
