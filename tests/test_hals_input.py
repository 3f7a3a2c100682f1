"""The input rules of nmf_amd.hals.hals: every refusal is raised before any device work (these tests run without a GPU: a call
that got as far as the device would raise `no HIP device`), with its type and the start of its message, and leaves the
caller's array as it was."""
import numpy as np
import pytest
import scipy.sparse as sp

from nmf_amd import _lib as L
from nmf_amd.hals import Experiment, hals
from nmf_amd.nmf import NMF


def data():
    return np.random.default_rng(3).uniform(0.1, 1.0, (12, 9))


REFUSALS = [
    (dict(distance_type="is"), ValueError, "hals: distance_type='is'"),
    (dict(distance_type="beta"), ValueError, "hals: distance_type='beta'"),
    (dict(distance_type="xx"), KeyError, "'Distance type unknown"),
    (dict(k=0), ValueError, "hals: supports 1 <= k <= 128 components"),
    (dict(k=-3), ValueError, "hals: supports 1 <= k <= 128 components"),
    (dict(k=129), ValueError, "hals: supports 1 <= k <= 128 components"),
    (dict(k=2.5), ValueError, "hals: supports 1 <= k <= 128 components"),
    (dict(sweeps=0), ValueError, "hals: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=17), ValueError, "hals: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=1.5), ValueError, "hals: sweeps must be an integer between 1 and 16"),
    (dict(sweeps=True), ValueError, "hals: sweeps must be an integer between 1 and 16"),
    (dict(lambda_w=-0.1), ValueError, "hals: lambda_w must be non-negative"),
    (dict(lambda_h=-1e-9), ValueError, "hals: lambda_h must be non-negative"),
    (dict(lambda_h=float("nan")), ValueError, "hals: lambda_h must be non-negative"),
    (dict(mask=np.ones((12, 9), bool)), TypeError, "hals() got an unexpected keyword argument 'mask'"),
    (dict(weights=np.ones((12, 9))), TypeError, "hals() got an unexpected keyword argument 'weights'"),
]


@pytest.mark.parametrize("kw,exc,start", REFUSALS, ids=[f"{i}-{next(iter(r[0]))}" for i, r in enumerate(REFUSALS)])
def test_refusals(kw, exc, start):
    x = data()
    keep = x.copy()
    args = dict(k=3)
    args.update(kw)
    with pytest.raises(exc) as e:
        hals(x, **args)
    assert str(e.value).startswith(start), str(e.value)
    assert "no HIP device" not in str(e.value)
    assert np.array_equal(x, keep)


@pytest.mark.parametrize("fmt", ["csr_matrix", "csc_matrix", "coo_matrix"])
def test_sparse_input_is_refused(fmt):
    x = getattr(sp, fmt)(data())
    with pytest.raises(TypeError) as e:
        hals(x, 3)
    assert "hals" in str(e.value) and "no HIP device" not in str(e.value)


def test_refusals_come_before_the_random_start():
    """A refused call draws nothing from the global generator: the next seeded start is the one the caller expects."""
    np.random.seed(11)
    want = np.random.rand(4)
    np.random.seed(11)
    with pytest.raises(ValueError):
        hals(data(), 3, sweeps=0, nndsvd_init=(False, "zero"))
    assert np.array_equal(np.random.rand(4), want)


def test_nmf_factorize_knows_hals():
    with pytest.raises(ValueError, match="hals: sweeps"):
        NMF(data(), 3).factorize("hals", sweeps=0)
    with pytest.raises(Exception, match="^Method not known") as e:
        NMF(data(), 3).factorize("hals2")
    assert "hals" in str(e.value)


def test_experiment_and_abi_table():
    assert Experiment._fields == ("method", "components", "distance_type", "nndsvd_init", "max_iter", "tol1", "tol2", "lambda_w",
                                  "lambda_h", "sweeps")
    assert "nmfx_hals_run" in L.SIGNATURES
    lib = L.load()
    assert lib.nmfx_version() >= 380 and hasattr(lib, "nmfx_hals_run")
