"""The float64 host objectives, bit for bit: masked.objective across its `chunk` boundaries, weighted.objective across its
1024-row block boundary and ard.objective on top of it, for every loss.  The expected values are float.hex() literals
recorded before the per-cell divergence was gathered into nmf_amd.losses.cells: blocking and summation order are part of
what these functions return, so the comparison is ==."""
import numpy as np
import pytest

BETAS = (-1.0, 0.0, 0.5, 1.0, 2.0, 3.0)
LOSSES = [("eu", None), ("kl", None), ("is", None)] + [("beta", b) for b in BETAS]


def zeros_allowed(loss, beta):
    return loss in ("eu", "kl") or (loss == "beta" and beta > 0)


def problem(m, n, k, seed, zeros):
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.05, 2.0, (m, n))
    w, h = rs.uniform(0.1, 1.0, (m, k)), rs.uniform(0.1, 1.0, (k, n))
    if zeros:
        x[rs.rand(m, n) < 0.2] = 0.0
    return rs, x, w, h


EXPECTED = {
    "masked eu": "0x1.d22ec0084c53ep+9",
    "masked kl": "0x1.12a2c37994a22p+10",
    "masked is": "0x1.6c60e06971864p+9",
    "weighted eu": "0x1.c6cd9d060bfdcp+13",
    "weighted kl": "0x1.513b59495547bp+14",
    "weighted is": "0x1.848b1e8ab8ac1p+14",
    "weighted beta -1": "0x1.6fa459e49eb2cp+15",
    "weighted beta 0": "0x1.848b1e8ab8ac1p+14",
    "weighted beta 0.5": "0x1.0cfc0beeddfa0p+15",
    "weighted beta 1": "0x1.513b59473380ep+14",
    "weighted beta 2": "0x1.c6cd9d060799fp+13",
    "weighted beta 3": "0x1.8d297a39ebd94p+13",
    "ard beta -1": "0x1.e6a4e34180674p+12",
    "ard beta 0": "0x1.1d52db70bfd46p+12",
    "ard beta 0.5": "0x1.9aec968bb1649p+12",
    "ard beta 1": "0x1.2ab254b4122dcp+12",
    "ard beta 2": "0x1.df05e549d0130p+11",
    "ard beta 3": "0x1.c7b6e8471a91ap+11",
    "ard-wt beta -1": "0x1.c5ade81329bb3p+15",
    "ard-wt beta 0": "0x1.be72088dda1ecp+14",
    "ard-wt beta 0.5": "0x1.3cf9f1c48e345p+15",
    "ard-wt beta 1": "0x1.9bb27abe0c7ebp+14",
    "ard-wt beta 2": "0x1.26a971849d93cp+14",
    "ard-wt beta 3": "0x1.0f44ce6a70127p+14",
}


def key(name, loss, beta):
    return f"{name} {loss}" + ("" if beta is None else f" {beta:g}")


def masked_value(loss):
    from nmf_amd import masked
    rs, x, w, h = problem(70, 50, 4, 11, zeros_allowed(loss, None))
    mask = rs.rand(70, 50) < 0.7
    x[~mask] = np.nan                                     # unobserved cells are never read
    return masked.objective(x, w, h, mask, loss, chunk=64)


def weighted_value(loss, beta):
    from nmf_amd import weighted
    rs, x, w, h = problem(1100, 7, 3, 12, zeros_allowed(loss, beta))
    om = 10.0 ** rs.uniform(-2.0, 2.0, x.shape)
    om[rs.rand(*x.shape) < 0.25] = 0.0
    x[om == 0] = np.nan                                   # cells of weight 0 are never read
    return weighted.objective(x, w, h, om, loss, beta=beta)


def ard_value(beta, with_weights):
    from nmf_amd import ard
    rs, x, w, h = problem(1100, 7, 3, 13, beta > 0)
    lam = rs.uniform(0.5, 2.0, 3)
    om = None
    if with_weights:
        om = 10.0 ** rs.uniform(-2.0, 2.0, x.shape)
        om[rs.rand(*x.shape) < 0.25] = 0.0
        x[om == 0] = np.nan
    return ard.objective(x, w, h, lam, beta, 0.7, 5.0, 1.3, weights=om)


@pytest.mark.parametrize("loss", ["eu", "kl", "is"])
def test_masked_objective(loss):
    assert float(masked_value(loss)).hex() == EXPECTED[key("masked", loss, None)]


@pytest.mark.parametrize("loss,beta", LOSSES)
def test_weighted_objective(loss, beta):
    assert float(weighted_value(loss, beta)).hex() == EXPECTED[key("weighted", loss, beta)]


@pytest.mark.parametrize("with_weights", [False, True])
@pytest.mark.parametrize("beta", BETAS)
def test_ard_objective(beta, with_weights):
    assert float(ard_value(beta, with_weights)).hex() == EXPECTED[key("ard-wt" if with_weights else "ard", "beta", beta)]
