"""Inputs shared by tests/test_ard_input.py (CPU) and tests/test_gpu_ard.py."""
import numpy as np

from ard_ref import ard_default_b, ard_mur, ard_relevance

# the rank-recovery case: x is 120 x 90 of planted rank 3, K = 8
RANK = dict(m=120, n=90, rank=3, k=8, phi=0.1, a=5.0, iters=600)
GAP = 1e3            # smallest kept relevance / largest pruned relevance must stay above this


def planted(seed):
    """(planted rank 3) x gamma(20, 1 / 20) noise + 1e-3.  The planted factors are uniform with about half of their entries 0:
    with dense uniform factors the three components are nearly collinear and the float64 rule itself keeps a fourth one
    from some starts (seen at beta = 1.5, seed 1), which would make the case a test of the start rather than of the rule."""
    rs = np.random.RandomState(seed)
    m, n, r = RANK["m"], RANK["n"], RANK["rank"]
    w = rs.rand(m, r) * (rs.rand(m, r) < 0.5)
    h = rs.rand(r, n) * (rs.rand(r, n) < 0.5)
    return (w @ h) * rs.gamma(20.0, 1.0 / 20.0, (m, n)) + 1e-3


def rank_reference(beta, seed):
    """(x, b, the float64 run, its relevances): start factors from np.random.seed(seed), 600 iterations, stop rule off."""
    x = planted(seed)
    b = ard_default_b(x, RANK["k"], RANK["a"])
    np.random.seed(seed)
    out = ard_mur(x, RANK["k"], beta, RANK["phi"], RANK["a"], b, min_iter=RANK["iters"], max_iter=RANK["iters"])
    return x, b, out, ard_relevance(out.trace["lam"], x.shape, RANK["a"], b)


def kept_and_gap(rel, count=3):
    """(indices of the `count` largest relevances, sorted; smallest of them / largest of the rest, inf where the rest is 0)."""
    order = np.argsort(rel)[::-1]
    low = float(np.max(rel[order[count:]]))
    top = float(rel[order[count - 1]])
    return sorted(int(i) for i in order[:count]), (top / low if low > 0 else np.inf)
