"""Inputs shared by tests/test_weighted_input.py (CPU) and tests/test_gpu_weighted.py."""
import numpy as np

from mur_step import OBJ_RTOL
from oracle import nmf_ref as R
from weighted_ref import weighted_mur


def log_uniform_weights(shape, seed, zero_fraction=0.3, edges=False):
    """Weights log-uniform in [2^-10, 2^10], rounded to f32, about `zero_fraction` of the cells 0.  edges: rows 1-2 and
    column 3 carry no weight at all, row 0 and column 0 are positive throughout."""
    rng = np.random.default_rng(seed)
    om = np.exp2(rng.uniform(-10.0, 10.0, shape)).astype(np.float32)
    zero = rng.random(shape) < zero_fraction
    if edges:
        zero[0, :] = False
        zero[:, 0] = False
        zero[1:3, :] = True
        zero[:, 3] = True
    om[zero] = 0
    return om


def run_case(seed=3):
    """250 x 200, k = 5: strictly positive data (every loss accepts it), real-valued weights, ~25 % of the cells unknown
    and holding NaN."""
    x = R.planted_matrix(250, 200, 5, seed=seed, dtype=np.float64) + 0.01
    om = log_uniform_weights(x.shape, seed + 100, zero_fraction=0.25).astype(np.float64)
    return np.where(om > 0, x, np.nan), om


# The stop-rule runs: tol2 is coarse, so that rule 2 (new >= old - tol2) fires while the objective still falls by far more
# than the f32-grade resolution of the recorded objective.  seed of the start factors, min_iter, tol2 per loss.
STOP = {"eu": dict(seed=2, min_iter=5, tol2=80.0), "kl": dict(seed=2, min_iter=5, tol2=280.0), "is": dict(seed=2, min_iter=5, tol2=1700.0)}


def stop_run(kind):
    """(x, om, keywords, the float64 run) of the stop-rule case of `kind`."""
    x, om = run_case()
    c = STOP[kind]
    kw = dict(min_iter=c["min_iter"], max_iter=400, tol1=1e-5, tol2=c["tol2"])
    np.random.seed(c["seed"])
    want = weighted_mur(x, om, 5, distance_type=kind, **kw)
    return x, om, c["seed"], kw, want


def stop_margins(want, tol2):
    """At the stop index and the one before it: |new - (old - tol2)| / (OBJ_RTOL * objective).  Both must be > 1, with room,
    for the device's f32-grade objective (within OBJ_RTOL of the float64 one) to take the same two decisions."""
    h = np.asarray(want.obj_history)
    out = []
    for j in (len(h) - 2, len(h) - 1):              # h[j] = the objective tested at loop index j - 1
        gap = h[j] - (h[j - 1] - tol2)
        out.append(abs(gap) / (OBJ_RTOL * (abs(h[j]) + abs(h[j - 1]))))
    return out
