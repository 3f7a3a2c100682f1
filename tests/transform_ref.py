"""float64 numpy statement of fold-in (tests/test_transform_input.py, tests/test_gpu_transform.py): H for data X against a
fixed W, written from the definition in DESIGN.md 4.7 on top of the H-step yardsticks the suite already has; nothing of it
is taken from the code under test.

Iteration t applies the H half-step of MUR for the loss and never touches W:

    'eu', 'kl' without weights      mur_step.ref_h           (the reference's h_update, nmf/mur.py:36-49)
    'eu', 'kl', 'is' with weights   weighted_ref.weighted_h_step
    'is' without weights            is_ref.is_h_step
    'beta'                          beta_ref.beta_h_step     (with or without weights)

obj_history[t] is the objective of (W, H_t), obj_history[0] that of the start; the start without h0 is ONE draw,
np.abs(rng.randn(k, n)); the stop rule is oracle.nmf_ref.stop_rule after min_iter, as in every MUR loop of the suite."""
import numpy as np

from beta_ref import beta_h_step, beta_objective
from is_ref import is_h_step, is_objective
from mur_step import objective as plain_objective
from mur_step import ref_h
from ref_loop import ref_loop
from weighted_ref import weighted_h_step, weighted_objective


def h_step(kind, x, w, h, lam=0.0, om=None, beta=None):
    """One fold-in step: the H half-step of `kind` ('eu' | 'kl' | 'is' | 'beta') with weights om (None: none)."""
    if kind == "beta":
        return beta_h_step(x, w, h, beta, lam, om)
    if om is not None:
        return weighted_h_step(kind, x, om, w, h, lam)
    if kind == "is":
        return is_h_step(x, w, h, lam)
    return ref_h(kind, x, w, h, lam)


def objective(kind, x, w, h, om=None, beta=None):
    if kind == "beta":
        return beta_objective(x, w, h, beta, om)
    if om is not None:
        return weighted_objective(kind, x, om, w, h)
    if kind == "is":
        return is_objective(x, w, h)
    return plain_objective(kind, x, w, h)


def transform_ref(x, w, kind="kl", *, beta=None, om=None, h0=None, min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5,
                  lambda_h=0.0, rng=np.random):
    """Outcome(w, h, i, obj_history, trace) of the fold-in loop; w is returned as it came."""
    w = np.asarray(w, dtype=np.float64)
    k, n = w.shape[1], np.asarray(x).shape[1]
    h = np.abs(rng.randn(k, n)) if h0 is None else np.array(h0, dtype=np.float64)
    return ref_loop(w, h, None, lambda w, h: h_step(kind, x, w, h, lambda_h, om, beta),
                    lambda w, h: objective(kind, x, w, h, om, beta), min_iter, max_iter, tol1, tol2)
