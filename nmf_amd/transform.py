"""Fold-in: the activations H of new data against a fixed dictionary W.

    res = transform(x_new, nmf.w, distance_type='is')          # or nmf.transform(x_new) after nmf.factorize(...)
    res.h                                                      # k x n, float64

Iteration t applies the H half-step of `mur` for the same loss and never updates W; obj_history[t] is the
objective of (w, h_t), obj_history[0] that of the start.  Every loss of `mur` on dense data is available -- 'eu', 'kl', 'is',
'beta' with beta=, each with or without weights= -- for 1 <= k <= 128.  A step is one pass over x on the device
(nmfx_foldin_run, kernels_phase.hip).  x is never lifted by its minimum and nothing of the caller's is modified.  A dense
hold-out pattern is weights= with a 0 / 1 array; `nmf_amd.weighted.objective` scores the result under any weights."""
from collections import namedtuple

import numpy as np

from . import losses
from . import sparse
from . import weighted
from ._driver import run_loop
from .engine import Engine

TransformResults = namedtuple('TransformResults', 'h i obj_history experiment')
Experiment = namedtuple('Experiment', 'method components distance_type max_iter tol1 tol2 lambda_h')
BetaExperiment = namedtuple('Experiment', Experiment._fields + ('beta',))
MAX_K = 128


def _check_factor(name, a, shape=None):
    """A factor the caller hands in: 2-D, real, finite, >= 0 (and of `shape`); returned as float64, the caller's untouched."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f'transform: {name} must be 2-D (got {a.ndim}-D)')
    if not losses.is_real(a):
        raise ValueError(f'transform: {name} must be a real array')
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f'transform: {name} has shape {tuple(a.shape)}, expected {tuple(shape)}')
    a = np.array(a, dtype=np.float64)                            # (a copy)
    if not np.all(np.isfinite(a)):
        raise ValueError(f'transform: {name} has an entry that is NaN or infinite')
    if a.size and np.min(a) < 0:
        raise ValueError(f'transform: {name} has a negative entry')
    return a


def transform(x, w, *, distance_type='kl', beta=None, weights=None, h0=None, min_iter=100, max_iter=100000,
              tol1=1e-5, tol2=1e-5, lambda_h=0.0, device=0):
    """H for the data x (m x n, dense) against the fixed dictionary w (m x k, >= 0, 1 <= k <= 128).

    distance_type, beta, weights, min_iter, max_iter, tol1, tol2 and lambda_h have the meaning they have in `mur`; h0 is
    the start (k x n, >= 0; None draws np.abs(np.random.randn(k, n)) from the global RNG: one draw).  Returns
    TransformResults(h, i, obj_history, experiment) with float64 h; i and obj_history follow `mur` (i + 2 entries).
    There is no mask= (a TypeError, like any unknown keyword): a dense 0 / 1 pattern is weights=."""
    if distance_type not in ('eu', 'kl', 'is', 'beta'):
        raise ValueError(f"transform: distance_type must be 'eu', 'kl', 'is' or 'beta' (got {distance_type!r})")
    beta = losses.check_beta(distance_type, beta)
    if sparse.is_sparse(x):
        raise TypeError('transform: scipy.sparse input is not supported; pass a dense array (a dense 0 / 1 hold-out '
                        'pattern is weights=)')
    xa = np.asarray(x)
    if xa.ndim != 2:
        raise ValueError(f'transform: x must be 2-D (got {xa.ndim}-D)')
    w64 = _check_factor('w', w)
    m, n = xa.shape
    k = w64.shape[1]
    if w64.shape[0] != m:
        raise ValueError(f'transform: w has {w64.shape[0]} rows, x has {m}')
    if not 1 <= k <= MAX_K:
        raise ValueError(f'transform supports 1 <= k <= {MAX_K} components (w has {k} columns)')
    if m < 1 or n < 1:
        raise ValueError('transform: x is empty')
    h64 = None if h0 is None else _check_factor('h0', h0, (k, n))
    if int(max_iter) < 1:
        raise ValueError(f'transform: max_iter must be >= 1 (got {max_iter})')
    if weights is not None:
        try:
            x32, w32 = weighted.prepare(xa, weights, k, distance_type, beta=beta)
        except TypeError as e:
            raise ValueError(f'transform: {e}') from None
    else:
        if not losses.is_real(xa):
            raise ValueError('transform: x must be a real array')
        # 'eu' and 'kl' are not lifted here: finite and >= 0 in float32, a zero is data, in transform's own name
        losses.check_f32_image(xa, distance_type, beta, label='transform' if distance_type in ('eu', 'kl') else None)
        x32, w32 = xa, None
    experiment = Experiment('transform', k, distance_type, max_iter, tol1, tol2, lambda_h)
    if distance_type == 'beta':
        experiment = BetaExperiment(*experiment, beta)
    if h64 is None:
        h64 = np.abs(np.random.randn(k, n))
    dist = losses.CODES[distance_type]

    with Engine.for_phase(x32, k, (w64, h64), weights=w32, beta=beta, device=device) as eng:
        i, history = run_loop(eng, eng.foldin_run, (dist, lambda_h), eng.foldin_finish, (dist,), min_iter, max_iter, tol1, tol2)
        _, h = eng.get_factors()
    return TransformResults(h=h, i=i, obj_history=history, experiment=experiment)
