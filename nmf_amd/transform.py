"""Fold-in: the activations H of new data against a fixed dictionary W.

    res = transform(x_new, nmf.w, distance_type='is')          # or nmf.transform(x_new) after nmf.factorize(...)
    res.h                                                      # k x n, float64

Iteration t applies the H half-step of `mur` for the same loss and never updates W; obj_history[t] is the
objective of (w, h_t), obj_history[0] that of the start.  Every loss of `mur` on dense data is available -- 'eu', 'kl', 'is',
'beta' with beta=, each with or without weights= -- for 1 <= k <= 128.  A step is one pass over x on the device
(nmfx_foldin_run, kernels_phase.hip).  x is never lifted by its minimum and nothing of the caller's is modified.  A dense
hold-out pattern is weights= with a 0 / 1 array; `nmf_amd.weighted.objective` scores the result under any weights."""
import logging
from collections import namedtuple

import numpy as np

from . import _lib as L
from . import sparse
from . import weighted
from ._driver import drive
from .engine import Engine
from .mur import _check_beta_input, _check_is_input, check_beta

TransformResults = namedtuple('TransformResults', 'h i obj_history experiment')
Experiment = namedtuple('Experiment', 'method components distance_type max_iter tol1 tol2 lambda_h')
BetaExperiment = namedtuple('Experiment', Experiment._fields + ('beta',))
MAX_K = 128


def _check_factor(name, a, shape=None):
    """A factor the caller hands in: 2-D, real, finite, >= 0 (and of `shape`); returned as float64, the caller's untouched."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f'transform: {name} must be 2-D (got {a.ndim}-D)')
    if a.dtype == object or not (np.issubdtype(a.dtype, np.number) or a.dtype == bool) or np.issubdtype(a.dtype, np.complexfloating):
        raise ValueError(f'transform: {name} must be a real array')
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f'transform: {name} has shape {tuple(a.shape)}, expected {tuple(shape)}')
    a = np.array(a, dtype=np.float64)                            # (a copy)
    if not np.all(np.isfinite(a)):
        raise ValueError(f'transform: {name} has an entry that is NaN or infinite')
    if a.size and np.min(a) < 0:
        raise ValueError(f'transform: {name} has a negative entry')
    return a


def _check_plain_input(x):
    """'eu' and 'kl' without weights: finite and >= 0 in float32; a zero is data, so a positive value must not underflow to
    one (the rules of mur._check_beta_input for beta > 0)."""
    try:
        _check_beta_input(x, 1.0)
    except ValueError as e:
        raise ValueError(str(e).replace("distance_type='beta' (beta=1.0)", 'transform')) from None


def transform(x, w, *, distance_type='kl', beta=None, weights=None, h0=None, min_iter=100, max_iter=100000,
              tol1=1e-5, tol2=1e-5, lambda_h=0.0, device=0):
    """H for the data x (m x n, dense) against the fixed dictionary w (m x k, >= 0, 1 <= k <= 128).

    distance_type, beta, weights, min_iter, max_iter, tol1, tol2 and lambda_h have the meaning they have in `mur`; h0 is
    the start (k x n, >= 0; None draws np.abs(np.random.randn(k, n)) from the global RNG: one draw).  Returns
    TransformResults(h, i, obj_history, experiment) with float64 h; i and obj_history follow `mur` (i + 2 entries).
    There is no mask= (a TypeError, like any unknown keyword): a dense 0 / 1 pattern is weights=."""
    if distance_type not in ('eu', 'kl', 'is', 'beta'):
        raise ValueError(f"transform: distance_type must be 'eu', 'kl', 'is' or 'beta' (got {distance_type!r})")
    beta = check_beta(distance_type, beta)
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
        if xa.dtype == object or not (np.issubdtype(xa.dtype, np.number) or xa.dtype == bool) or np.issubdtype(xa.dtype, np.complexfloating):
            raise ValueError('transform: x must be a real array')
        if distance_type == 'is':
            _check_is_input(xa, k)
        elif distance_type == 'beta':
            _check_beta_input(xa, beta)
        else:
            _check_plain_input(xa)
        x32, w32 = xa, None
    experiment = Experiment('transform', k, distance_type, max_iter, tol1, tol2, lambda_h)
    if distance_type == 'beta':
        experiment = BetaExperiment(*experiment, beta)
    if h64 is None:
        h64 = np.abs(np.random.randn(k, n))
    dist = {'eu': L.EU, 'kl': L.KL, 'is': L.IS, 'beta': L.BETA}[distance_type]

    with Engine(m, n, k, device=device) as eng:
        eng.upload_v(x32)
        if w32 is not None:
            eng.upload_weights(w32)
        eng.set_factors(w64, h64)
        if dist == L.BETA:
            eng.set_beta(beta)
        logging.info('Entering Main Loop.')
        i, history = drive(
            eng,
            lambda first, count: eng.foldin_run(dist, lambda_h, min_iter, tol1, tol2, first, count),
            lambda done: eng.foldin_finish(dist, min_iter, tol1, tol2, done),
            max_iter, tol1, tol2, referee=None)
        _, h = eng.get_factors()
    return TransformResults(h=h, i=i, obj_history=history, experiment=experiment)
