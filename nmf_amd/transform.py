"""Fold-in: the activations H of new data against a fixed dictionary W.

    res = transform(x_new, nmf.w, distance_type='is')          # or nmf.transform(x_new) after nmf.factorize(...)
    res.h                                                      # k x n, float64

Iteration t applies the H half-step of `mur` for the same loss and never updates W; obj_history[t] is the
objective of (w, h_t), obj_history[0] that of the start.  Every loss of `mur` on dense data is available -- 'eu', 'kl', 'is',
'beta' with beta=, each with or without weights= -- for 1 <= k <= 128.  A step is one pass over x on the device
(nmfx_foldin_run, kernels_phase.hip).  x is never lifted by its minimum and nothing of the caller's is modified.  A dense
hold-out pattern is weights= with a 0 / 1 array; `nmf_amd.weighted.objective` scores the result under any weights.

scipy.sparse data, or data with mask=, goes to `transform_sparse` (below): 'eu' / 'kl' on sparse data and 'eu' / 'kl' / 'is'
on masked data, 1 <= k <= 256, every column of H iterated to its own stop rule in one launch."""
import numbers
from collections import namedtuple

import numpy as np

from . import losses
from . import masked
from . import sparse
from . import weighted
from ._driver import run_loop
from .engine import Engine

TransformResults = namedtuple('TransformResults', 'h i obj_history experiment')
Experiment = namedtuple('Experiment', 'method components distance_type max_iter tol1 tol2 lambda_h')
BetaExperiment = namedtuple('Experiment', Experiment._fields + ('beta',))
MAX_K = 128


def _check_factor(name, a, shape=None, who='transform'):
    """A factor the caller hands in (to `who`): 2-D, real, finite, >= 0 (and of `shape`); returned as float64, the caller's untouched."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f'{who}: {name} must be 2-D (got {a.ndim}-D)')
    if not losses.is_real(a):
        raise ValueError(f'{who}: {name} must be a real array')
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f'{who}: {name} has shape {tuple(a.shape)}, expected {tuple(shape)}')
    a = np.array(a, dtype=np.float64)                            # (a copy)
    if not np.all(np.isfinite(a)):
        raise ValueError(f'{who}: {name} has an entry that is NaN or infinite')
    if a.size and np.min(a) < 0:
        raise ValueError(f'{who}: {name} has a negative entry')
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


SparseTransformResults = namedtuple('SparseTransformResults', 'h iters obj_history experiment')
SparseExperiment = namedtuple('Experiment', 'method components distance_type tol max_iter lambda_h')
MAX_STEPS = 10000


def transform_sparse(x_new, w, mask=None, *, distance_type='kl', h0=None, lambda_h=0.0, tol=1e-4, max_iter=1000, device=0):
    """Multiplicative fold-in for sparse or masked new data: H for `x_new` (m x n) against the fixed dictionary `w`
    (m x k, real, finite, >= 0, 1 <= k <= 256) under the loss of sparse / masked `mur`.

    Without `mask`, `x_new` is scipy.sparse under the rules of nmf_amd.sparse.normalise, its zeros are data, and
    distance_type is 'eu' or 'kl' ('is' is infinite at the zeros).  With `mask`, `x_new` and `mask` follow
    nmf_amd.masked.observed and 'eu', 'kl' and 'is' run ('is': every observed value > 0).  Nothing of the caller's is
    modified or lifted.  With W fixed the columns of H are independent: column c repeats the H half-step of `mur` for that
    loss from h0[:, c] in ONE launch, its iterate in registers (csrc/kernels_sparse.hip), until after step
    t the largest change of a component, max_j |h'_j - h_j|, is at most `tol` times the largest component max_j h'_j, or
    `max_iter` (1 .. 10000).  `h0`: k x n, real, finite, >= 0; the default is the constant sqrt(mean(x_new) / k),
    scikit-learn's start for transform, the float64 mean taken over all m n cells (with `mask`: over the observed
    cells) -- no RNG draw in any case.  Returns SparseTransformResults: h float64 k x n; iters int32 [n], the steps each
    column took; obj_history = [objective(w, h0), objective(w, h)] as sparse / masked `mur` records that pair (float64);
    experiment ('transform_sparse', k, distance_type, tol, max_iter, lambda_h).  Every refusal comes before any device
    work."""
    who = 'transform_sparse'
    if not (isinstance(distance_type, str) and distance_type in ('eu', 'kl', 'is')):
        raise ValueError(f"{who}: distance_type must be 'eu', 'kl' or 'is' (got {distance_type!r})")
    if mask is None and not sparse.is_sparse(x_new):
        raise TypeError(f'{who}: dense x_new needs mask=; without a mask x_new must be a scipy.sparse matrix '
                        '(dense data without a mask: nmf_amd.transform.transform)')
    if mask is None and distance_type == 'is':
        raise ValueError(f"{who}: distance_type='is': the zeros of a sparse matrix have infinite Itakura-Saito divergence; "
                         "pass mask= (for instance the matrix's own pattern) to fit the stored entries only")
    w64 = _check_factor('w', w, who=who)
    k = w64.shape[1]
    if not 1 <= k <= sparse.MAX_K:
        raise ValueError(f'{who}: supports 1 <= k <= {sparse.MAX_K} components (w has {k} columns)')
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not 0 <= tol < 1:
        raise ValueError(f'{who}: tol must be a real number with 0 <= tol < 1 (got tol = {tol!r})')
    if isinstance(max_iter, bool) or not isinstance(max_iter, numbers.Integral) or not 1 <= max_iter <= MAX_STEPS:
        raise ValueError(f'{who}: max_iter must be an integer between 1 and {MAX_STEPS} (got max_iter = {max_iter!r})')
    if isinstance(lambda_h, bool) or not isinstance(lambda_h, numbers.Real) or not lambda_h >= 0:
        raise ValueError(f'{who}: lambda_h must be a real number >= 0 (got lambda_h = {lambda_h!r})')
    try:
        xs = sparse.normalise(x_new, k) if mask is None else masked.observed(x_new, mask, k)
        if distance_type == 'is':
            masked.check_positive(xs)
    except (ValueError, TypeError) as e:
        raise type(e)(f'{who}: {e}') from None
    m, n = xs.shape
    if w64.shape[0] != m:
        raise ValueError(f'{who}: w has {w64.shape[0]} rows, x_new has {m}')
    if h0 is None:
        cells = m * n if mask is None else xs.nnz
        h64 = np.full((k, n), np.sqrt(float(np.sum(xs.data, dtype=np.float64)) / cells / k))
    else:
        h64 = _check_factor('h0', h0, (k, n), who=who)
    experiment = SparseExperiment('transform_sparse', k, distance_type, tol, max_iter, lambda_h)
    with Engine.for_sparse(xs, k, device=device, masked=mask is not None) as eng:
        eng.set_factors(w64, h64)
        eng.sparse_foldin_run(losses.CODES[distance_type], lambda_h, tol, max_iter)
        _, h = eng.get_factors()
        iters = eng.sparse_foldin_iters()
        history = [np.float64(v) for v in eng.objectives(0, 2)]
    return SparseTransformResults(h=h, iters=iters, obj_history=history, experiment=experiment)
