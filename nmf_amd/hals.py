"""HALS on the MI355X engine: hierarchical alternating least squares (Cichocki & Phan 2009; scikit-learn's solver='cd').

Least-squares NMF with the per-iteration cost of a MUR iteration and, usually, far fewer iterations.  One outer iteration
is the W half-step and then the H half-step of `anls` with each exact NNLS solve replaced by `sweeps` projected
Gauss-Seidel sweeps over the k components, from the current row of W / column of H:

    for j = 0 .. k-1:   if G[j, j] > 0:   x[j] = max(0, x[j] + (r[j] - G[j, :] @ x) / G[j, j])

on the same G = F^T F + 2 lambda I and r = F^T b (csrc/kernels_hals.hip on the products of csrc/kernels_anls.hip).  The
clamp is an exact zero.  Defaults, start, printed lines, stop rule, its float64 referee and the history are those of
`anls`; `distance_type` only selects the reported objective, as there.

`rescale_start`: before the first iteration both start factors are multiplied by sqrt(alpha), alpha = <V, W0 H0> / ||W0 H0||^2,
the least-squares optimal scale of the start.  A start scaled far above V (uniform or |randn| factors) makes the very
first W sweep clamp most of W to zero, and the run then needs many iterations to recover."""
import math
import numbers
from collections import namedtuple

import numpy as np

from . import _lib as L
from . import sparse
from . import utils
from ._driver import NEVER, Referee, Results, drive
from .engine import Engine

Experiment = namedtuple('Experiment', 'method components distance_type nndsvd_init max_iter tol1 tol2 lambda_w lambda_h sweeps')

MAX_K = 128
MAX_SWEEPS = 16


def start_scale(eng, w0, h0):
    """alpha = <V, W0 H0> / ||W0 H0||^2 for the V the engine holds, or None where ||W0 H0||^2 = 0.  Nothing V-sized is
    computed on the host: <V, W0 H0> = (||V||^2 + ||W0 H0||^2) / 2 - obj(W0, H0) with both objectives (the second at zero
    factors) in float64 on the device, and ||W0 H0||^2 = <W0^T W0, H0 H0^T> in float64 from the float32 values the device
    holds.  Leaves (W0, H0) set on the engine."""
    w32 = np.asarray(w0, dtype=np.float32).astype(np.float64)
    h32 = np.asarray(h0, dtype=np.float32).astype(np.float64)
    whwh = float(np.sum((w32.T @ w32) * (h32 @ h32.T)))
    if not whwh > 0:
        eng.set_factors(w0, h0)
        return None
    eng.set_factors(np.zeros_like(w32), np.zeros_like(h32))
    half_vv = eng.objective_f64()                      # 1/2 ||V||^2
    eng.set_factors(w0, h0)
    return (half_vv + 0.5 * whwh - eng.objective_f64()) / whwh


def _check(x, k, distance_type, sweeps, lambda_w, lambda_h):
    """Every refusal of hals, before any device work."""
    if distance_type == 'is':
        raise ValueError("hals: distance_type='is' (Itakura-Saito) is a loss of mur only")
    if distance_type == 'beta':
        raise ValueError("hals: distance_type='beta' (the beta-divergence) is a loss of mur only")
    if distance_type not in ('eu', 'kl'):
        raise KeyError('Distance type unknown: use "kl" or "eu"')   # as anls
    sparse.reject(x, 'hals')
    if not isinstance(k, numbers.Integral) or isinstance(k, bool) or k < 1 or k > MAX_K:
        raise ValueError(f'hals: supports 1 <= k <= {MAX_K} components (got k = {k!r})')
    if not isinstance(sweeps, numbers.Integral) or isinstance(sweeps, bool) or not 1 <= sweeps <= MAX_SWEEPS:
        raise ValueError(f'hals: sweeps must be an integer between 1 and {MAX_SWEEPS} (got sweeps = {sweeps!r})')
    for name, lam in (('lambda_w', lambda_w), ('lambda_h', lambda_h)):
        if not lam >= 0:
            raise ValueError(f'hals: {name} must be non-negative (got {name} = {lam!r})')


def hals(x, k, *, distance_type='eu', sweeps=1, rescale_start=True, lambda_w=0, lambda_h=0, min_iter=10,
         max_iter=1000, tol1=1e-3, tol2=1e-3, nndsvd_init=(True, 'zero'), save_dir='./results/',
         device=0, engine=None):
    experiment = Experiment('hals', k, distance_type, nndsvd_init, max_iter, tol1, tol2, lambda_w, lambda_h, sweeps)
    _check(x, k, distance_type, sweeps, lambda_w, lambda_h)
    dist = L.EU if distance_type == 'eu' else L.KL
    init = utils.initial_factors(x, k, nndsvd_init, uniform=True, defer_device=True)
    with Engine.for_data(x, k, device=device, engine=engine) as eng:
        w0, h0 = utils.device_initial_factors(eng, x, k, nndsvd_init, init)
        alpha = start_scale(eng, w0, h0) if rescale_start else None
        if alpha is not None and alpha > 0 and math.isfinite(alpha):
            w0, h0 = np.asarray(w0, dtype=np.float64) * math.sqrt(alpha), np.asarray(h0, dtype=np.float64) * math.sqrt(alpha)
        hals.last_alpha = alpha
        eng.set_factors(w0, h0)
        eng.anls_set_distance(dist)
        referee = None
        if distance_type == 'eu':                   # the stop rule refereed in float64 near the stop (nmf_amd._driver.Referee)
            referee = Referee(eng, lambda i: eng.hals_run(lambda_w, lambda_h, sweeps, NEVER, tol1, tol2, i, 1), min_iter, tol1, tol2)
        hals.last_referee = referee
        i, history = drive(
            eng,
            lambda first, count: eng.hals_run(lambda_w, lambda_h, sweeps, min_iter, tol1, tol2, first, count),
            lambda done: eng.aoadmm_finish(NEVER if referee is not None and referee.walked else min_iter, tol1, tol2, done),
            max_iter, tol1, tol2, referee=referee)
        w, h = eng.get_factors()
    return Results(w=w, h=h, i=i, obj_history=history, experiment=experiment)
