"""Automatic relevance determination (ARD) for MUR with the beta-divergence: `mur_ard(x, k, beta=, phi=)` chooses the rank
inside one fit.  The l1 form of Tan & Fevotte, "Automatic relevance determination in NMF with the beta-divergence" (TPAMI
2013): component c carries a relevance lambda_c shared by column c of W and row c of H; start with k too large and the
superfluous components are driven to zero during the run.

With F x N the shape of x, q = W H + 1e-9, d_beta, gamma and the weights Om of DESIGN.md 4.5, phi > 0 (the dispersion),
a > 0, b > 0 and c = F + N + a + 1:

    C(W, H, lambda) = Sum om d_beta(x | q)  +  phi Sum_c [ (|w_c|_1 + |h_c|_1 + b) / lambda_c + c log lambda_c ]
    lambda_c = (|w_c|_1 + |h_c|_1 + b) / c                     (the closed-form minimiser; its floor is B = b / c)
    W <- W ( ((Om.X.q^(beta-2)) H^T) / ((Om.q^(beta-1)) H^T + phi / lambda_c) )^gamma           column c uses phi / lambda_c
    H <- H ( (W'^T (Om.X.q^(beta-2))) / (W'^T (Om.q^(beta-1)) + phi / lambda_c) )^gamma         q from W' H, the same lambda

Iteration t: the W half-step and the H half-step with lambda_t, then lambda_{t+1} from (W_{t+1}, H_{t+1}); lambda_0 comes
from the start factors.  obj_history[t] = C(W_t, H_t, lambda_t) under the usual tol1 / tol2 stop rule.  The loop runs on the
device (nmfx_set_ard, include/nmfx.h); `objective` evaluates C in float64 on the host."""
from collections import namedtuple

import numpy as np

from . import _lib as L
from . import losses
from . import utils
from . import weighted
from ._driver import run_loop
from .engine import Engine
from .mur import BetaExperiment, check_beta_request, weighted_start

ArdResults = namedtuple('ArdResults', 'w h i obj_history experiment relevance k_eff')
ArdExperiment = namedtuple('Experiment', BetaExperiment._fields + ('phi', 'a', 'b'))


def _positive(name, value):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f'mur_ard: {name} must be a real number (got {name}={value!r})') from None
    if not np.isfinite(v) or v <= 0:
        raise ValueError(f'mur_ard: {name} must be finite and > 0 (got {name}={value!r})')
    return v


def _check_prune_tol(prune_tol):
    try:
        p = float(prune_tol)
    except (TypeError, ValueError):
        raise ValueError(f'prune_tol must be a real number (got prune_tol={prune_tol!r})') from None
    if not 0.0 < p < 1.0:                                       # (NaN included)
        raise ValueError(f'prune_tol must lie in (0, 1) (got prune_tol={prune_tol!r})')
    return p


def _check_default_b(a):
    if not a > 2:
        raise ValueError(f'mur_ard: the default b = sqrt((a - 1)(a - 2) mean(x) / k) needs a > 2 (got a={a!r}); pass b=')


def default_b(x, k, a, weights=None):
    """b = sqrt((a - 1)(a - 2) mean(x) / k), which needs a > 2; with weights, mean(x) is the weighted mean
    Sum om x / Sum om over the cells with om > 0 (x is not read elsewhere)."""
    a = float(a)
    _check_default_b(a)
    if weights is None:
        mean = float(np.mean(np.asarray(x, dtype=np.float64)))
    else:
        om = np.asarray(weights, dtype=np.float64)
        live = om > 0
        mean = float(np.sum(om[live] * np.asarray(x)[live].astype(np.float64)) / np.sum(om[live]))
    return float(np.sqrt((a - 1.0) * (a - 2.0) * mean / int(k)))


def relevance(lam, shape, a, b):
    """(lambda_c - B) / B with the floor B = b / c, c = F + N + a + 1: 0 for a component that has been driven to zero."""
    floor = float(b) / (shape[0] + shape[1] + float(a) + 1.0)
    return (np.asarray(lam, dtype=np.float64) - floor) / floor


def effective_rank(rel, prune_tol=1e-3):
    """#{c : relevance_c > prune_tol max relevance}."""
    rel = np.asarray(rel, dtype=np.float64)
    return int(np.sum(rel > _check_prune_tol(prune_tol) * np.max(rel)))


def objective(x, w, h, lam, beta, phi, a, b, weights=None):
    """C(W, H, lambda) in float64 on the host: the (weighted) beta objective of nmf_amd.weighted.objective plus
    phi Sum_c [ (|w_c|_1 + |h_c|_1 + b) / lambda_c + c log lambda_c ]."""
    x = np.asarray(x)
    w = np.asarray(w, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    om = np.ones(x.shape, dtype=np.float32) if weights is None else weights
    fit = weighted.objective(x, w, h, om, 'beta', beta=beta)
    c = x.shape[0] + x.shape[1] + float(a) + 1.0
    norms = np.sum(np.abs(w), axis=0) + np.sum(np.abs(h), axis=1) + float(b)
    return fit + float(phi) * float(np.sum(norms / lam + c * np.log(lam)))


def mur_ard(x, k, *, beta, phi, a=5.0, b=None, weights=None, prune_tol=1e-3, min_iter=100, max_iter=100000, tol1=1e-5,
            tol2=1e-5, nndsvd_init=(False, 'zero'), save_dir='./results/', device=0):
    """MUR with the beta-divergence and automatic relevance determination.  x, k, beta, weights, min_iter, max_iter, tol1,
    tol2, nndsvd_init, save_dir and device as in mur(x, k, distance_type='beta', ...): dense x, k <= 128 (choose it larger
    than the rank expected), x >= 0 for beta > 0 and strictly positive for beta <= 0, never lifted or modified.  phi > 0:
    the dispersion (a larger phi prunes harder); a > 0, b > 0: the prior's shape and scale, b=None takes
    sqrt((a - 1)(a - 2) mean(x) / k) and needs a > 2.  There is no lambda_w / lambda_h: the penalty is the ARD one.

    Returns ArdResults(w, h, i, obj_history, experiment, relevance, k_eff): relevance = (lambda_c - B) / B per component
    (float64 [k], B = b / (F + N + a + 1) the floor of lambda), k_eff = #{c : relevance_c > prune_tol max relevance}."""
    beta = losses.check_beta('beta', beta)
    phi, a = _positive('phi', phi), _positive('a', a)
    if b is not None:
        b = _positive('b', b)
    else:
        _check_default_b(a)                                     # (before the data is looked at)
    prune_tol = _check_prune_tol(prune_tol)
    check_beta_request(x, k, None, beta)
    if weights is not None:
        x32, w32 = weighted.prepare(x, weights, k, 'beta', beta=beta)
    else:
        losses.check_f32_image(x, 'beta', beta)
        x32, w32 = x, None
    if b is None:
        b = _positive('b', default_b(x, k, a, weights))        # (all-zero data: mean(x) = 0 leaves no default)
    experiment = ArdExperiment('mur_ard', k, 'beta', nndsvd_init, max_iter, tol1, tol2, 0.0, 0.0, beta, phi, a, b)

    if w32 is not None:                                         # the starts of mur(..., distance_type='beta'), with and without weights=
        init = weighted_start(x, x32, w32, k, nndsvd_init)
    else:
        host = utils.initial_factors(x32, k, nndsvd_init, defer_device=True)

        def init(eng):                                          # (an NNDSVD start is computed on the device, from the uploaded x)
            return utils.device_initial_factors(eng, x32, k, nndsvd_init, host)
    with Engine.for_phase(x32, k, init, weights=w32, beta=beta, device=device) as eng:
        eng.set_ard(phi, a, b)
        i, history = run_loop(eng, eng.mur_run, (L.BETA, 0.0, 0.0), eng.mur_finish, (L.BETA,), min_iter, max_iter, tol1, tol2)
        w, h = eng.get_factors()
        rel = relevance(eng.relevance(), x32.shape, a, b)
    return ArdResults(w=w, h=h, i=i, obj_history=history, experiment=experiment, relevance=rel,
                      k_eff=effective_rank(rel, prune_tol))
