"""Multiplicative update rules on the MI355X engine.

Same call signature, defaults, side effects and return value as the reference's
`mur.mur` (nmf/mur.py:52-146); the loop body (mur.py:119-131) runs on the
device through libnmfx (nmfx_mur_run, include/nmfx.h)."""
import logging
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

from . import _lib as L
from . import losses
from . import masked
from . import sparse
from . import utils
from . import weighted
from ._driver import BATCH, NEVER, Referee, Results, run_loop, say_objective
from .engine import Engine

Experiment = namedtuple('Experiment', 'method components distance_type nndsvd_init max_iter tol1 tol2 lambda_w lambda_h')
BetaExperiment = namedtuple('Experiment', Experiment._fields + ('beta',))      # distance_type='beta' alone: one trailing field


def experiment_of(k, kw):
    """The Experiment tuple of a mur run with the keyword arguments `kw` (mur's own, and dist.factorize's)."""
    return Experiment('mur', k, kw['distance_type'], kw['nndsvd_init'], kw['max_iter'], kw['tol1'], kw['tol2'],
                      kw['lambda_w'], kw['lambda_h'])


def mur(x, k, *, distance_type='kl', min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5,
        lambda_w=0.0, lambda_h=0.0, nndsvd_init=(False, 'zero'), save_dir='./results/', device=0, engine=None, mask=None, weights=None,
        beta=None):
    """Lee-Seung NMF.  x: 2-D non-negative data (a numpy array, or any scipy.sparse matrix / array with 1 <= k <= 256:
    never densified), k: number of components.

    distance_type 'eu' | 'kl' (default 'kl' as in the reference) | 'is' (Itakura-Saito, beyond the reference: dense
    strictly positive x with k <= 128, or any x with mask= whose observed entries are strictly positive; x is never
    lifted) | 'beta' (the beta-divergence with beta=b, -1 <= b <= 3, beyond the reference: dense x with k <= 128, with or
    without weights=; x >= 0 for b > 0, strictly positive for b <= 0; never lifted; b = 0, 1, 2 are the IS, KL and Euclidean
    losses under the general rule), min_iter, max_iter, tol1, tol2, lambda_w, lambda_h, nndsvd_init=(bool, variant) and
    save_dir have the reference's meaning.  mask: None, or a boolean / 0-1 array or scipy.sparse matrix of x's shape
    whose non-zero entries are the observed set -- only x there is fitted and read (masked MUR, nmf_amd.masked;
    1 <= k <= 256).  weights: None, or a dense real array Omega >= 0 of x's shape (boolean counts as 0 / 1): the fit is
    Sum omega * loss(x, wh) on the dense kernels with k <= 128; a cell with weight 0 is unknown and x is not read there
    (nmf_amd.weighted; not together with mask= or engine=).  Returns Results(w, h, i, obj_history, experiment) with float64 w, h."""
    experiment = experiment_of(k, locals())
    losses.check_loss(distance_type)
    dist = losses.CODES[distance_type]
    beta = losses.check_beta(distance_type, beta)
    loop = (lambda_w, lambda_h, min_iter, max_iter, tol1, tol2)
    if dist == L.BETA:
        experiment = BetaExperiment(*experiment, beta)
        check_beta_request(x, k, mask, beta)
    if weights is not None:
        return _mur_weighted(x, weights, mask, k, dist, experiment, loop, nndsvd_init, device, engine, beta)
    if dist == L.IS and mask is None:
        check_is_request(x, k)
    if dist == L.BETA or (dist == L.IS and mask is None):
        losses.check_f32_image(x, distance_type, beta)         # (not lifted by its minimum, never modified)
    if mask is not None:
        return _mur_masked(x, mask, k, dist, experiment, loop, nndsvd_init, device, engine)
    if sparse.is_sparse(x):
        return _mur_sparse(x, k, dist, experiment, loop, nndsvd_init, device, engine)

    # negative data is lifted IN PLACE on the caller's array (nmf/mur.py:99-101)
    lowest = np.min(x)
    lifted = lowest < 0
    if lifted:
        x += abs(lowest)
        logging.info('Data elevated by {}.'.format(abs(lowest)))

    init = utils.initial_factors(x, k, nndsvd_init, defer_device=True)
    with Engine.for_data(x, k, device=device, engine=engine) as eng:
        if lifted and engine is not None:
            eng.upload_v(x)             # a resident engine still holds the data as it was before the lift
        w0, h0 = utils.device_initial_factors(eng, x, k, nndsvd_init, init)
        eng.set_factors(w0, h0)
        if dist == L.BETA:
            eng.set_beta(beta)
        referee = None
        if distance_type == 'eu':                   # (the float64 objective kernel is the Euclidean one)
            referee = Referee(eng, lambda i: eng.mur_run(dist, lambda_w, lambda_h, NEVER, tol1, tol2, i, 1), min_iter, tol1, tol2)
        return _run(eng, dist, experiment, loop, referee)


def _run(eng, dist, experiment, loop, referee=None):
    """The iterations on an engine that is ready to run, and the Results."""
    lambda_w, lambda_h, min_iter, max_iter, tol1, tol2 = loop
    i, history = run_loop(eng, eng.mur_run, (dist, lambda_w, lambda_h), eng.mur_finish, (dist,), min_iter, max_iter, tol1, tol2,
                          referee=referee)
    mur.last_referee = referee                      # diagnostic: guard in force, iterations walked with the float64 objective
    w, h = eng.get_factors()
    return Results(w=w, h=h, i=i, obj_history=history, experiment=experiment)


def check_is_request(x, k):
    """What Itakura-Saito without a mask runs on, checked before any device work: dense x, k <= 128."""
    if sparse.is_sparse(x):
        raise ValueError("distance_type='is': the zeros of a sparse matrix have infinite Itakura-Saito divergence; "
                         "pass mask= (for instance the matrix's own pattern) to fit the stored entries only")
    if int(k) > 128:
        raise ValueError(f"distance_type='is' supports k <= 128 components on dense input (got k = {k})")


def check_beta_request(x, k, mask, beta):
    """What distance_type='beta' runs on, checked before any device work: dense x, no mask=, k <= 128."""
    if mask is not None:
        raise ValueError(f"distance_type='beta' (beta={beta}): mask= is not supported; pass the 0 / 1 pattern as weights= "
                         "(a dense 0 / 1 array is a mask on the dense kernels)")
    if sparse.is_sparse(x):
        raise ValueError(f"distance_type='beta' (beta={beta}): scipy.sparse input is not supported (the k x k shortcut of the "
                         "sparse path exists only for beta = 1 and beta = 2: distance_type='kl' / 'eu'); pass a dense array")
    if int(k) > 128:
        raise ValueError(f"distance_type='beta' (beta={beta}) supports k <= 128 components (got k = {k})")


def _mur_sparse(x, k, dist, experiment, loop, nndsvd_init, device, engine):
    """MUR on scipy.sparse input (kernels_sparse.hip): the caller's matrix is copied into canonical CSR and never modified.
    The recorded objective is evaluated in float64 from the non-zeros plus k x k terms, so the Euclidean stop rule needs
    no float64 referee here ("Sparse V")."""
    if engine is not None:
        raise ValueError('sparse input: engine= is not supported (the engine is created for the sparse matrix)')
    xs = sparse.normalise(x, k)
    init = utils.initial_factors(xs, k, nndsvd_init)
    with Engine.for_sparse(xs, k, device=device) as eng:
        eng.set_factors(*init)
        return _run(eng, dist, experiment, loop)


def _mur_masked(x, mask, k, dist, experiment, loop, nndsvd_init, device, engine):
    """Masked MUR (kernels_sparse.hip on a masked handle): the observed entries of x, stored zeros included, are the data;
    the rest is unknown.  Everything is validated before any device work; nothing of the caller's is modified.  Same start
    (the global RNG's draws as in mur; NNDSVD of x with the unobserved entries set to 0), Results, printed lines and batching
    as the sparse path; the recorded objective is the masked one, summed in float64 (nmf_amd.masked.objective)."""
    if engine is not None:
        raise ValueError('mask=: engine= is not supported (the engine is created for the observed entries)')
    xs = masked.observed(x, mask, k)
    if dist == L.IS:
        masked.check_positive(xs)
    init = utils.initial_factors(xs, k, nndsvd_init)
    with Engine.for_sparse(xs, k, device=device, masked=True) as eng:
        eng.set_factors(*init)
        return _run(eng, dist, experiment, loop)


def _mur_weighted(x, weights, mask, k, dist, experiment, loop, nndsvd_init, device, engine, beta=None):
    """MUR with per-entry weights (kernels_phase.hip on a dense handle, exact f32): Sum omega * loss(x, wh).  Everything
    is validated before any device work; nothing of the caller's is modified or lifted.  Same start as the masked path
    (the global RNG's draws as in mur; NNDSVD, unweighted and on the host, of x with the zero-weight cells set to 0),
    same Results, printed lines and batching; the recorded objective is the weighted one (nmf_amd.weighted.objective),
    summed per entry, so no float64 referee is needed."""
    if mask is not None:
        raise ValueError('weights= and mask= exclude each other (a mask is the 0 / 1 case of weights)')
    if engine is not None:
        raise ValueError('weights=: engine= is not supported (the engine is created for the weighted data)')
    x32, w32 = weighted.prepare(x, weights, k, experiment.distance_type, beta=beta)
    init = weighted_start(x, x32, w32, k, nndsvd_init)
    with Engine.for_phase(x32, k, init, weights=w32, beta=beta, device=device) as eng:
        return _run(eng, dist, experiment, loop)


def weighted_start(x, x32, w32, k, nndsvd_init):
    """The start factors of a weighted run (x32, w32 from weighted.prepare): the global RNG's draws as in mur, or the
    NNDSVD, unweighted and on the host, of x with the zero-weight cells set to 0."""
    if nndsvd_init[0]:
        with np.errstate(invalid='ignore'):
            start = np.where(w32 > 0, np.asarray(x), 0)
        return utils.initial_factors(sp.csr_matrix(start), k, nndsvd_init)      # (the masked path's NNDSVD)
    return utils.initial_factors(x32, k, nndsvd_init)


def mur_pair(x, k, params, *, min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5, nndsvd_init=(False, 'zero'),
             save_dir='./results/', engine=None, device=0):
    """TWO Euclidean MUR factorizations of the same data in one pass over it (the parameter grids of the
    reference's author, nmf/nmf_old.py:52-66): `params` = two dicts with `lambda_w`, `lambda_h` (and optionally `k`, each
    <= 64; default: the common `k`).  Equivalent to two consecutive `mur(x, k_p, distance_type='eu', ...)` calls -- same draws
    from the global numpy RNG in the same order (W, H of the first problem, then of the second), same printed lines in the same
    order, same Results -- but V is streamed once per half-iteration for both problems (nmfx_mur_pair_run: the two problems
    sit in the halves of the k = 128 layouts).  `engine`: a k = 128 Engine that already holds x (nmf_amd.grid keeps one
    resident).  Returns [Results, Results]."""
    if len(params) != 2:
        raise ValueError('mur_pair takes exactly two parameter sets')
    ks = [int(p.get('k', k)) for p in params]
    if max(ks) > 64 or min(ks) < 1:
        raise ValueError('mur_pair: each problem needs 1 <= k <= 64')
    lws = [float(p.get('lambda_w', 0.0)) for p in params]
    lhs = [float(p.get('lambda_h', 0.0)) for p in params]
    if max_iter <= 0:
        raise UnboundLocalError("local variable 'i' referenced before assignment")
    lowest = np.min(x)
    lifted = lowest < 0
    if lifted:                                                  # nmf/mur.py:99-101 (the first call lifts, the second sees >= 0)
        x += abs(lowest)
        logging.info('Data elevated by {}.'.format(abs(lowest)))
    m, n = x.shape
    inits = [utils.initial_factors(x, kk, nndsvd_init, defer_device=True) for kk in ks]     # reference RNG order: problem 0, then 1
    with Engine.for_data(x, 128, device=device, engine=engine) as eng:
        if eng.precision() != 'bf16':
            raise RuntimeError('mur_pair runs on the split-bf16 path only (NMFX_PRECISION=f32 is set, or the engine fell back)')
        if lifted and engine is not None:
            eng.upload_v(x)
        w0 = np.zeros((m, 128))
        h0 = np.zeros((128, n))
        for p, kk in enumerate(ks):
            wp, hp = utils.device_initial_factors(eng, x, kk, nndsvd_init, inits[p])
            w0[:, 64 * p:64 * p + kk] = wp
            h0[64 * p:64 * p + kk] = hp
        eng.set_factors(w0, h0)
        logging.info('Entering Main Loop.')
        done, rules = 0, [0, 0]
        while done < max_iter and not all(rules):
            count = min(BATCH, max_iter - done)
            eng.mur_pair_run(lws, lhs, min_iter, tol1, tol2, done, count)
            done += count
            if done == max_iter:
                eng.mur_pair_finish(min_iter, tol1, tol2, done)
            rules = [eng.pair_state(p)[0] for p in (0, 1)]
        out = []
        digits = utils.tol_digits(tol1, tol2)
        for p, kk in enumerate(ks):
            rule, stop_i, n_obj = eng.pair_state(p)
            history = [np.float64(v) for v in eng.pair_objectives(p, 0, n_obj)]
            w, h = eng.pair_get_factors(p, kk)
            if rule:
                i, history = stop_i, history[:stop_i + 2]
            else:
                i = max_iter - 1
            for it, val in enumerate(history[1:]):              # the lines the reference prints, problem by problem
                say_objective(it, val, digits)
            if rule:
                utils.convergence_message(rule)
                logging.warning('Converged.')
            else:
                logging.info('Max iteration reached.')
            experiment = Experiment('mur', kk, 'eu', nndsvd_init, max_iter, tol1, tol2, lws[p], lhs[p])
            out.append(Results(w=w, h=h, i=i, obj_history=history, experiment=experiment))
    return out
