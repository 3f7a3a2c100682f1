"""ANLS on the MI355X engine.

Same call signature, defaults and return value as the reference's `anls.anls`
(nmf/anls.py:50-135).  Per outer iteration every row of W and then every column
of H is the exact solution of a regularised NNLS problem (anls.py:18-47); the
device solves them from the shared Gram matrix by block principal pivoting
(csrc/kernels_anls.hip).  `use_fcnnls` selects between two solvers of the SAME
strictly convex problems in the reference (scipy's Lawson-Hanson vs
nmf/fcnnls.py); here it is recorded in the experiment tuple (and therefore in
the save-file name) and otherwise has no effect.  `distance_type` only selects
the reported objective, exactly as in the reference."""
import logging
from collections import namedtuple

from . import _lib as L
from . import sparse
from . import utils
from ._driver import Results, run_least_squares
from .engine import Engine

Experiment = namedtuple('Experiment', 'method components distance_type nndsvd_init max_iter tol1 tol2 lambda_w lambda_h fcnnls')


def experiment_of(k, kw):
    """The Experiment tuple of an anls run with the keyword arguments `kw` (anls's own, and dist.factorize's)."""
    return Experiment('anls', k, kw['distance_type'], kw['nndsvd_init'], kw['max_iter'], kw['tol1'], kw['tol2'],
                      kw['lambda_w'], kw['lambda_h'], kw['use_fcnnls'])


def loss_code(solver, distance_type):
    """The library code of 'eu' / 'kl', the objectives the least-squares solvers (`solver`: 'anls', 'hals') report; the
    losses of mur and unknown names are refused."""
    if distance_type == 'is':
        raise ValueError(f"{solver}: distance_type='is' (Itakura-Saito) is a loss of mur only")
    if distance_type == 'beta':
        raise ValueError(f"{solver}: distance_type='beta' (the beta-divergence) is a loss of mur only")
    if distance_type not in ('eu', 'kl'):
        raise KeyError('Distance type unknown: use "kl" or "eu"')   # nmf/utils.py:31 via anls.py:108
    return L.EU if distance_type == 'eu' else L.KL


def anls(x, k, *, distance_type='eu', use_fcnnls=False, lambda_w=0, lambda_h=0, min_iter=10,
         max_iter=1000, tol1=1e-3, tol2=1e-3, nndsvd_init=(True, 'zero'), save_dir='./results/',
         device=0, engine=None):
    experiment = experiment_of(k, locals())
    dist = loss_code('anls', distance_type)
    sparse.reject(x, 'anls')
    init = utils.initial_factors(x, k, nndsvd_init, uniform=True, defer_device=True)
    with Engine.for_data(x, k, device=device, engine=engine) as eng:
        w0, h0 = utils.device_initial_factors(eng, x, k, nndsvd_init, init)
        eng.set_factors(w0, h0)
        eng.anls_set_distance(dist)
        (i, history), _ = run_least_squares(anls, eng, eng.anls_run, (lambda_w, lambda_h), distance_type,
                                            min_iter, max_iter, tol1, tol2)
        w, h = eng.get_factors()
        evicted, capped = eng.diagnostics()
    if capped:                    # (the reference's FCNNLS prints 'Not converged.' there, nmf/fcnnls.py:118)
        logging.warning('%d NNLS solves reached the iteration cap', capped)
    if evicted:
        logging.info('%d passive NNLS variables had a vanished pivot (dead or collinear component) and stay at zero', evicted)
    anls.last_diagnostics = {'nnls_evicted': evicted, 'nnls_capped': capped}
    return Results(w=w, h=h, i=i, obj_history=history, experiment=experiment)
