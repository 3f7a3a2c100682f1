"""`NMF(data, components).factorize(method=...)` -- the reference's class API
(nmf/nmf.py:7-135) on top of the MI355X engine."""
import os
from importlib import import_module

from . import sparse
from . import utils

_METHODS = ('mur', 'anls', 'admm', 'ao_admm', 'hals')


def _beyond_hals(factors):
    """More components than nmf_amd.hals.hals takes: factorize('hals') then runs hals_wide (which words the refusal beyond 1024)."""
    import numbers
    from .hals import MAX_K
    return isinstance(factors, numbers.Integral) and not isinstance(factors, bool) and factors > MAX_K


class NMF:
    """Non-negative matrix factorisation of 2-D `data` into `factors`
    components by MUR, ANLS, ADMM or AO-ADMM.

        nmf = NMF(data, factors)
        nmf.factorize(method='mur', **method_params)
        nmf.w, nmf.h            # also nmf.results.w / .h / .i / .obj_history
    """

    def __init__(self, data=None, factors=None, saving=True, param_file=None):
        self.data = data
        self.factors = factors
        self.saving = saving
        self.results = None
        self.w = None
        self.h = None
        if param_file is not None:
            try:
                self.method_params = import_module(param_file).method_params
            except ImportError:
                print('No parameter file found.')

    def factorize(self, method='mur', saving=False, **method_params):
        if method not in _METHODS:
            raise Exception('Method not known. Choose one from: ' + ' '.join(_METHODS))
        solver = getattr(import_module('.' + method, __package__), method)
        if method == 'hals' and 'mask' in method_params:           # (hals_masked takes dense or sparse data)
            masked = import_module('.hals', __package__).hals_masked
            solver = lambda data, factors, mask, **kw: masked(data, factors, mask, **kw)
        elif method == 'hals' and sparse.is_sparse(self.data):     # (hals itself takes dense data only)
            solver = import_module('.hals', __package__).hals_sparse
        elif method == 'hals' and _beyond_hals(self.factors):      # (dense, unmasked, more components than hals keeps in LDS)
            solver = import_module('.hals', __package__).hals_wide
        self.results = solver(self.data, self.factors, **method_params)
        # README.md:22 promises nmf.w / nmf.h; the reference only sets .results
        self.w, self.h = self.results.w, self.results.h
        print('Factorization done.')
        if saving:
            self.save_factorization()

    def transform(self, data, **kw):
        """H for new `data` against the dictionary self.w of the last factorize (nmf_amd.transform.transform): returns
        TransformResults(h, i, obj_history, experiment).  distance_type, and beta with it, default to what that factorize
        used; every keyword of transform may be given.  Sparse `data`, or a mask= among the keywords, goes to the least-squares
        fold-in nmf_amd.hals.hals_transform instead, with the keywords as they are (HalsTransformResults).
        solver='hals' asks for the least-squares fold-in on dense data too: nmf_amd.hals.hals_transform_dense with the other
        keywords as they are (sparse data or mask=: hals_transform, as without it); solver='mur', the default, is everything
        above.  Any other solver is a ValueError."""
        solver = kw.pop('solver', 'mur')
        if not (isinstance(solver, str) and solver in ('mur', 'hals')):
            raise ValueError(f"NMF.transform: solver must be 'mur' or 'hals' (got {solver!r})")
        if self.results is None or self.w is None:
            raise RuntimeError('NMF.transform needs a dictionary: call factorize first')
        if sparse.is_sparse(data) or 'mask' in kw:
            return import_module('.hals', __package__).hals_transform(data, self.w, **kw)
        if solver == 'hals':
            return import_module('.hals', __package__).hals_transform_dense(data, self.w, **kw)
        from .transform import transform
        exp = self.results.experiment
        if 'distance_type' not in kw:
            kw['distance_type'] = getattr(exp, 'distance_type', 'kl')
            if kw['distance_type'] == 'beta' and 'beta' not in kw:
                kw['beta'] = getattr(exp, 'beta', None)
        return transform(data, self.w, **kw)

    def transform_sparse(self, data, mask=None, **kw):
        """H for new sparse or masked `data` against the dictionary self.w of the last factorize, under the loss that
        factorize used (nmf_amd.transform.transform_sparse): returns SparseTransformResults(h, iters, obj_history,
        experiment).  distance_type defaults to the last factorize's when that was 'eu', 'kl' or 'is' (the function's own
        default otherwise); every keyword of transform_sparse may be given.  `transform` keeps the routes it has."""
        if self.results is None or self.w is None:
            raise RuntimeError('NMF.transform needs a dictionary: call factorize first')
        from .transform import transform_sparse
        fitted = getattr(self.results.experiment, 'distance_type', None)
        if 'distance_type' not in kw and isinstance(fitted, str) and fitted in ('eu', 'kl', 'is'):
            kw['distance_type'] = fitted
        return transform_sparse(data, self.w, mask, **kw)

    def save_factorization(self, save_dir='./results', save_name=None):
        """Write results to `save_dir`/`save_name`.npz; the default name follows
        the grammar of nmf/nmf.py:95-126, e.g. nmf_ao_admm_3_eu_0:nn_0.5:l1n_random."""
        os.makedirs(save_dir, exist_ok=True)
        exp = self.results.experiment
        if save_name is None:
            with_prox = exp.method in ('admm', 'ao_admm')
            parts = ['nmf', str(exp.method), str(self.factors), str(exp.distance_type)]
            if exp.method == 'admm':
                parts.append(str(exp.rho))
            parts.append(f'{exp.lambda_w}:{exp.prox_w}' if with_prox else str(exp.lambda_w))
            parts.append(f'{exp.lambda_h}:{exp.prox_h}' if with_prox else str(exp.lambda_h))
            parts.append('nndsvd' + exp.nndsvd_init[1][0] if exp.nndsvd_init[0] else 'random')
            if exp.method == 'anls' and exp.fcnnls:
                parts.append('fcnnls')
            save_name = '_'.join(parts)
        utils.save_results(os.path.join(save_dir, save_name), w=self.results.w, h=self.results.h,
                           i=self.results.i, obj_history=self.results.obj_history,
                           experiment=exp._asdict())
