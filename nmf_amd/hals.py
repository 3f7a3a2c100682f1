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
first W sweep clamp most of W to zero, and the run then needs many iterations to recover.

`hals_sparse` is the same iteration on scipy.sparse input: the right-hand sides are gathered from the non-zeros and swept in
the same launch (csrc/kernels_sparse.hip); `hals` itself takes dense data only.

`hals_wide` is `hals` for 129 <= k <= 1024 on dense data.

`hals_sparse_wide` is `hals_sparse` for 129 <= k <= 256: the right-hand sides are gathered into a buffer and
swept by the kernel of `hals_wide`.

`hals_stack` runs many Euclidean problems on the same data side by side in the factor columns of one engine: one pair of
passes over V per iteration for all of them.

`hals_masked` fits only the observed entries of V.  With entries missing the rows no longer share one Gram
matrix: each owned row (a row of W, or a column of H) is swept on its own system over its observed set Omega,

    G = Sum_{e in Omega} f_e f_e^T + 2 lambda I        r = Sum_{e in Omega} v_e f_e

where F is the other factor (for the H half-step the W just updated) and f_e its row at entry e: `sweeps` passes of the sweep
above, the clamp an exact zero.  A component with G_jj = 0 keeps its value -- with lambda = 0 that is every component of a
row with no observed entry, and a dead component.  An observed zero is data: it adds to G and not to r.  Values of x outside
the mask are never read (NaN is fine there).  With an all-ones mask this is `hals(x, k, distance_type='eu')`.

`hals_transform` is the least-squares fold-in of such fits: H for new sparse or masked data against a fixed
W.  With W fixed a column's (G, r) never changes, so it is formed once and swept to convergence in place.
`hals_transform_dense` is the same fold-in for dense new data: all columns share one Gram matrix and the
right-hand sides are the H half-step's own product, so it costs one pass over the data and k x n work behind it."""
import logging
import math
import numbers
from collections import namedtuple

import numpy as np

from . import losses
from . import masked
from . import sparse
from . import utils
from ._driver import BATCH, Referee, Results, drive, require_iterations, say_objective, run_least_squares
from .anls import loss_code
from .engine import Engine

Experiment = namedtuple('Experiment', 'method components distance_type nndsvd_init max_iter tol1 tol2 lambda_w lambda_h sweeps')

MAX_K = 128
MAX_K_WIDE = 1024            # hals_wide: the sweep keeps k / 64 variables per lane in registers
MAX_K_MASKED = 64            # hals_masked: a k x k Gram per row, formed in registers and swept from LDS
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


def scaled_start(alpha, w0, h0):
    """The start (w0, h0) times sqrt(alpha), in float64, where alpha (start_scale's, or None) is positive and finite; the start
    as it is otherwise."""
    if alpha is None or not (alpha > 0 and math.isfinite(alpha)):
        return w0, h0
    return np.asarray(w0, dtype=np.float64) * math.sqrt(alpha), np.asarray(h0, dtype=np.float64) * math.sqrt(alpha)


def _is_count(value, most=None):
    return isinstance(value, numbers.Integral) and not isinstance(value, bool) and value >= 1 and (most is None or value <= most)


_ABSENT = object()


def check_args(who, *, k=_ABSENT, sweeps=_ABSENT, lambda_w=_ABSENT, lambda_h=_ABSENT, real_lambdas, problem=None, most=MAX_K):
    """The HALS rules for k, sweeps and a lambda, stated once, in the order k, sweeps, lambda_w, lambda_h; what is not given is
    not checked.  `who` is the front end's name.  `problem`: the index of a problem of a stack, whose k has no bound of its own
    (the stack's total has); `most`: the front end's largest k.  `real_lambdas` is inherited: hals_stack and hals_sparse refuse a bool or a non-Real lambda, hals
    takes whatever answers `lam >= 0` with something true (True, for one)."""
    at = who if problem is None else f'{who}: problem {problem}'
    if k is not _ABSENT and not _is_count(k, most if problem is None else None):
        if problem is None:
            raise ValueError(f'{who}: supports 1 <= k <= {most} components (got k = {k!r})')
        raise ValueError(f'{at} needs an integer k >= 1 (got k = {k!r})')
    if sweeps is not _ABSENT and not _is_count(sweeps, MAX_SWEEPS):
        raise ValueError(f'{who}: sweeps must be an integer between 1 and {MAX_SWEEPS} (got sweeps = {sweeps!r})')
    for name, lam in (('lambda_w', lambda_w), ('lambda_h', lambda_h)):
        if lam is _ABSENT:
            continue
        if (real_lambdas and (isinstance(lam, bool) or not isinstance(lam, numbers.Real))) or not lam >= 0:
            raise ValueError(f'{at}: {name} must be non-negative (got {name} = {lam!r})')


def check_hals(x, k, distance_type, sweeps, lambda_w, lambda_h):
    """Every refusal of hals, before any device work (nmf_amd.grid asks for a whole grid first).  Returns the loss's library code."""
    dist = loss_code('hals', distance_type)
    sparse.reject(x, 'hals')
    check_args('hals', k=k, sweeps=sweeps, lambda_w=lambda_w, lambda_h=lambda_h, real_lambdas=False)
    return dist


_STACK_KEYS = ('k', 'lambda_w', 'lambda_h')


def _check_stack(x, problems, sweeps):
    """Every refusal of hals_stack, before any device work and before any RNG draw.  Returns [(k, lambda_w, lambda_h)]."""
    sparse.reject(x, 'hals_stack')
    try:
        problems = list(problems)
    except TypeError:
        raise ValueError(f'hals_stack: problems must be a non-empty sequence of dicts (got {problems!r})') from None
    if not problems:
        raise ValueError('hals_stack: problems is empty: it takes at least one dict with the key k')
    out = []
    for p, prob in enumerate(problems):
        if not isinstance(prob, dict):
            raise ValueError(f'hals_stack: problem {p} is not a dict (got {prob!r})')
        unknown = sorted(set(prob) - set(_STACK_KEYS), key=str)
        if unknown:
            raise ValueError(f'hals_stack: problem {p} has the unknown key {unknown[0]!r} (known: k, lambda_w, lambda_h)')
        if 'k' not in prob:
            raise ValueError(f'hals_stack: problem {p} has no k')
        k, lw, lh = prob['k'], prob.get('lambda_w', 0), prob.get('lambda_h', 0)
        check_args('hals_stack', k=k, lambda_w=lw, lambda_h=lh, real_lambdas=True, problem=p)
        out.append((int(k), lw, lh))
    total = sum(k for k, _, _ in out)
    if total > MAX_K:
        raise ValueError(f'hals_stack: the problems hold {total} components together; a stack takes at most {MAX_K}')
    check_args('hals_stack', sweeps=sweeps, real_lambdas=True)
    return out


def hals_stack(x, problems, *, sweeps=1, rescale_start=True, min_iter=10, max_iter=1000, tol1=1e-3, tol2=1e-3,
               nndsvd_init=(True, 'zero'), device=0, engine=None):
    """MANY Euclidean HALS factorizations of the same data in one pass over it per half-iteration: `problems` is a
    non-empty sequence of dicts with `k` and optionally `lambda_w`, `lambda_h` (default 0), 1 <= k_p, sum of the k_p <= 128.
    Returns [Results], one per problem in order; problem p's result is what
    `hals(x, k_p, lambda_w=.., lambda_h=.., sweeps=.., rescale_start=.., distance_type='eu', ...)` defines from the same
    start: the problems draw from the global numpy RNG in problem order as consecutive `hals` calls would, each start is
    scaled by its own sqrt(alpha_p) (`hals_stack.last_alpha`), and history, stop rule and the iterate kept at a stop are per
    problem -- a problem that has stopped keeps its iterate while the others go on.  The lines `hals` prints come problem
    by problem after the run.

    The problems sit side by side in the factor columns of one engine (nmfx_hals_stack_*): the two products with V per
    iteration serve all of them, and the Gram entries between different problems are masked in the sweep.

    The stop rule runs on the stack's own recorded objective,
        1/2 ||V||^2 - <W_p, V H_p^T> + 1/2 <W_p^T W_p, H_p H_p^T>
    (float32 product V H^T, everything else float64).  It carries more rounding than the residual objective `hals` records
    (a difference of large terms near an exact fit), and no float64 Referee stands behind it: a single `hals` run may stop
    at another index where the decrease per iteration is near tol2.  `hals_stack.last_would_arm` holds, per problem,
    `Referee.would_arm(history_p, tol2)`: True says a single run would have been refereed there.

    `engine`: an Engine with k >= the sum of the k_p that already holds x (nmf_amd.grid keeps a k = 128 one resident)."""
    probs = _check_stack(x, problems, sweeps)
    require_iterations(max_iter)
    ks = [k for k, _, _ in probs]
    lws = [float(lw) for _, lw, _ in probs]
    lhs = [float(lh) for _, _, lh in probs]
    total = sum(ks)
    inits = [utils.initial_factors(x, k, nndsvd_init, uniform=True, defer_device=True) for k in ks]     # RNG order: problem by problem
    m, n = x.shape
    if engine is not None and (engine.m, engine.n) == (m, n) and total <= engine.k <= MAX_K:
        scope_k = engine.k
    else:
        scope_k = total
    with Engine.for_data(x, scope_k, device=device, engine=engine) as eng:
        def stacked(alphas):
            w0, h0 = np.zeros((m, eng.k)), np.zeros((eng.k, n))
            o = 0
            for p, k in enumerate(ks):
                w0[:, o:o + k], h0[o:o + k] = scaled_start(alphas[p], *starts[p])
                o += k
            return w0, h0
        starts = [utils.device_initial_factors(eng, x, k, nndsvd_init, inits[p]) for p, k in enumerate(ks)]
        alphas = [None] * len(ks)
        eng.set_factors(*stacked(alphas))
        eng.hals_stack_set(ks)
        if rescale_start:
            alphas = [dot / whwh if whwh > 0 else None for dot, whwh in eng.hals_stack_terms()]
            eng.set_factors(*stacked(alphas))
        hals_stack.last_alpha = alphas
        logging.info('Entering Main Loop.')
        done, rules = 0, [0] * len(ks)
        while done < max_iter and not all(rules):
            count = min(BATCH, max_iter - done)
            eng.hals_stack_run(lws, lhs, sweeps, min_iter, tol1, tol2, done, count)
            done += count
            if done == max_iter:
                eng.hals_stack_finish(min_iter, tol1, tol2, done)
            rules = [eng.hals_stack_state(p)[0] for p in range(len(ks))]
        out, arm = [], []
        digits = utils.tol_digits(tol1, tol2)
        for p, k in enumerate(ks):
            rule, stop_i, n_obj = eng.hals_stack_state(p)
            history = [np.float64(v) for v in eng.hals_stack_objectives(p, 0, n_obj)]
            w, h = eng.hals_stack_get_factors(p)
            if rule:
                i, history = stop_i, history[:stop_i + 2]
            else:
                i = max_iter - 1
            for it, val in enumerate(history[1:]):              # the lines hals prints, problem by problem
                say_objective(it, val, digits)
            if rule:
                utils.convergence_message(rule)
                logging.warning('Converged.')
            else:
                logging.info('Max iteration reached.')
            arm.append(Referee.would_arm(history, tol2))
            experiment = Experiment('hals', k, 'eu', nndsvd_init, max_iter, tol1, tol2, probs[p][1], probs[p][2], sweeps)
            out.append(Results(w=w, h=h, i=i, obj_history=history, experiment=experiment))
        hals_stack.last_would_arm = arm
    return out


def _run_dense(solver, run_of, x, k, dist, distance_type, sweeps, rescale_start, lambda_w, lambda_h, min_iter, max_iter, tol1,
               tol2, nndsvd_init, device, engine):
    """hals and hals_wide behind their refusals: the start, its scale, the run loop and the Results.  `run_of(eng)` is the
    engine's run call; `solver` takes last_alpha and last_referee."""
    experiment = Experiment('hals', k, distance_type, nndsvd_init, max_iter, tol1, tol2, lambda_w, lambda_h, sweeps)
    init = utils.initial_factors(x, k, nndsvd_init, uniform=True, defer_device=True)
    with Engine.for_data(x, k, device=device, engine=engine) as eng:
        w0, h0 = utils.device_initial_factors(eng, x, k, nndsvd_init, init)
        alpha = start_scale(eng, w0, h0) if rescale_start else None
        solver.last_alpha = alpha
        eng.set_factors(*scaled_start(alpha, w0, h0))
        eng.anls_set_distance(dist)
        (i, history), _ = run_least_squares(solver, eng, run_of(eng), (lambda_w, lambda_h, sweeps), distance_type,
                                            min_iter, max_iter, tol1, tol2)
        w, h = eng.get_factors()
    return Results(w=w, h=h, i=i, obj_history=history, experiment=experiment)


def _run_sparse(solver, *, check, prepare, refusals, keep_class, masked_engine, scale_of, calls_of, k, sweeps, rescale_start, lambda_w,
                lambda_h, min_iter, max_iter, tol1, tol2, nndsvd_init, device):
    """hals_sparse, hals_sparse_wide and hals_masked: the argument check, the data, the start, its scale, the run loop and the
    Results.  `check()` makes the front end's refusals; `prepare()` returns the canonical sparse data and refuses with one of
    `refusals`, raised again under the solver's name as a ValueError, or with `keep_class` as the class it had;
    `masked_engine` is Engine.for_sparse's masked=; `scale_of(eng, w0, h0)` is the start's scale; `calls_of(eng)` the engine's
    run and finish calls; `solver` takes last_alpha."""
    experiment = Experiment('hals', k, 'eu', nndsvd_init, max_iter, tol1, tol2, lambda_w, lambda_h, sweeps)
    check()
    try:
        xs = prepare()
    except refusals as e:
        raise (type(e) if keep_class else ValueError)(f'{solver.__name__}: {e}') from None
    w0, h0 = utils.initial_factors(xs, k, nndsvd_init, uniform=True)
    with Engine.for_sparse(xs, k, device=device, masked=masked_engine) as eng:
        alpha = scale_of(eng, w0, h0) if rescale_start else None
        solver.last_alpha = alpha
        eng.set_factors(*scaled_start(alpha, w0, h0))
        run, finish = calls_of(eng)
        i, history = drive(
            eng,
            lambda first, count: run(lambda_w, lambda_h, sweeps, min_iter, tol1, tol2, first, count),
            lambda done: finish(min_iter, tol1, tol2, done),
            max_iter, tol1, tol2, referee=None)
        w, h = eng.get_factors()
    return Results(w=w, h=h, i=i, obj_history=history, experiment=experiment)


def hals(x, k, *, distance_type='eu', sweeps=1, rescale_start=True, lambda_w=0, lambda_h=0, min_iter=10,
         max_iter=1000, tol1=1e-3, tol2=1e-3, nndsvd_init=(True, 'zero'), save_dir='./results/',
         device=0, engine=None):
    dist = check_hals(x, k, distance_type, sweeps, lambda_w, lambda_h)
    return _run_dense(hals, lambda eng: eng.hals_run, x, k, dist, distance_type, sweeps, rescale_start, lambda_w, lambda_h,
                      min_iter, max_iter, tol1, tol2, nndsvd_init, device, engine)


def check_hals_wide(x, k, distance_type, sweeps, lambda_w, lambda_h):
    """Every refusal of hals_wide, before any device work and before any RNG draw.  Returns the loss's library code."""
    dist = loss_code('hals_wide', distance_type)
    if sparse.is_sparse(x):
        raise TypeError(f'hals_wide: takes dense data only; hals_sparse runs scipy.sparse input with k <= {MAX_K}')
    if not (_is_count(k, MAX_K_WIDE) and k > MAX_K):
        hint = f'; hals runs 1 <= k <= {MAX_K}' if _is_count(k, MAX_K) else ''
        raise ValueError(f'hals_wide: supports {MAX_K + 1} <= k <= {MAX_K_WIDE} components (got k = {k!r}){hint}')
    check_args('hals_wide', sweeps=sweeps, lambda_w=lambda_w, lambda_h=lambda_h, real_lambdas=False)
    return dist


def hals_wide(x, k, *, distance_type='eu', sweeps=1, rescale_start=True, lambda_w=0, lambda_h=0, min_iter=10,
              max_iter=1000, tol1=1e-3, tol2=1e-3, nndsvd_init=(True, 'zero'), save_dir='./results/',
              device=0, engine=None):
    """`hals` with 129 <= k <= 1024 components on dense data: the same outer iteration -- start, RNG draws, `rescale_start`,
    printed lines, stop rule with its float64 referee, history, Results and Experiment('hals', ...) are those of `hals` -- on the
    products `anls` runs beyond 128 components, with the sweeps by a kernel that streams the k x k Gram matrix through LDS in
    row tiles where `hals` keeps it there whole (csrc/kernels_hals.hip).  The update order within a sweep is
    the definition above: component j sees the new x_0 .. x_{j-1}."""
    dist = check_hals_wide(x, k, distance_type, sweeps, lambda_w, lambda_h)
    return _run_dense(hals_wide, lambda eng: eng.hals_wide_run, x, k, dist, distance_type, sweeps, rescale_start, lambda_w,
                      lambda_h, min_iter, max_iter, tol1, tol2, nndsvd_init, device, engine)


def _check_sparse(x, k, sweeps, lambda_w, lambda_h):
    """Every refusal of hals_sparse but the one of the stored values, before any device work and before any RNG draw."""
    if not sparse.is_sparse(x):
        raise TypeError('hals_sparse: x must be a scipy.sparse matrix; use hals')
    check_args('hals_sparse', k=k, sweeps=sweeps, lambda_w=lambda_w, lambda_h=lambda_h, real_lambdas=True)


def hals_sparse(x, k, *, sweeps=1, rescale_start=True, lambda_w=0, lambda_h=0, min_iter=10, max_iter=1000, tol1=1e-3,
                tol2=1e-3, nndsvd_init=(True, 'zero'), device=0):
    """HALS on scipy.sparse input (any format; canonicalised by sparse.normalise, never densified, never modified),
    1 <= k <= 128: the outer iteration of `hals` on x.toarray() -- the W half-step, then the H half-step, each `sweeps`
    projected Gauss-Seidel sweeps with an exact-zero clamp on G = F^T F + 2 lambda I, r = F^T b; a component with
    G_jj = 0 keeps its value -- with r gathered from the non-zeros (csrc/kernels_sparse.hip).  Start, RNG
    draws, `rescale_start`, printed lines, stop rule and history are those of `hals`; the recorded objective is the Euclidean
    one, evaluated in float64 from the non-zeros plus k x k terms, so no float64 referee stands behind the stop rule.
    Returns Results with the Experiment of `hals` (distance_type 'eu')."""
    return _run_sparse(hals_sparse, check=lambda: _check_sparse(x, k, sweeps, lambda_w, lambda_h),
                       prepare=lambda: sparse.normalise(x, k), refusals=ValueError, keep_class=False, masked_engine=False,
                       scale_of=start_scale, calls_of=lambda eng: (eng.hals_sparse_run, eng.hals_sparse_finish),
                       k=k, sweeps=sweeps, rescale_start=rescale_start,
                       lambda_w=lambda_w, lambda_h=lambda_h, min_iter=min_iter, max_iter=max_iter, tol1=tol1, tol2=tol2,
                       nndsvd_init=nndsvd_init, device=device)


def _check_sparse_wide(x, k, sweeps, lambda_w, lambda_h):
    """Every refusal of hals_sparse_wide but the one of the stored values, before any device work and before any RNG draw."""
    if not sparse.is_sparse(x):
        raise TypeError(f'hals_sparse_wide: x must be a scipy.sparse matrix; hals_wide runs dense data with '
                        f'{MAX_K + 1} <= k <= {MAX_K_WIDE}')
    if not (_is_count(k, sparse.MAX_K) and k > MAX_K):
        hint = f'; hals_sparse runs 1 <= k <= {MAX_K}' if _is_count(k, MAX_K) else ''
        raise ValueError(f'hals_sparse_wide: supports {MAX_K + 1} <= k <= {sparse.MAX_K} components (got k = {k!r}){hint}')
    check_args('hals_sparse_wide', sweeps=sweeps, lambda_w=lambda_w, lambda_h=lambda_h, real_lambdas=True)


def hals_sparse_wide(x, k, *, sweeps=1, rescale_start=True, lambda_w=0, lambda_h=0, min_iter=10, max_iter=1000, tol1=1e-3,
                     tol2=1e-3, nndsvd_init=(True, 'zero'), device=0):
    """`hals_sparse` with 129 <= k <= 256 components: the same outer iteration -- the W half-step, then the H half-step, each
    `sweeps` projected Gauss-Seidel sweeps with an exact-zero clamp on G = F^T F + 2 lambda I and r = F^T b gathered from the
    non-zeros; a component with G_jj = 0 keeps its value -- with r gathered into a buffer and the sweeps by the kernel of
    `hals_wide`, which streams the k x k Gram matrix through LDS in row tiles (csrc/kernels_sparse.hip).  Input
    rules (any scipy.sparse format, never densified, never modified), start, RNG draws, `rescale_start`
    (`hals_sparse_wide.last_alpha`), printed lines, the stop rule on the float64 Euclidean objective with no referee, history,
    Results and Experiment('hals', k, 'eu', ...) are those of `hals_sparse`.  Called by name: NMF.factorize('hals') routes sparse
    data to `hals_sparse`, which refuses k > 128."""
    return _run_sparse(hals_sparse_wide, check=lambda: _check_sparse_wide(x, k, sweeps, lambda_w, lambda_h),
                       prepare=lambda: sparse.normalise(x, k), refusals=ValueError, keep_class=False, masked_engine=False,
                       scale_of=start_scale, calls_of=lambda eng: (eng.hals_sparse_wide_run, eng.hals_sparse_wide_finish),
                       k=k, sweeps=sweeps, rescale_start=rescale_start,
                       lambda_w=lambda_w, lambda_h=lambda_h, min_iter=min_iter, max_iter=max_iter, tol1=tol1, tol2=tol2,
                       nndsvd_init=nndsvd_init, device=device)


HalsTransformResults = namedtuple('HalsTransformResults', 'h sweeps obj_history experiment')
TransformExperiment = namedtuple('Experiment', 'method components tol max_sweeps lambda_h')
MAX_SOLVE_SWEEPS = 10000


def _check_transform_factor(name, a, shape=None, who='hals_transform'):
    """A factor the caller hands to hals_transform (or to `who`): 2-D, real, finite, >= 0 (and of `shape`); a float64 copy."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError(f'{who}: {name} must be 2-D (got {a.ndim}-D)')
    if a.dtype == object or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)
                                 or np.issubdtype(a.dtype, np.bool_)):
        raise ValueError(f'{who}: {name} must be a real array')
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f'{who}: {name} has shape {tuple(a.shape)}, expected {tuple(shape)}')
    a = np.array(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError(f'{who}: {name} has an entry that is NaN or infinite')
    if a.size and np.min(a) < 0:
        raise ValueError(f'{who}: {name} has a negative entry')
    return a


def _check_solve_args(who, tol, max_sweeps, lambda_h):
    """The stop rule and the penalty of a fold-in (`who`: hals_transform or hals_transform_dense), in the order tol, max_sweeps,
    lambda_h.  The factors w and h0 go through _check_transform_factor where each front end's order of refusals has them."""
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not 0 <= tol < 1:
        raise ValueError(f'{who}: tol must be a real number with 0 <= tol < 1 (got tol = {tol!r})')
    if not _is_count(max_sweeps, MAX_SOLVE_SWEEPS):
        raise ValueError(f'{who}: max_sweeps must be an integer between 1 and {MAX_SOLVE_SWEEPS} (got max_sweeps = {max_sweeps!r})')
    check_args(who, lambda_h=lambda_h, real_lambdas=True)


def hals_transform(x_new, w, mask=None, *, h0=None, lambda_h=0, tol=1e-4, max_sweeps=200, device=0):
    """Least-squares fold-in: H for new data `x_new` (m x n) against the fixed dictionary `w` (m x k, real, finite, >= 0).

    Without `mask`, `x_new` is scipy.sparse under the rules of `hals_sparse`, 1 <= k <= 128; with `mask`, `x_new` and `mask`
    follow nmf_amd.masked.observed as in `hals_masked`, 1 <= k <= 64.  Nothing of the caller's is modified.  With W fixed a
    column's system depends on x_new and W only (G = W^T W + 2 lambda_h I, r_c = W^T x_c; masked: the sums over the column's
    observed entries), so it is formed once and solved in place (csrc/kernels_sparse.hip): projected
    Gauss-Seidel sweeps from h0[:, c] (`h0`: k x n, real, finite, >= 0; default all zeros -- no RNG draw in any case) until,
    after sweep s, the largest step of that sweep is at most `tol` times the largest component, or `max_sweeps`.  The
    defaults are scikit-learn's for its cd solver.  Returns HalsTransformResults: h float64 k x n; sweeps int32, the sweeps
    each column took; obj_history = [objective(w, h0), objective(w, h)] as `hals_sparse` / `hals_masked` record it;
    experiment ('hals_transform', k, tol, max_sweeps, lambda_h).  Every refusal comes before any device work."""
    if mask is None and not sparse.is_sparse(x_new):
        raise TypeError("hals_transform: dense x_new needs mask=; without a mask x_new must be a scipy.sparse matrix "
                        "(dense data without a mask: nmf_amd.transform.transform(x_new, w, distance_type='eu'))")
    w64 = _check_transform_factor('w', w)
    k = w64.shape[1]
    most = MAX_K if mask is None else MAX_K_MASKED
    if not 1 <= k <= most:
        raise ValueError(f'hals_transform: supports 1 <= k <= {most} components{"" if mask is None else " with a mask"} (w has {k} columns)')
    _check_solve_args('hals_transform', tol, max_sweeps, lambda_h)
    try:
        xs = sparse.normalise(x_new, k) if mask is None else masked.observed(x_new, mask, k)
    except (ValueError, TypeError) as e:
        raise type(e)(f'hals_transform: {e}') from None
    m, n = xs.shape
    if w64.shape[0] != m:
        raise ValueError(f'hals_transform: w has {w64.shape[0]} rows, x_new has {m}')
    h64 = np.zeros((k, n)) if h0 is None else _check_transform_factor('h0', h0, (k, n))
    experiment = TransformExperiment('hals_transform', k, tol, max_sweeps, lambda_h)
    with Engine.for_sparse(xs, k, device=device, masked=mask is not None) as eng:
        eng.set_factors(w64, h64)
        eng.hals_foldin_run(lambda_h, tol, max_sweeps)
        _, h = eng.get_factors()
        sweeps = eng.hals_foldin_sweeps()
        history = [np.float64(v) for v in eng.objectives(0, 2)]
    return HalsTransformResults(h=h, sweeps=sweeps, obj_history=history, experiment=experiment)


def hals_transform_dense(x_new, w, *, h0=None, lambda_h=0, tol=1e-4, max_sweeps=200, device=0):
    """Least-squares fold-in for DENSE new data: H for `x_new` (m x n, dense, real, finite and >= 0 in float32; a zero is data
    and nothing is lifted) against the fixed dictionary `w` (m x k, real, finite, >= 0), 1 <= k <= 128 -- the minimiser the H
    half-step of `hals` works towards, where `transform(x_new, w, distance_type='eu')` takes multiplicative steps.

    Every column shares G = W^T W + 2 lambda_h I and its right-hand side is a column of W^T x_new: the products of the H
    half-step of `hals`, formed once in the engine's arithmetic mode -- ONE pass over x_new -- and then every column is solved
    in place by the sweeps and under the stop rule of `hals_transform` (`h0`, `tol`, `max_sweeps`, `lambda_h` as there; h0
    defaults to all zeros and no RNG draw is made in any case): k x n work that never reads x_new again
    (csrc/kernels_hals.hip, hals_solve_kernel).  Returns HalsTransformResults: h float64 k x n; sweeps
    int32, the sweeps each column took; obj_history = [objective(w, h0), objective(w, h)], each 1/2 ||x_new - w h||^2 in
    float64 on the device (Engine.objective_f64); experiment ('hals_transform', k, tol, max_sweeps, lambda_h).  There is no
    mask= (sparse or masked data: `hals_transform`).  Every refusal comes before any device work."""
    who = 'hals_transform_dense'
    if sparse.is_sparse(x_new):
        raise TypeError(f'{who}: x_new must be a dense array; scipy.sparse data (or dense data with mask=) goes to '
                        'nmf_amd.hals.hals_transform')
    xa = np.asarray(x_new)
    if xa.ndim != 2:
        raise ValueError(f'{who}: x_new must be 2-D (got {xa.ndim}-D)')
    w64 = _check_transform_factor('w', w, who=who)
    m, n = xa.shape
    k = w64.shape[1]
    if w64.shape[0] != m:
        raise ValueError(f'{who}: w has {w64.shape[0]} rows, x_new has {m}')
    if not 1 <= k <= MAX_K:
        raise ValueError(f'{who}: supports 1 <= k <= {MAX_K} components (w has {k} columns)')
    if m < 1 or n < 1:
        raise ValueError(f'{who}: x_new is empty')
    _check_solve_args(who, tol, max_sweeps, lambda_h)
    h64 = np.zeros((k, n)) if h0 is None else _check_transform_factor('h0', h0, (k, n), who=who)
    if not losses.is_real(xa):
        raise ValueError(f'{who}: x_new must be a real array')
    losses.check_f32_image(xa, 'eu', None, label=who)
    experiment = TransformExperiment('hals_transform', k, tol, max_sweeps, lambda_h)
    with Engine.for_data(xa, k, device=device) as eng:
        eng.set_factors(w64, h64)
        eng.hals_foldin_dense_run(lambda_h, tol, max_sweeps)
        _, h = eng.get_factors()
        sweeps = eng.hals_foldin_dense_sweeps()
        history = [np.float64(v) for v in eng.objectives(0, 2)]
    return HalsTransformResults(h=h, sweeps=sweeps, obj_history=history, experiment=experiment)


def masked_start_scale(eng, w0, h0):
    """The least-squares scale of the start over the observed set, alpha = <v, q>_Omega / Sum_Omega q^2 with q = w0 h0, for the
    observed entries a masked engine holds; None unless Sum_Omega q^2 > 0.  The masked objective of (s w0, h0) is the parabola
    1/2 Sum v^2 - s <v, q> + 1/2 s^2 Sum q^2, so three float64 objective passes on the device, a, b, c at s = 0, 1, 2, give
    e = c - 2 b + a = Sum q^2 and d = a - b + e / 2 = <v, q>.  Leaves (w0, h0) set on the engine."""
    w64 = np.asarray(w0, dtype=np.float64)
    h64 = np.asarray(h0, dtype=np.float64)
    eng.set_factors(np.zeros_like(w64), np.zeros_like(h64))
    a = eng.objective_f64()
    eng.set_factors(2.0 * w64, h64)                    # (doubling is exact in float32: the device holds 2 (float) w0)
    c = eng.objective_f64()
    eng.set_factors(w0, h0)
    b = eng.objective_f64()
    e = c - 2.0 * b + a
    if not e > 0:
        return None
    return (a - b + 0.5 * e) / e


def hals_masked(x, k, mask, *, sweeps=1, rescale_start=True, lambda_w=0, lambda_h=0, min_iter=10, max_iter=1000, tol1=1e-3,
                tol2=1e-3, nndsvd_init=(True, 'zero'), device=0):
    """HALS on the observed entries of `x` only, 1 <= k <= 64 (the module docstring's definition; csrc/kernels_sparse.hip,
    DESIGN.md 4.14).  `x` and `mask` follow nmf_amd.masked.observed: dense or scipy.sparse `x`, a boolean, 0 / 1 or sparse
    `mask` of the same shape; neither is modified and `x` is never read outside the mask.  Every refusal comes before any
    device work and before any RNG draw.  Start, RNG draws, printed lines, stop rule and history are those of `hals_sparse` on
    masked.observed(x, mask, k); `rescale_start` multiplies both start factors by sqrt(alpha) of `masked_start_scale`
    (`hals_masked.last_alpha`).  The recorded objective is 1/2 Sum_Omega (x - wh)^2 summed per entry in float64
    (nmf_amd.masked.objective), so no float64 referee stands behind the stop rule.  Returns Results with the Experiment of
    `hals` (distance_type 'eu')."""
    return _run_sparse(hals_masked,
                       check=lambda: check_args('hals_masked', k=k, sweeps=sweeps, lambda_w=lambda_w, lambda_h=lambda_h,
                                                real_lambdas=True, most=MAX_K_MASKED),
                       prepare=lambda: masked.observed(x, mask, k), refusals=(ValueError, TypeError), keep_class=True,
                       masked_engine=True, scale_of=masked_start_scale,
                       calls_of=lambda eng: (eng.hals_masked_run, eng.hals_masked_finish),
                       k=k, sweeps=sweeps, rescale_start=rescale_start,
                       lambda_w=lambda_w, lambda_h=lambda_h, min_iter=min_iter, max_iter=max_iter, tol1=tol1, tol2=tol2,
                       nndsvd_init=nndsvd_init, device=device)
