"""Digest of what the MUR and least-squares front ends return through the public API: one SHA-256 per call.

    python tools/frontend_digest.py > digest.txt

Every case seeds the global numpy RNG, calls mur, mur_pair, mur_ard or transform, and hashes the bytes of every array of
the result (w, h, obj_history, relevance), i, the experiment tuple, the lines printed, the caller's x after the call (the
in-place lift of negative data is behaviour) and the RNG's state after the call (how much was drawn is behaviour).  Each
case runs twice: max_iter=5, where nothing stops, and min_iter=2, max_iter=200, tol2=1e30, where rule 2 fires at the first
tested index and the history is trimmed.  The cases are dense 'eu' (one on negative data), 'kl', 'is' and 'beta' at
beta = -1, 0.5, 2.5, each of them with weights=, mask= with 'eu', 'kl', 'is', scipy.sparse x with 'eu', 'kl', mur_pair,
mur_ard and transform for all four losses, with and without weights= and h0=, on three shapes at which the padding arms
differ; the NNDSVD starts run on the middle shape.  An exception is hashed as its class and message.  Behind them the
least-squares part, on the same shapes with the same two stops: anls and hals with 'eu' and 'kl', hals with sweeps=2,
rescale_start=False and lambdas, hals_sparse, hals_stack with three problems, factorize_grid(x, 'hals') on a 2 x 2 grid and
NMF(x, k).factorize('hals') on dense and sparse x; there the hash also covers last_alpha, last_would_arm and the referee's
walked / confirmed / final_rule.  Behind those (variant_cases) hals_masked, hals_transform on sparse x and with mask=, and
hals_transform_dense on the three shapes, hals_wide and hals_sparse_wide at 300 x 200, k = 160, and one refused call of each
(imported from nmf_amd.hals inside variant_cases).

Two commits that print the same lines hand the library the same inputs in the same order and return what it computed
unchanged: the file is what a change of the Python in front of the kernels that is meant to change nothing is checked
against.  The script imports nmf_amd.mur.mur, mur_pair, nmf_amd.ard.mur_ard, nmf_amd.transform.transform, nmf_amd.anls.anls,
nmf_amd.hals.hals, hals_sparse, hals_stack, nmf_amd.grid.factorize_grid and nmf_amd.nmf.NMF only, so it runs unmodified in a
checkout of another commit; all cases run in one process."""
import contextlib
import hashlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import scipy.sparse as sp

SHAPES = [(127, 1, 3), (300, 200, 20), (257, 130, 64)]
NNDSVD_SHAPE = (300, 200, 20)
STOPS = [("5it", dict(max_iter=5)), ("stop", dict(min_iter=2, max_iter=200, tol2=1e30))]
LOSSES = [("eu", None), ("kl", None), ("is", None), ("beta", -1.0), ("beta", 0.5), ("beta", 2.5)]


def make_inputs(m, n, k, seed):
    """x uniform in [0.05, 1) (strictly positive: 'is' and beta <= 0 need that), weights log-uniform over four decades with
    a tenth of the cells at zero, a 70 % mask, a non-negative dictionary w and a start h0."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.05, 1.0, (m, n))
    om = 10.0 ** rng.uniform(-2.0, 2.0, (m, n))
    om[rng.random((m, n)) < 0.1] = 0
    om[0, 0] = 1.0
    mask = rng.random((m, n)) < 0.7
    mask[0, 0] = True
    return x, om, mask, rng.uniform(0.1, 1.0, (m, k)), rng.uniform(0.1, 1.0, (k, n))


def loss_kw(loss, beta):
    return dict(distance_type=loss) if beta is None else dict(distance_type=loss, beta=beta)


def cases(m, n, k, nndsvd):
    """(name, front end, x, positional arguments after x, keywords); x is the array the call may modify."""
    from nmf_amd.ard import mur_ard
    from nmf_amd.mur import mur, mur_pair
    from nmf_amd.transform import transform
    x, om, mask, w, h0 = make_inputs(m, n, k, seed=4000 + k)
    xs = sp.csr_matrix(np.where(mask, x, 0.0))
    pair = [dict(k=min(k, 64), lambda_w=0.0, lambda_h=0.1), dict(k=max(1, min(k, 64) // 2), lambda_w=0.05, lambda_h=0.0)]
    init = dict(nndsvd_init=(True, 'zero')) if nndsvd else {}
    tag = 'nndsvd ' if nndsvd else ''
    out = []
    if nndsvd:
        out += [('mur eu', mur, x, (k,), dict(distance_type='eu')),
                ('mur wt-kl', mur, x, (k,), dict(distance_type='kl', weights=om)),
                ('mur mask-eu', mur, x, (k,), dict(distance_type='eu', mask=mask)),
                ('mur sparse-kl', mur, xs, (k,), dict(distance_type='kl')),
                ('mur_pair', mur_pair, x, (k, pair), {}),
                ('mur_ard', mur_ard, x, (k,), dict(beta=0.5, phi=0.2)),
                ('mur_ard wt', mur_ard, x, (k,), dict(beta=1.5, phi=0.2, weights=om))]
        return [(tag + name, fn, xx, args, {**kw, **init}) for name, fn, xx, args, kw in out]
    out.append(('mur eu negative', mur, x - 0.3, (k,), dict(distance_type='eu', lambda_w=0.1)))
    for loss, beta in LOSSES:
        name = loss if beta is None else f'beta{beta:g}'
        out.append((f'mur {name}', mur, x, (k,), dict(loss_kw(loss, beta), lambda_h=0.05)))
        out.append((f'mur wt-{name}', mur, x, (k,), dict(loss_kw(loss, beta), weights=om, lambda_w=0.05)))
    for loss in ('eu', 'kl', 'is'):
        out.append((f'mur mask-{loss}', mur, x, (k,), dict(distance_type=loss, mask=mask)))
    for loss in ('eu', 'kl'):
        out.append((f'mur sparse-{loss}', mur, xs, (k,), dict(distance_type=loss, lambda_w=0.02)))
    out.append(('mur_pair', mur_pair, x, (k, pair), {}))
    out.append(('mur_pair negative', mur_pair, x - 0.3, (k, pair), {}))
    out.append(('mur_ard', mur_ard, x, (k,), dict(beta=0.5, phi=0.2)))
    out.append(('mur_ard wt', mur_ard, x, (k,), dict(beta=1.5, phi=0.2, b=0.7, weights=om)))
    for loss, beta in [("eu", None), ("kl", None), ("is", None), ("beta", 0.5)]:
        out.append((f'transform {loss}', transform, x, (w,), dict(loss_kw(loss, beta), lambda_h=0.05)))
        out.append((f'transform wt-{loss} h0', transform, x, (w,), dict(loss_kw(loss, beta), weights=om, h0=h0)))
    return out


def ls_cases(m, n, k, nndsvd):
    """The least-squares part: (name, call, x, positional arguments, keywords, diagnostics); `diagnostics()` is what the front
    end left on itself (last_alpha, last_would_arm, the referee's counters), hashed with the result."""
    from nmf_amd.anls import anls
    from nmf_amd.grid import factorize_grid
    from nmf_amd.hals import hals, hals_sparse, hals_stack
    from nmf_amd.nmf import NMF
    x, om, mask, w, h0 = make_inputs(m, n, k, seed=4000 + k)
    xs = sp.csr_matrix(np.where(mask, x, 0.0))
    stack = [dict(k=max(1, k // 4)), dict(k=max(1, k // 2), lambda_w=0.05), dict(k=max(1, k // 8), lambda_w=0.01, lambda_h=0.1)]

    def referee(fn):
        r = getattr(fn, 'last_referee', None)
        return None if r is None else (r.walked, r.confirmed, r.final_rule)

    def grid(x, ks, **kw):
        return [r for _, r in factorize_grid(x, 'hals', features=ks, lambda_w=(0.0, 0.05), lambda_h=(0.02,), **kw)]

    def nmf_hals(x, k, **kw):
        nmf = NMF(x, k)
        nmf.factorize('hals', **kw)
        return nmf.results
    of_hals = lambda: (getattr(hals, 'last_alpha', None), referee(hals))
    of_sparse = lambda: getattr(hals_sparse, 'last_alpha', None)
    of_stack = lambda: (getattr(hals_stack, 'last_alpha', None), getattr(hals_stack, 'last_would_arm', None))
    out = []
    if nndsvd:
        out += [('anls eu', anls, x, (k,), {}, lambda: referee(anls)),
                ('hals eu', hals, x, (k,), {}, of_hals),
                ('hals_sparse', hals_sparse, xs, (k,), {}, of_sparse),
                ('hals_stack', hals_stack, x, (stack,), {}, of_stack)]
        return [('nndsvd ' + name, fn, xx, args, kw, diag) for name, fn, xx, args, kw, diag in out]
    rand = dict(nndsvd_init=(False, 'zero'))
    for loss in ('eu', 'kl'):
        out.append((f'anls {loss}', anls, x, (k,), dict(rand, distance_type=loss, lambda_h=0.05), lambda: referee(anls)))
        out.append((f'hals {loss}', hals, x, (k,), dict(rand, distance_type=loss, lambda_w=0.05), of_hals))
    out.append(('hals sweeps=2', hals, x, (k,), dict(rand, sweeps=2), of_hals))
    out.append(('hals no rescale', hals, x, (k,), dict(rand, rescale_start=False, lambda_w=0.02, lambda_h=0.05), of_hals))
    out.append(('hals_sparse', hals_sparse, xs, (k,), dict(rand, lambda_h=0.05), of_sparse))
    out.append(('hals_sparse sweeps=2', hals_sparse, xs, (k,), dict(rand, sweeps=2, rescale_start=False), of_sparse))
    out.append(('hals_stack', hals_stack, x, (stack,), dict(rand), of_stack))
    out.append(('hals_stack sweeps=2', hals_stack, x, (stack,), dict(rand, sweeps=2, rescale_start=False), of_stack))
    out.append(('grid hals', grid, x, ((max(1, k // 2), k),), dict(rand), lambda: (of_hals(), of_stack())))
    out.append(('NMF hals', nmf_hals, x, (k,), dict(rand), of_hals))
    out.append(('NMF hals sparse', nmf_hals, xs, (k,), dict(rand), of_sparse))
    return out


WIDE_SHAPE = (300, 200, 160)
SOLVES = [("3sw", dict(tol=0, max_sweeps=3)), ("tol", {})]


def variant_cases(m, n, k):
    """The HALS variants behind hals_stack: (name, call, x, positional arguments, keywords, diagnostics, the two sets of stop
    keywords).  hals_wide and hals_sparse_wide on WIDE_SHAPE; hals_masked, hals_transform (sparse and mask=) and
    hals_transform_dense on SHAPES, the fold-ins under a cap of 3 sweeps at tol = 0 and with their defaults; and one refused
    call of each."""
    from nmf_amd.hals import hals_masked, hals_sparse_wide, hals_transform, hals_transform_dense, hals_wide
    x, om, mask, w, h0 = make_inputs(m, n, k, seed=4000 + k)
    xs = sp.csr_matrix(np.where(mask, x, 0.0))
    rand = dict(nndsvd_init=(False, 'zero'))
    alpha_of = lambda fn: lambda: getattr(fn, 'last_alpha', None)
    if k > 128:
        r = lambda: getattr(hals_wide, 'last_referee', None)
        of_wide = lambda: (getattr(hals_wide, 'last_alpha', None), None if r() is None else (r().walked, r().confirmed, r().final_rule))
        return [('hals_wide', hals_wide, x, (k,), dict(rand, lambda_w=0.05), of_wide, STOPS),
                ('hals_wide sweeps=2', hals_wide, x, (k,), dict(rand, sweeps=2, rescale_start=False, distance_type='kl'), of_wide, STOPS),
                ('hals_wide k=64', hals_wide, x, (64,), dict(rand), of_wide, STOPS[:1]),
                ('hals_sparse_wide', hals_sparse_wide, xs, (k,), dict(rand, lambda_h=0.05), alpha_of(hals_sparse_wide), STOPS),
                ('hals_sparse_wide dense x', hals_sparse_wide, x, (k,), dict(rand), alpha_of(hals_sparse_wide), STOPS[:1])]
    return [('hals_masked', hals_masked, x, (k, mask), dict(rand, lambda_h=0.05), alpha_of(hals_masked), STOPS),
            ('hals_masked sweeps=2', hals_masked, x, (k, mask), dict(rand, sweeps=2, rescale_start=False), alpha_of(hals_masked), STOPS),
            ('hals_masked sweeps=17', hals_masked, x, (k, mask), dict(rand, sweeps=17), alpha_of(hals_masked), STOPS[:1]),
            ('hals_transform', hals_transform, xs, (w,), dict(lambda_h=0.05), None, SOLVES),
            ('hals_transform h0', hals_transform, xs, (w,), dict(h0=h0), None, SOLVES),
            ('hals_transform mask', hals_transform, x, (w, mask), dict(lambda_h=0.05, h0=h0), None, SOLVES),
            ('hals_transform tol=1', hals_transform, xs, (w,), dict(tol=1.0, max_sweeps=0, lambda_h=-1, h0=h0[:, :-1]), None, SOLVES[1:]),
            ('hals_transform_dense', hals_transform_dense, x, (w,), dict(lambda_h=0.05), None, SOLVES),
            ('hals_transform_dense h0', hals_transform_dense, x, (w,), dict(h0=h0), None, SOLVES),
            ('hals_transform_dense cap=0', hals_transform_dense, x, (w,), dict(max_sweeps=0, lambda_h=-1, h0=h0[:, :-1]), None, SOLVES[1:])]


def as_bytes(v):
    if sp.issparse(v):
        return v.data.tobytes() + v.indices.tobytes() + v.indptr.tobytes()
    if isinstance(v, (np.ndarray, list)):
        return np.asarray(v, dtype=None if isinstance(v, np.ndarray) else np.float64).tobytes()
    return repr(v).encode()


def digest(fn, x, args, kw, seed, diagnostics=None):
    """One call on a private copy of x, everything observable hashed."""
    x = x.copy()
    np.random.seed(seed)
    printed = io.StringIO()
    try:
        with contextlib.redirect_stdout(printed):
            res = fn(x, *args, **kw)
        results = res if isinstance(res, list) else [res]          # (mur_pair returns two)
        parts = [as_bytes(v) for r in results for v in r]
        # (a fold-in result has the columns' sweep counts where a run has i)
        note = ' '.join((f'i={r.i}' if hasattr(r, 'i') else f'sweeps<={int(np.max(r.sweeps))}') + f' obj[-1]={r.obj_history[-1]!r}'
                        for r in results)
    except Exception as e:  # noqa: BLE001  (a refusal is an outcome like any other)
        parts, note = [type(e).__name__.encode(), str(e).encode()], f'{type(e).__name__}: {e}'
    parts += [printed.getvalue().encode(), as_bytes(x), np.random.get_state()[1].tobytes()]
    if diagnostics is not None:
        parts.append(repr(diagnostics()).encode())
    sha = hashlib.sha256()
    for p in parts:
        sha.update(len(p).to_bytes(8, 'little') + p)
    return sha.hexdigest(), note


def main():
    for nndsvd, shapes in ((False, SHAPES), (True, [NNDSVD_SHAPE])):
        for m, n, k in shapes:
            for c, (name, fn, x, args, kw) in enumerate(cases(m, n, k, nndsvd)):
                for s, (stop, stop_kw) in enumerate(STOPS):
                    sha, note = digest(fn, x, args, {**kw, **stop_kw}, seed=100 * c + s)
                    print(f'{name:<22} {m}x{n} k={k} {stop:<4}  {sha}  {note}', flush=True)
    for nndsvd, shapes in ((False, SHAPES), (True, [NNDSVD_SHAPE])):             # (behind the lines above, which stay where they were)
        for m, n, k in shapes:
            for c, (name, fn, x, args, kw, diag) in enumerate(ls_cases(m, n, k, nndsvd)):
                for s, (stop, stop_kw) in enumerate(STOPS):
                    sha, note = digest(fn, x, args, {**kw, **stop_kw}, seed=100 * c + s, diagnostics=diag)
                    print(f'{name:<22} {m}x{n} k={k} {stop:<4}  {sha}  {note}', flush=True)
    for m, n, k in SHAPES + [WIDE_SHAPE]:                                        # (and behind those) the later HALS variants
        for c, (name, fn, x, args, kw, diag, stops) in enumerate(variant_cases(m, n, k)):
            for s, (stop, stop_kw) in enumerate(stops):
                sha, note = digest(fn, x, args, {**kw, **stop_kw}, seed=100 * c + s, diagnostics=diag)
                print(f'{name:<22} {m}x{n} k={k} {stop:<4}  {sha}  {note}', flush=True)


if __name__ == '__main__':
    main()
