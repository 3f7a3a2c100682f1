"""Digest of what the MUR front ends return through the public API: one SHA-256 per call.

    python tools/frontend_digest.py > digest.txt

Every case seeds the global numpy RNG, calls mur, mur_pair, mur_ard or transform, and hashes the bytes of every array of
the result (w, h, obj_history, relevance), i, the experiment tuple, the lines printed, the caller's x after the call (the
in-place lift of negative data is behaviour) and the RNG's state after the call (how much was drawn is behaviour).  Each
case runs twice: max_iter=5, where nothing stops, and min_iter=2, max_iter=200, tol2=1e30, where rule 2 fires at the first
tested index and the history is trimmed.  The cases are dense 'eu' (one on negative data), 'kl', 'is' and 'beta' at
beta = -1, 0.5, 2.5, each of them with weights=, mask= with 'eu', 'kl', 'is', scipy.sparse x with 'eu', 'kl', mur_pair,
mur_ard and transform for all four losses, with and without weights= and h0=, on three shapes at which the padding arms
differ; the NNDSVD starts run on the middle shape.  An exception is hashed as its class and message.

Two commits that print the same lines hand the library the same inputs in the same order and return what it computed
unchanged: the file is what a change of the Python in front of the kernels that is meant to change nothing is checked
against.  The script imports nmf_amd.mur.mur, mur_pair, nmf_amd.ard.mur_ard and nmf_amd.transform.transform only, so it
runs unmodified in a checkout of another commit; all cases run in one process."""
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


def as_bytes(v):
    if sp.issparse(v):
        return v.data.tobytes() + v.indices.tobytes() + v.indptr.tobytes()
    if isinstance(v, (np.ndarray, list)):
        return np.asarray(v, dtype=None if isinstance(v, np.ndarray) else np.float64).tobytes()
    return repr(v).encode()


def digest(fn, x, args, kw, seed):
    """One call on a private copy of x, everything observable hashed."""
    x = x.copy()
    np.random.seed(seed)
    printed = io.StringIO()
    try:
        with contextlib.redirect_stdout(printed):
            res = fn(x, *args, **kw)
        results = res if isinstance(res, list) else [res]          # (mur_pair returns two)
        parts = [as_bytes(v) for r in results for v in r]
        note = ' '.join(f'i={r.i} obj[-1]={r.obj_history[-1]!r}' for r in results)
    except Exception as e:  # noqa: BLE001  (a refusal is an outcome like any other)
        parts, note = [type(e).__name__.encode(), str(e).encode()], f'{type(e).__name__}: {e}'
    parts += [printed.getvalue().encode(), as_bytes(x), np.random.get_state()[1].tobytes()]
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


if __name__ == '__main__':
    main()
