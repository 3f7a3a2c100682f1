"""float64 numpy statement of MUR with the Itakura-Saito divergence (tests/test_is_input.py, tests/test_gpu_is.py), written
directly from the definition in DESIGN.md ("Itakura-Saito"); nothing of it is taken from the code under test.

    q = W H + 1e-9
    W <- W sqrt( ((X / q^2) H^T) / ((1 / q) H^T + lambda_w) )
    H <- H sqrt( (W'^T (X / q^2)) / (W'^T (1 / q) + lambda_h) )      W' = the W just updated, q from W' H
    a zero denominator gives 0
    objective  Sum [ x / q - log(x / q) - 1 ]

With a mask M (boolean m x n) every sum runs over the observed cells only, and X is read nowhere else (other cells may
hold NaN, inf or negative values)."""
import numpy as np

from oracle import nmf_ref as R
from ref_loop import ref_loop

EPS = 1e-9


def _quotients(x, w, h, m):
    """(x / q^2, 1 / q), both 0 at unobserved cells."""
    q = w @ h + EPS
    if m is None:
        xv = np.asarray(x, dtype=np.float64)
        return xv / q ** 2, 1.0 / q
    with np.errstate(invalid="ignore"):
        xv = np.where(m, x, 0.0)
    return xv / q ** 2, np.where(m, 1.0 / q, 0.0)


def _update(f, num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        out = f * np.sqrt(num / den)
    return np.where(den > 0, out, 0.0)


def is_w_step(x, w, h, lam=0.0, m=None):
    n2, n1 = _quotients(x, w, h, m)
    return _update(w, n2 @ h.T, n1 @ h.T + lam)


def is_h_step(x, w, h, lam=0.0, m=None):
    """Called with the NEW w."""
    n2, n1 = _quotients(x, w, h, m)
    return _update(h, w.T @ n2, w.T @ n1 + lam)


def is_objective(x, w, h, m=None, block=2048):
    """Sum over the (observed) cells of x / q - log(x / q) - 1, by row blocks."""
    tot = 0.0
    for a in range(0, x.shape[0], block):
        b = min(x.shape[0], a + block)
        q = w[a:b] @ h + EPS
        if m is None:
            r = np.asarray(x[a:b], dtype=np.float64) / q
            tot += float(np.sum(r - np.log(r) - 1.0))
        else:
            mb = m[a:b]
            r = np.asarray(x[a:b], dtype=np.float64)[mb] / q[mb]
            tot += float(np.sum(r - np.log(r) - 1.0))
    return tot


def is_mur(x, k, m=None, *, min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5, lambda_w=0.0, lambda_h=0.0,
           nndsvd_init=(False, "zero"), w0=None, h0=None, rng=np.random):
    """The loop of oracle.nmf_ref.mur (same start factors from the same RNG draws -- with a mask, NNDSVD of x with the
    unobserved cells set to 0 --, obj_history[0] for the start, same stop rule) on the IS steps and objective."""
    if m is not None:
        m = np.asarray(m, dtype=bool)
    if w0 is None:
        with np.errstate(invalid="ignore"):
            start = x if m is None else np.where(m, x, 0.0)
        w, h = R.start_factors(start, k, nndsvd_init, rng)
    else:
        w, h = w0.copy(), h0.copy()
    return ref_loop(w, h, lambda w, h: is_w_step(x, w, h, lambda_w, m), lambda w, h: is_h_step(x, w, h, lambda_h, m),
                    lambda w, h: is_objective(x, w, h, m), min_iter, max_iter, tol1, tol2)
