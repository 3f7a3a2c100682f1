"""float64 numpy statement of MUR with the beta-divergence (tests/test_beta_input.py, tests/test_gpu_beta.py), written
directly from the definition in DESIGN.md 4.5; nothing of it is taken from the code under test.

q = W H + 1e-9, W' the W just updated, Om >= 0 optional weights of X's shape (None: 1 everywhere).  X is read only where
om > 0 (other cells may hold NaN, inf or negative values).

    d_beta(x | q) = (x^beta + (beta-1) q^beta - beta x q^(beta-1)) / (beta (beta-1))        beta not in {0, 1}
                    x log(x / q) - x + q     (log term 0 at x = 0)                          beta = 1
                    x / q - log(x / q) - 1                                                  beta = 0
    gamma = 1 / (2 - beta) for beta < 1,  1 for 1 <= beta <= 2,  1 / (beta - 1) for beta > 2
    W <- W ( ((Om.X.q^(beta-2)) H^T) / ((Om.q^(beta-1)) H^T + lambda_w) )^gamma
    H <- H ( (W'^T (Om.X.q^(beta-2))) / (W'^T (Om.q^(beta-1)) + lambda_h) )^gamma            q from W' H
    a denominator of 0 gives 0;   objective  Sum om d_beta(x | q)

Function shapes as tests/weighted_ref.py."""
import numpy as np

from oracle import nmf_ref as R
from ref_loop import ref_loop

EPS = 1e-9


def gamma(beta):
    if beta < 1:
        return 1.0 / (2.0 - beta)
    if beta <= 2:
        return 1.0
    return 1.0 / (beta - 1.0)


def beta_cells(x, q, beta):
    """d_beta(x | q) per cell."""
    x = np.asarray(x, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    if beta == 0:
        r = x / q
        return r - np.log(r) - 1.0
    if beta == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(x > 0, x * np.log(x / q), 0.0)
        return t - x + q
    return (x ** beta + (beta - 1.0) * q ** beta - beta * x * q ** (beta - 1.0)) / (beta * (beta - 1.0))


def _known(x, om):
    """(x with the zero-weight cells set to 0, om as float64; om None = all ones)."""
    x = np.asarray(x, dtype=np.float64)
    if om is None:
        return x, np.ones(x.shape)
    om = np.asarray(om, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(om > 0, x, 0.0), om


def _terms(x, w, h, beta, om):
    """(num, den): Om.X.q^(beta-2) and Om.q^(beta-1), both 0 where om = 0."""
    xo, om = _known(x, om)
    q = w @ h + EPS
    return om * xo * q ** (beta - 2.0), om * q ** (beta - 1.0)


def _closed_form(f, a, d, lam, beta):
    d = d + lam
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, f * (a / d) ** gamma(beta), 0.0)


def beta_w_step(x, w, h, beta, lam=0.0, om=None):
    num, den = _terms(x, w, h, beta, om)
    return _closed_form(w, num @ h.T, den @ h.T, lam, beta)


def beta_h_step(x, w, h, beta, lam=0.0, om=None):
    """Called with the NEW w, as the reference's H step."""
    num, den = _terms(x, w, h, beta, om)
    return _closed_form(h, w.T @ num, w.T @ den, lam, beta)


def beta_objective(x, w, h, beta, om=None):
    xo, om = _known(x, om)
    live = om > 0
    q = (w @ h + EPS)[live]
    return float(np.sum(om[live] * beta_cells(xo[live], q, beta)))


def beta_mur(x, k, beta, om=None, *, min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5, lambda_w=0.0, lambda_h=0.0,
             nndsvd_init=(False, "zero"), w0=None, h0=None, rng=np.random):
    """The loop of tests/weighted_ref.py:weighted_mur (same start factors from the same RNG draws, obj_history[0] for the
    start, same stop rule) on the beta steps."""
    if w0 is None:
        w, h = R.start_factors(_known(x, om)[0], k, nndsvd_init, rng)
    else:
        w, h = w0.copy(), h0.copy()
    return ref_loop(w, h, lambda w, h: beta_w_step(x, w, h, beta, lambda_w, om), lambda w, h: beta_h_step(x, w, h, beta, lambda_h, om),
                    lambda w, h: beta_objective(x, w, h, beta, om), min_iter, max_iter, tol1, tol2)
