"""float64 numpy statement of MUR with per-entry weights (tests/test_weighted_input.py, tests/test_gpu_weighted.py), written
directly from the definition in DESIGN.md 4.4; nothing of it is taken from the code under test.

Om >= 0 has the shape of X; X is read only where om > 0 (other cells may hold NaN, inf or negative values).  W' is the
W just updated, T = W H:

    eu   W <- W ((Om.X) H^T) / ((Om.T) H^T + lambda_w W + 1e-9)                         1/2 Sum om (x - T)^2
    kl   A = W ((Om.X / (T + 1e-9)) H^T),  B = Om H^T
         W <- 2 A / (B + sqrt(B^2 + 4 lambda_w A)),  0 where B = 0                       Sum om [x log(x / T) - x + T]
    is   q = T + 1e-9,  W <- W sqrt( ((Om.X / q^2) H^T) / ((Om / q) H^T + lambda_w) ),   Sum om [x / q - log(x / q) - 1]
         0 where the denominator is 0
    H likewise with W' and lambda_h.

With Om in {0, 1} these are tests/masked_ref.py and tests/is_ref.py with a mask; with Om = 1 oracle.nmf_ref.mur_w_step /
mur_h_step and the IS rule (pinned by tests/test_weighted_input.py)."""
import numpy as np

from oracle import nmf_ref as R
from ref_loop import ref_loop

EPS = 1e-9


def _known(x, om):
    """(x with the zero-weight cells set to 0, om as float64)."""
    om = np.asarray(om, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(om > 0, x, 0.0), om


def _terms(kind, x, om, w, h):
    """(num, den): the two per-entry quantities of the loss, both 0 where om = 0."""
    xo, om = _known(x, om)
    wh = w @ h
    if kind == "eu":
        return om * xo, om * wh
    if kind == "kl":
        return om * (xo / (wh + EPS)), om
    if kind == "is":
        q = wh + EPS
        return om * (xo / q ** 2), om * (1.0 / q)
    raise KeyError("Unknown distance type.")


def _closed_form(kind, f, a, d, lam):
    """f = the old factor, a / d = the numerator / denominator sums."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "eu":
            return f * a / (d + lam * f + EPS)
        if kind == "kl":
            num = f * a
            return np.where(d > 0, 2 * num / (d + np.sqrt(d ** 2 + 4 * lam * num)), 0.0)
        d = d + lam
        return np.where(d > 0, f * np.sqrt(a / d), 0.0)


def weighted_w_step(kind, x, om, w, h, lam=0.0):
    num, den = _terms(kind, x, om, w, h)
    return _closed_form(kind, w, num @ h.T, den @ h.T, lam)


def weighted_h_step(kind, x, om, w, h, lam=0.0):
    """Called with the NEW w, as the reference's H step."""
    num, den = _terms(kind, x, om, w, h)
    return _closed_form(kind, h, w.T @ num, w.T @ den, lam)


def weighted_objective(kind, x, om, w, h):
    xo, om = _known(x, om)
    live = om > 0
    wh = w @ h
    with np.errstate(all="ignore"):
        if kind == "eu":
            return 0.5 * float(np.sum(np.where(live, om * (xo - wh) ** 2, 0.0)))
        if kind == "kl":
            t = xo * np.log(xo / wh)
            t = np.where(t == np.inf, 0, t)
            t = np.where(np.isnan(t), 0, t)
            return float(np.sum(np.where(live, om * (t - xo + wh), 0.0)))
        if kind == "is":
            r = xo[live] / (wh[live] + EPS)
            return float(np.sum(om[live] * (r - np.log(r) - 1.0)))
    raise KeyError('Distance type unknown: use "kl" or "eu"')


def weighted_mur(x, om, k, *, distance_type="kl", min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5, lambda_w=0.0,
                 lambda_h=0.0, nndsvd_init=(False, "zero"), w0=None, h0=None, rng=np.random):
    """The loop of tests/masked_ref.py:masked_mur (same start factors from the same RNG draws -- NNDSVD, unweighted, of x
    with the zero-weight cells set to 0 --, obj_history[0] for the start, same stop rule) on the weighted steps."""
    if w0 is None:
        w, h = R.start_factors(_known(x, om)[0], k, nndsvd_init, rng)
    else:
        w, h = w0.copy(), h0.copy()
    return ref_loop(w, h, lambda w, h: weighted_w_step(distance_type, x, om, w, h, lambda_w),
                    lambda w, h: weighted_h_step(distance_type, x, om, w, h, lambda_h),
                    lambda w, h: weighted_objective(distance_type, x, om, w, h), min_iter, max_iter, tol1, tol2)
