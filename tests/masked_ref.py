"""float64 numpy restatement of masked MUR (tests/test_masked_input.py, tests/test_gpu_masked.py).

M is the observed set (a boolean m x n array), X the data; only X at M is read (other cells may hold NaN, inf or negative
values).  W' is the W just updated, as in oracle/nmf_ref.py:mur (nmf/mur.py:122-123):

    Euclidean  W <- W (M.X) H^T / ((M.(W H)) H^T + lambda_w W + 1e-9)      H <- H W'^T (M.X) / (W'^T (M.(W' H)) + lambda_h H + 1e-9)
    KL         A = W ((M.X / (W H + 1e-9)) H^T), B = M H^T                  C = H (W'^T (M.X / (W' H + 1e-9))), D = W'^T M
               W <- 2 A / (B + sqrt(B^2 + 4 lambda_w A)), 0 where B = 0     H <- 2 C / (D + sqrt(D^2 + 4 lambda_h C)), 0 where D = 0

With M all ones these are oracle.nmf_ref.mur_w_step / mur_h_step, operation for operation (pinned by
tests/test_masked_input.py)."""
import numpy as np

from oracle import nmf_ref as R
from ref_loop import ref_loop


def _observed(x, m):
    with np.errstate(invalid="ignore"):
        return np.where(m, x, 0.0)


def _kl_update(num, den, lam):
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 2 * num / (den + np.sqrt(den ** 2 + 4 * lam * num))
    return np.where(den > 0, out, 0.0)


def masked_w_step(kind, x, m, w, h, lam=0.0):
    wh = w @ h
    xm = _observed(x, m)
    if kind == "eu":
        return w * (xm @ h.T) / (np.where(m, wh, 0.0) @ h.T + lam * w + R.EPS)
    if kind == "kl":
        num = w * (np.where(m, xm / (wh + R.EPS), 0.0) @ h.T)
        den = m.astype(np.float64) @ h.T
        return _kl_update(num, den, lam)
    raise KeyError("Unknown distance type.")


def masked_h_step(kind, x, m, w, h, lam=0.0):
    """Called with the NEW w, as the reference's H step."""
    wh = w @ h
    xm = _observed(x, m)
    if kind == "eu":
        return h * (w.T @ xm) / (w.T @ np.where(m, wh, 0.0) + lam * h + R.EPS)
    if kind == "kl":
        num = h * (w.T @ np.where(m, xm / (wh + R.EPS), 0.0))
        den = w.T @ m.astype(np.float64)
        return _kl_update(num, den, lam)
    raise KeyError("Unknown distance type.")


def masked_objective(kind, x, m, wh):
    """nmf/utils.py:18-33 over the observed cells: 1/2 Sum_M (x - wh)^2, or Sum_M [x log(x / wh) - x + wh] with inf / nan
    log terms set to 0."""
    with np.errstate(all="ignore"):
        if kind == "eu":
            d = np.where(m, x - wh, 0.0)
            return 0.5 * np.sum(d ** 2)
        if kind == "kl":
            xm = _observed(x, m)
            t = xm * np.log(xm / wh)
            t = np.where(t == np.inf, 0, t)
            t = np.where(np.isnan(t), 0, t)
            return np.sum(np.where(m, t - xm + wh, 0.0))
    raise KeyError('Distance type unknown: use "kl" or "eu"')


def masked_mur(x, m, k, *, distance_type="kl", min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5, lambda_w=0.0,
               lambda_h=0.0, nndsvd_init=(False, "zero"), w0=None, h0=None, rng=np.random):
    """The loop of oracle.nmf_ref.mur (same start factors from the same RNG draws -- NNDSVD of x with the unobserved cells
    set to 0 --, same stop rule) on the masked steps and objective."""
    m = np.asarray(m, dtype=bool)
    if w0 is None:
        w, h = R.start_factors(_observed(x, m), k, nndsvd_init, rng)
    else:
        w, h = w0.copy(), h0.copy()
    return ref_loop(w, h, lambda w, h: masked_w_step(distance_type, x, m, w, h, lambda_w),
                    lambda w, h: masked_h_step(distance_type, x, m, w, h, lambda_h),
                    lambda w, h: masked_objective(distance_type, x, m, w @ h), min_iter, max_iter, tol1, tol2)
