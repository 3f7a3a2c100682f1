"""float64 numpy statement of MUR with the beta-divergence and automatic relevance determination (tests/test_ard_input.py,
tests/test_gpu_ard.py), written from the definition in DESIGN.md 4.6 on top of tests/beta_ref.py; nothing of it is taken
from the code under test.

X is F x N, q = W H + 1e-9, Om >= 0 optional weights (None: 1 everywhere), phi > 0, a > 0, b > 0, c = F + N + a + 1.

    C(W, H, lambda) = Sum om d_beta(x | q) + phi Sum_k [ (|w_k|_1 + |h_k|_1 + b) / lambda_k + c log lambda_k ]
    lambda_k = (|w_k|_1 + |h_k|_1 + b) / c
    W <- W ( ((Om.X.q^(beta-2)) H^T) / ((Om.q^(beta-1)) H^T + phi / lambda_k) )^gamma        column k uses phi / lambda_k
    H <- H ( (W'^T (Om.X.q^(beta-2))) / (W'^T (Om.q^(beta-1)) + phi / lambda_k) )^gamma      q from W' H, row k, same lambda
    iteration t: W step, H step with lambda_t, then lambda_{t+1} from the new pair; history[t] = C(W_t, H_t, lambda_t)."""
import numpy as np

from beta_ref import _terms, beta_objective, gamma
from oracle import nmf_ref as R
from ref_loop import ref_loop


def ard_c(shape, a):
    return shape[0] + shape[1] + float(a) + 1.0


def ard_lambda(w, h, a, b):
    return (np.sum(np.abs(w), axis=0) + np.sum(np.abs(h), axis=1) + b) / ard_c((w.shape[0], h.shape[1]), a)


def _closed_form(f, num, den, pen, beta):
    d = den + pen
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, f * (num / d) ** gamma(beta), 0.0)


def ard_w_step(x, w, h, lam, beta, phi, om=None):
    num, den = _terms(x, w, h, beta, om)
    return _closed_form(w, num @ h.T, den @ h.T, (phi / lam)[None, :], beta)


def ard_h_step(x, w, h, lam, beta, phi, om=None):
    """Called with the NEW w and the lambda the W step used."""
    num, den = _terms(x, w, h, beta, om)
    return _closed_form(h, w.T @ num, w.T @ den, (phi / lam)[:, None], beta)


def ard_penalty(w, h, lam, phi, a, b):
    norms = np.sum(np.abs(w), axis=0) + np.sum(np.abs(h), axis=1) + b
    return phi * float(np.sum(norms / lam + ard_c((w.shape[0], h.shape[1]), a) * np.log(lam)))


def ard_objective(x, w, h, lam, beta, phi, a, b, om=None):
    return beta_objective(x, w, h, beta, om) + ard_penalty(w, h, lam, phi, a, b)


def ard_relevance(lam, shape, a, b):
    floor = b / ard_c(shape, a)
    return (np.asarray(lam) - floor) / floor


def ard_k_eff(rel, prune_tol=1e-3):
    rel = np.asarray(rel)
    return int(np.sum(rel > prune_tol * rel.max()))


def ard_default_b(x, k, a, om=None):
    x = np.asarray(x, dtype=np.float64)
    if om is None:
        mean = x.mean()
    else:
        live = om > 0
        mean = np.sum(om[live] * x[live]) / np.sum(om[live])
    return float(np.sqrt((a - 1.0) * (a - 2.0) * mean / k))


def ard_mur(x, k, beta, phi, a, b, om=None, *, min_iter=100, max_iter=100000, tol1=1e-5, tol2=1e-5,
            nndsvd_init=(False, "zero"), w0=None, h0=None, rng=np.random):
    """The loop of tests/beta_ref.py:beta_mur (same start factors from the same RNG draws, history[0] for the start, same
    stop rule) on the ARD steps.  trace["lam"]: the lambda of the returned pair."""
    if w0 is None:
        xs = np.asarray(x, dtype=np.float64) if om is None else np.where(np.asarray(om) > 0, x, 0.0)
        w, h = R.start_factors(xs, k, nndsvd_init, rng)
    else:
        w, h = w0.copy(), h0.copy()
    lam = [ard_lambda(w, h, a, b)]                         # lambda travels with the pair: the H step leaves the next one

    def h_step(w, h):
        h = ard_h_step(x, w, h, lam[0], beta, phi, om)
        lam[0] = ard_lambda(w, h, a, b)
        return h

    out = ref_loop(w, h, lambda w, h: ard_w_step(x, w, h, lam[0], beta, phi, om), h_step,
                   lambda w, h: ard_objective(x, w, h, lam[0], beta, phi, a, b, om), min_iter, max_iter, tol1, tol2)
    out.trace["lam"] = lam[0]
    return out
