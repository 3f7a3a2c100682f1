"""Per-entry weights for MUR: `mur(x, k, weights=...)` fits  Sum omega * loss(x, wh)  on dense data.

Omega >= 0 has the shape of x.  A cell with weight 0 is unknown, not zero: x is never read there (it may hold NaN) and
the device receives 0.  With 0 / 1 weights this is `mask=` on the dense kernels; real-valued weights are, for instance,
inverse variances of heteroscedastic data.  `prepare` validates and returns what is uploaded, `objective` scores
factors under any weights on the host, e.g. held-out cells.  Neither `x` nor `weights` is modified."""
import numpy as np
import scipy.sparse as sp

from . import masked

MAX_K = 128
ROWS = 1024          # rows handled at a time


def _check_weights(weights, shape):
    """The weights as given (bool counts as 0 / 1), validated; returns the array and its float32 image."""
    if sp.issparse(weights):
        raise TypeError('weights must be a dense array of the shape of the data (for a sparse 0 / 1 pattern use mask=)')
    weights = np.asarray(weights)
    if np.issubdtype(weights.dtype, np.complexfloating):
        raise TypeError('weights must be real')
    if weights.dtype == object or not (np.issubdtype(weights.dtype, np.number) or weights.dtype == bool):
        raise TypeError('weights must be a real array')
    if tuple(weights.shape) != tuple(shape):
        raise ValueError(f'weights have shape {tuple(weights.shape)}, data has shape {tuple(shape)}')
    if weights.dtype == bool:
        return weights, weights.astype(np.float32)
    if not np.all(np.isfinite(weights)):
        raise ValueError('weights: an entry is NaN or infinite')
    if weights.size and np.min(weights) < 0:
        raise ValueError('weights: an entry is negative')
    with np.errstate(over='ignore', under='ignore'):            # (the device holds float32: judge that image)
        w32 = weights.astype(np.float32)
    if not np.all(np.isfinite(w32)):
        raise ValueError('weights: an entry is beyond the float32 range')
    if np.any((w32 == 0) & (weights > 0)):
        raise ValueError('weights: a positive entry underflows to 0 in float32 (scale the weights: only their ratios, '
                         'and their size against lambda, matter)')
    return weights, w32


def _beta(distance, beta):
    from .mur import check_beta                                 # (one statement of beta's rules)
    return check_beta(distance, beta)


def beta_cells(x, q, beta):
    """d_beta(x | q) per cell in float64: the three-term form, its limits at beta = 0 and 1."""
    if beta == 0:
        r = x / q
        return r - np.log(r) - 1.0
    if beta == 1:
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.where(x > 0, x * np.log(x / q), 0.0)
        return t - x + q
    return (x ** beta + (beta - 1.0) * q ** beta - beta * x * q ** (beta - 1.0)) / (beta * (beta - 1.0))


def prepare(x, weights, k, distance='eu', beta=None):
    """Validate (x, weights, k) for the loss `distance` ('eu' | 'kl' | 'is' | 'beta' with beta=) and return the two float32 arrays the device
    takes: x with the zero-weight cells set to 0, and the weights.  Where the weight is positive x is held to what `mask=`
    asks of observed entries (nmf_amd.masked): finite and non-negative, with 'is' and 'beta' at beta <= 0 strictly positive
    in float32.  Raises
    ValueError for a bad entry, shape or k (1 <= k <= 128), TypeError for sparse or complex input."""
    if distance not in ('eu', 'kl', 'is', 'beta'):
        raise KeyError('Distance type unknown: use "kl" or "eu"')
    beta = _beta(distance, beta)
    if sp.issparse(x):
        raise TypeError('weights= needs dense data; for a sparse matrix use mask= (0 / 1 weights on the stored pattern)')
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError('weighted input must be 2-D')
    masked._dtype(x)                                            # (TypeError for complex data)
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f'weights= supports 1 <= k <= {MAX_K} components (got k = {k})')
    _, w32 = _check_weights(weights, x.shape)
    live = w32 > 0
    if not live.any():
        raise ValueError('weights: no entry is positive')
    vals = x[live]
    masked.check_values(vals)
    if distance == 'is':
        masked.check_positive_values(vals)
    if distance == 'beta':
        _check_beta_values(vals, beta)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        x32 = np.where(live, x, 0).astype(np.float32)
    if not np.all(np.isfinite(x32)):
        raise ValueError('weighted input: a value is beyond the float32 range')
    return x32, w32


def _check_beta_values(vals, beta):
    """The cells under positive weight for the beta-divergence: strictly positive in float32 for beta <= 0; for beta > 0 a
    zero is data, but a positive value must not underflow to one."""
    with np.errstate(over='ignore', under='ignore'):
        v32 = vals.astype(np.float32)
    if beta <= 0 and not np.min(v32) > 0:
        raise ValueError(f"distance_type='beta' (beta={beta}): a value under positive weight is 0, or underflows to 0 in float32 "
                         "(beta <= 0 needs strictly positive data; give such cells weight 0)")
    if np.any((v32 == 0) & (vals > 0)):
        raise ValueError(f"distance_type='beta' (beta={beta}): a positive value under positive weight is below the float32 range")
    if not np.all(np.isfinite(v32)):
        raise ValueError(f"distance_type='beta' (beta={beta}): a value under positive weight is beyond the float32 range")


def objective(x, w, h, weights, distance_type='eu', beta=None):
    """The weighted objective in float64 on the host, a block of rows at a time:
        eu  1/2 Sum om (x - wh)^2
        kl  Sum om [x log(x / wh) - x + wh]       (inf / nan log terms -> 0)
        is  Sum om [x / q - log(x / q) - 1],  q = wh + 1e-9       (x > 0 wherever om > 0)
        beta (with beta=b)  Sum om d_b(x | q),  q = wh + 1e-9      (x > 0 wherever om > 0 if b <= 0)
    Cells with weight 0 contribute nothing and x is not read there.  With the training weights it is the objective
    `mur(x, k, weights=...)` records; with other weights (for instance 1 on held-out cells) it scores the fit there."""
    if distance_type not in ('eu', 'kl', 'is', 'beta'):
        raise KeyError('Distance type unknown: use "kl" or "eu"')
    beta = _beta(distance_type, beta)
    if sp.issparse(x):
        raise TypeError('weights= needs dense data; for a sparse matrix use nmf_amd.masked.objective')
    x = np.asarray(x)
    weights, _ = _check_weights(weights, x.shape)
    w = np.asarray(w, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    s = 0.0
    for a in range(0, x.shape[0], ROWS):
        om = weights[a:a + ROWS].astype(np.float64)
        live = om > 0
        if not live.any():
            continue
        xa = np.asarray(x[a:a + ROWS][live], dtype=np.float64)
        masked.check_values(xa)
        oa = om[live]
        wh = (w[a:a + ROWS] @ h)[live]
        if distance_type == 'eu':
            s += 0.5 * float(np.sum(oa * (xa - wh) ** 2))
        elif distance_type == 'beta':
            if beta <= 0 and not np.min(xa) > 0:
                raise ValueError(f"distance_type='beta' (beta={beta}): a scored value is 0 (beta <= 0 needs strictly positive data)")
            s += float(np.sum(oa * beta_cells(xa, wh + 1e-9, beta)))
        elif distance_type == 'is':
            masked.check_positive_values(xa)
            r = xa / (wh + 1e-9)
            s += float(np.sum(oa * (r - np.log(r) - 1.0)))
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                t = xa * np.log(xa / wh)
            t = np.where(t == np.inf, 0, t)
            t = np.where(np.isnan(t), 0, t)
            s += float(np.sum(oa * (t - xa + wh)))
    return s
