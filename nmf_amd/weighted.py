"""Per-entry weights for MUR: `mur(x, k, weights=...)` fits  Sum omega * loss(x, wh)  on dense data.

Omega >= 0 has the shape of x.  A cell with weight 0 is unknown, not zero: x is never read there (it may hold NaN) and
the device receives 0.  With 0 / 1 weights this is `mask=` on the dense kernels; real-valued weights are, for instance,
inverse variances of heteroscedastic data.  `prepare` validates and returns what is uploaded, `objective` scores
factors under any weights on the host, e.g. held-out cells.  Neither `x` nor `weights` is modified."""
import numpy as np
import scipy.sparse as sp

from . import losses
from . import masked

MAX_K = 128
ROWS = 1024          # rows handled at a time
# whose words a value under positive weight is refused in (losses.WORDING): 'is' speaks as mask= does
CONTEXT = {'eu': 'weighted input', 'kl': 'weighted input', 'is': 'observed', 'beta': 'weighted'}


def _check_weights(weights, shape):
    """The weights as given (bool counts as 0 / 1), validated; returns the array and its float32 image."""
    if sp.issparse(weights):
        raise TypeError('weights must be a dense array of the shape of the data (for a sparse 0 / 1 pattern use mask=)')
    weights = np.asarray(weights)
    if np.issubdtype(weights.dtype, np.complexfloating):
        raise TypeError('weights must be real')
    if not losses.is_real(weights):
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
    if losses.underflows(weights):
        raise ValueError('weights: a positive entry underflows to 0 in float32 (scale the weights: only their ratios, '
                         'and their size against lambda, matter)')
    return weights, w32


def prepare(x, weights, k, distance='eu', beta=None):
    """Validate (x, weights, k) for the loss `distance` ('eu' | 'kl' | 'is' | 'beta' with beta=) and return the two float32 arrays the device
    takes: x with the zero-weight cells set to 0, and the weights.  Where the weight is positive x is held to what `mask=`
    asks of observed entries (nmf_amd.masked): finite and non-negative, with 'is' and 'beta' at beta <= 0 strictly positive
    in float32.  Raises
    ValueError for a bad entry, shape or k (1 <= k <= 128), TypeError for sparse or complex input."""
    losses.check_loss(distance)
    beta = losses.check_beta(distance, beta)
    if sp.issparse(x):
        raise TypeError('weights= needs dense data; for a sparse matrix use mask= (0 / 1 weights on the stored pattern)')
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError('weighted input must be 2-D')
    masked.value_dtype(x)                                            # (TypeError for complex data)
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f'weights= supports 1 <= k <= {MAX_K} components (got k = {k})')
    _, w32 = _check_weights(weights, x.shape)
    live = w32 > 0
    if not live.any():
        raise ValueError('weights: no entry is positive')
    vals = x[live]
    masked.check_values(vals)
    losses.check_f32_image(vals, distance, beta, CONTEXT[distance])
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return np.where(live, x, 0).astype(np.float32), w32


def objective(x, w, h, weights, distance_type='eu', beta=None):
    """The weighted objective in float64 on the host, a block of rows at a time:
        eu  1/2 Sum om (x - wh)^2
        kl  Sum om [x log(x / wh) - x + wh]       (inf / nan log terms -> 0)
        is  Sum om [x / q - log(x / q) - 1],  q = wh + 1e-9       (x > 0 wherever om > 0)
        beta (with beta=b)  Sum om d_b(x | q),  q = wh + 1e-9      (x > 0 wherever om > 0 if b <= 0)
    Cells with weight 0 contribute nothing and x is not read there.  With the training weights it is the objective
    `mur(x, k, weights=...)` records; with other weights (for instance 1 on held-out cells) it scores the fit there."""
    losses.check_loss(distance_type)
    beta = losses.check_beta(distance_type, beta)
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
        if distance_type == 'beta' and beta <= 0 and not np.min(xa) > 0:        # (in float64: nothing is uploaded from here)
            raise ValueError(f"distance_type='beta' (beta={beta}): a scored value is 0 (beta <= 0 needs strictly positive data)")
        if distance_type == 'is':
            masked.check_positive_values(xa)
        s += float(np.sum(oa * losses.cells(distance_type, xa, wh, beta)))
    return s
