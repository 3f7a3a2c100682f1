"""The rules of the MUR loss family -- 'eu', 'kl', 'is' and 'beta' with beta= --, stated once: the names and their library
codes, what beta= may be, which loss needs strictly positive data, what the float32 image of the data has to satisfy, and the
per-cell divergence in float64 that the host objectives sum.  mur, masked, weighted, ard, transform and grid import from
here; this module imports none of them."""
import numpy as np

from . import _lib as L

CODES = {'eu': L.EU, 'kl': L.KL, 'is': L.IS, 'beta': L.BETA}
BETA_RANGE = (-1.0, 3.0)          # what float32 carries: q^(beta - 2) x at q = 1e-9
ROWS = 1024                       # rows scanned at a time (no m x n temporaries)


def check_loss(name, known=tuple(CODES)):
    if name not in known:
        raise KeyError('Distance type unknown: use "kl" or "eu"')   # nmf/utils.py:31


def check_beta(distance_type, beta):
    """beta= belongs to distance_type='beta' and to nothing else; returns it as a float (None for the other losses)."""
    if distance_type != 'beta':
        if beta is not None:
            raise ValueError(f"beta= is the parameter of distance_type='beta' (got beta={beta!r} with distance_type={distance_type!r})")
        return None
    if beta is None:
        raise ValueError("distance_type='beta' needs beta= (a number in [-1, 3]; 0, 1 and 2 are the IS, KL and Euclidean losses)")
    try:
        b = float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"distance_type='beta': beta must be a real number (got beta={beta!r})") from None
    if not np.isfinite(b) or not BETA_RANGE[0] <= b <= BETA_RANGE[1]:
        raise ValueError(f"distance_type='beta': beta must be finite and lie in [-1, 3], the range float32 carries (got beta={beta!r})")
    return b


def needs_positive(loss, beta=None):
    """The divergence is undefined at x = 0 for 'is' and for 'beta' with beta <= 0; elsewhere a zero is data."""
    return loss == 'is' or (loss == 'beta' and beta <= 0)


def loss_label(loss, beta=None):
    """How a message names the loss."""
    return f"distance_type='beta' (beta={beta})" if loss == 'beta' else f"distance_type={loss!r}"


def is_real(a):
    """An array of real numbers (boolean counts): not object, string or complex."""
    return bool(np.issubdtype(a.dtype, np.number) or a.dtype == bool) and not np.issubdtype(a.dtype, np.complexfloating)


# ---- the float32 image (the device holds float32: a value is judged by what arrives there) ---------------------------------
def f32_range(a):
    """(lowest, highest) of `a` as float32; NaN if `a` holds one."""
    with np.errstate(over='ignore', under='ignore'):
        return np.float32(np.min(a)), np.float32(np.max(a))


def underflows(a):
    """True if a positive value of `a` is 0 in float32."""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return False
    for r in range(0, a.shape[0], ROWS):
        blk = a[r:r + ROWS]
        with np.errstate(under='ignore', over='ignore'):
            if np.any((blk > 0) & (blk.astype(np.float32) == 0)):
                return True
    return False


# What each context says when a rule of check_f32_image is broken.  A context that has no wording for a rule does not apply
# it: observed and weighted values have been through masked.check_values (finite, >= 0 in float64) before they come here.
WORDING = {
    'dense': dict(
        positive="{label}: {for_beta}the data must be strictly positive in float32 (an entry is <= 0, NaN or below the float32 "
                 "range); it is not lifted by its minimum",
        nonneg="{label}: the data must be non-negative (an entry is negative or NaN); it is not lifted by its minimum",
        underflow="{label}: a positive entry is below the float32 range",
        range="{label}: an entry is infinite or beyond the float32 range"),
    'observed': dict(
        positive="{label}: an observed value is 0, or underflows to 0 in float32 (the Itakura-Saito divergence needs strictly "
                 "positive data; leave such entries out of the mask)",
        range="{label}: an observed value is beyond the float32 range"),
    'weighted': dict(
        positive="{label}: a value under positive weight is 0, or underflows to 0 in float32 (beta <= 0 needs strictly positive "
                 "data; give such cells weight 0)",
        underflow="{label}: a positive value under positive weight is below the float32 range",
        range="{label}: a value under positive weight is beyond the float32 range"),
    'weighted input': dict(
        range="weighted input: a value is beyond the float32 range"),
}


def check_f32_image(vals, loss, beta=None, context='dense', label=None):
    """The float32 image of the data `vals` under `loss`: its minimum > 0 where the loss needs positive data, else >= 0 with
    no positive value underflowing to 0 (a zero is data there), and its maximum finite.  NaN fails the first rule that looks.
    Raises ValueError in the words of `context`; `label` names the caller where that is not the loss."""
    say = WORDING[context]
    names = dict(label=label or loss_label(loss, beta), for_beta='for beta <= 0 ' if loss == 'beta' else '')
    lowest, highest = f32_range(vals)
    if needs_positive(loss, beta):
        if not lowest > 0:                                      # (NaN included)
            raise ValueError(say['positive'].format(**names))
    else:
        if 'nonneg' in say and not lowest >= 0:                 # (NaN included)
            raise ValueError(say['nonneg'].format(**names))
        if 'underflow' in say and underflows(vals):
            raise ValueError(say['underflow'].format(**names))
    if not np.isfinite(highest):
        raise ValueError(say['range'].format(**names))


# ---- the divergence ----------------------------------------------------------------------------------------------------------
def cells(loss, x, wh, beta=None):
    """d(x | wh) per cell in float64, as the device's recorded objective defines it (nmf/utils.py:18-33):
        eu    1/2 (x - wh)^2
        kl    x log(x / wh) - x + wh                       (inf / nan log terms -> 0)
        is    x / q - log(x / q) - 1,  q = wh + 1e-9       (= beta at 0)
        beta  (x^b + (b - 1) q^b - b x q^(b - 1)) / (b (b - 1)),  q = wh + 1e-9;  its limits at b = 0 and b = 1
    'eu' and 'kl' take wh unguarded."""
    if loss == 'eu':
        return 0.5 * (x - wh) ** 2
    if loss == 'kl':
        with np.errstate(divide='ignore', invalid='ignore'):
            t = x * np.log(x / wh)
        t = np.where(t == np.inf, 0, t)
        t = np.where(np.isnan(t), 0, t)
        return t - x + wh
    q = wh + 1e-9
    if loss == 'is' or beta == 0:
        r = x / q
        return r - np.log(r) - 1.0
    if beta == 1:
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.where(x > 0, x * np.log(x / q), 0.0)
        return t - x + q
    return (x ** beta + (beta - 1.0) * q ** beta - beta * x * q ** (beta - 1.0)) / (beta * (beta - 1.0))
