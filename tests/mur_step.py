"""Element-wise checks of single MUR steps (tests/test_gpu_mur_step.py, tests/test_mur_step_bars.py).

One MUR iteration is a closed-form function of (V, W, H, lambda): oracle/nmf_ref.py:mur_w_step, mur_h_step.  The device
runs s = 1 and s = 2 iterations from the same start; every half-step is compared, element by element, with that function
in float64, fed the exact f32 values the device held before it:

    W_s  against  mur_w_step(V, W_{s-1}, H_{s-1}, W_{s-1} H_{s-1}, lambda_w)
    H_s  against  mur_h_step(V, W_s,     H_{s-1}, W_s H_{s-1},     lambda_h)     (the device's own W_s)

Step 2 reads the bf16 images that the update epilogues of step 1 wrote; step 1 alone cannot see those writes.  The
trajectory tests (||W H - W_ref H_ref|| / ||V||) average a fault confined to a row, a tile or a split range over the whole
matrix; these checks name the element and its 128 x 64 tile."""
import json
import os

import numpy as np

from oracle import nmf_ref as R

NEVER = 10 ** 15            # min_iter that keeps the stop rule off (nmf_amd/mur.py)
TILE_R, TILE_C = 128, 64    # the row block of the split-bf16 product kernels and the 64-column group of their contraction

# Largest |dev - ref| / ref allowed per half-step.  'bf16': the split-bf16 products (three terms hi.hi + lo.hi + hi.lo with f32
# accumulation; kernels_bf16.hip); 'f32': the exact-f32 MFMA kernels and the sparse kernels.  KL chains two products (W H, then
# the quotient times a factor).  Largest measured over tests/test_gpu_mur_step.py on an MI355X (NMFX_RECORD_BARS) / over the
# CPU emulation of the same arithmetic (tests/test_mur_step_bars.py):
#   bf16 eu  2.7e-5 / 2.1e-5        bf16 kl  2.7e-5 / 2.1e-5        f32  2.5e-6 (GPU; the sparse kernels 1.3e-6)
# The KL bar sits at 1e-4 rather than the 2e-4 of the error model: a cross term lost for one row block of plain rows costs KL
# about 1.8e-4 (the CPU emulation), which 2e-4 would let through.  DESIGN.md 2.
BARS = {("bf16", "eu"): 1e-4, ("bf16", "kl"): 1e-4, ("f32", "eu"): 2e-5, ("f32", "kl"): 2e-5}
OBJ_RTOL = 1e-5             # recorded objective vs the float64 objective of the returned factors (tests/test_gpu_fullsize.py)
OBJ_FLOOR = 1e-2            # ... relative to the objective, or to 1e-2 of the data's scale where the fit is nearly exact (k >= m)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def make_inputs(m, n, k, seed, edges=False, dead=False, zeros=False):
    """(V f32, W0, H0 float64 holding f32 values).  V is uniform in [0.05, 1): full rank, so that one step moves every entry
    (planted_matrix starts next to a fixed point).  W0, H0 uniform in [0.1, 1), drawn as f32 so that set_factors rounds
    nothing.  edges (m, n >= 8): an all-zero row and column of V, a row with one non-zero, the last row scaled by 2^12 and
    the last column by 2^-12 (both in the ragged tiles of a ragged shape).  dead: W0's last column zero (a dead component;
    Euclidean only -- the reference's KL update of its H row is 0 / 0).  zeros: exact zeros scattered in W0 and H0."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 1.0, (m, n)).astype(np.float32)
    w0 = rng.uniform(0.1, 1.0, (m, k)).astype(np.float32).astype(np.float64)
    h0 = rng.uniform(0.1, 1.0, (k, n)).astype(np.float32).astype(np.float64)
    if edges:
        if m < 8 or n < 8:
            raise ValueError("edge features need m, n >= 8")
        v[1, :] = 0
        v[:, 2] = 0
        v[3, :] = 0
        v[3, 5] = 0.7
        v[m - 1, :] *= np.float32(2.0 ** 12)
        v[:, n - 1] *= np.float32(2.0 ** -12)
    if dead and k >= 2:
        w0[:, k - 1] = 0
    if zeros and k >= 2:
        w0[rng.random(w0.shape) < 0.01] = 0
        h0[rng.random(h0.shape) < 0.01] = 0
    return v, w0, h0


def split_counts(m, n, k, ncu=256, occ=2):
    """The split configuration a dense handle picks (engine.hip nmfx_create; kernels_bf16.hip nmfx_bf16_prepare), for `ncu`
    CUs and `occ` resident blocks per CU of the exact-f32 phase kernels.  wsplit / hsplit: slabs of the exact-f32 W / H phase;
    bf_wsplit / bt_split: slabs of the split-bf16 W / H phase (128-row blocks of V / V^T); gram_ng_w / gram_ng_h: row blocks
    that share one Gram by-product slab."""
    mp, np_ = -(-m // 128) * 128, -(-n // 128) * 128
    rb, cb = mp // 64, np_ // 64
    ws = min(max(1, (ncu * occ + rb // 2) // rb), max(1, cb // 4))
    hs = min(max(1, (ncu * occ + cb // 2) // cb), rb)
    rbt, cbt = np_ // 128, mp // 64
    hs2 = min(max(1, (ncu + rbt // 2) // rbt), max(1, cbt // 4))
    ws2 = min(max(1, (ncu + (mp // 128) // 2) // (mp // 128)), max(1, (np_ // 64) // 4), ws)
    return dict(wsplit=ws, hsplit=hs, bf_wsplit=ws2, bt_split=hs2,
                gram_ng_w=max(1, min(8, 16 // ws2, mp // 128)), gram_ng_h=max(1, min(4, 16 // hs2, np_ // 128)))


# ---- device runners -------------------------------------------------------------------------------------------------------
def _dist(kind):
    from nmf_amd import _lib as L
    return L.EU if kind == "eu" else L.KL


def _drive(eng, kind, w0, h0, lw, lh, steps):
    """The calls nmf_amd.mur.mur makes, with the stop rule off: {s: (W_s, H_s, recorded objectives 0 .. s)}."""
    dist = _dist(kind)
    out = {}
    for s in steps:
        eng.set_factors(w0, h0)
        eng.mur_run(dist, lw, lh, NEVER, 0, 0, 0, s)
        eng.mur_finish(dist, NEVER, 0, 0, s)
        w, h = eng.get_factors()
        out[s] = (w, h, eng.objectives(0, s + 1))
    return out


def run_dense(v, w0, h0, kind, lw=0.0, lh=0.0, precision=None, steps=(1, 2)):
    """A fresh dense handle on V; precision 'f32' | 'bf16' | None (the handle's default, NMFX_PRECISION).  Returns
    (runs, arithmetic): arithmetic names the bar, 'bf16' where split-bf16 products run (k padded to 64 or 128 with the
    mode on, and the composed path beyond 128 components unless the mode is f32)."""
    from nmf_amd.engine import Engine
    m, n = v.shape
    k = w0.shape[1]
    with Engine(m, n, k) as eng:
        if precision is not None:
            eng.set_precision(precision)
        requested = precision or ("f32" if os.environ.get("NMFX_PRECISION") in ("f32", "fp32") else "bf16")
        arith = "bf16" if eng.precision() == "bf16" or (k > 128 and requested == "bf16") else "f32"
        eng.upload_v(v)
        return _drive(eng, kind, w0, h0, lw, lh, steps), arith


def run_sparse(x, w0, h0, kind, lw=0.0, lh=0.0, steps=(1, 2)):
    """Engine.for_sparse on scipy.sparse `x` (the CSR kernels, exact f32)."""
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    xs = sparse.normalise(x, w0.shape[1])
    with Engine.for_sparse(xs, w0.shape[1]) as eng:
        return _drive(eng, kind, w0, h0, lw, lh, steps)


def run_pair(v, starts, lws, lhs, steps=(1, 2)):
    """Two Euclidean problems stacked into one k = 128 handle (nmfx_mur_pair_run; problem p in columns [64 p, 64 p + k_p)).
    starts = [(W0_p, H0_p)] * 2.  Returns [{s: (W_s, H_s, objectives)}] * 2."""
    from nmf_amd.engine import Engine
    m, n = v.shape
    ks = [w.shape[1] for w, _ in starts]
    w0 = np.zeros((m, 128))
    h0 = np.zeros((128, n))
    for p, (w, h) in enumerate(starts):
        w0[:, 64 * p:64 * p + ks[p]] = w
        h0[64 * p:64 * p + ks[p]] = h
    out = [{}, {}]
    with Engine(m, n, 128) as eng:
        if eng.precision() != "bf16":
            raise RuntimeError("pair mode needs the split-bf16 path")
        eng.upload_v(v)
        for s in steps:
            eng.set_factors(w0, h0)
            eng.mur_pair_run(lws, lhs, NEVER, 0, 0, 0, s)
            eng.mur_pair_finish(NEVER, 0, 0, s)
            for p in (0, 1):
                w, h = eng.pair_get_factors(p, ks[p])
                out[p][s] = (w, h, eng.pair_objectives(p, 0, s + 1))
    return out


# ---- float64 half-steps ---------------------------------------------------------------------------------------------------
def ref_w(kind, v, w, h, lam, block=2048):
    """mur_w_step in float64, by row blocks of V (each row of W_new depends on its own row of V and W only)."""
    out = np.empty_like(w)
    for a in range(0, v.shape[0], block):
        b = min(v.shape[0], a + block)
        vb = np.asarray(v[a:b], dtype=np.float64)
        out[a:b] = R.mur_w_step(kind, vb, w[a:b], h, w[a:b] @ h, lam)
    return out


def ref_h(kind, v, w, h, lam, block=2048):
    """mur_h_step in float64.  Matrices beyond `block` rows: the same formula (nmf/mur.py:36-49) with its two m-long
    contractions summed over row blocks, so that no m x n float64 temporary is formed."""
    m = v.shape[0]
    if m <= block:
        vv = np.asarray(v, dtype=np.float64)
        return R.mur_h_step(kind, vv, w, h, w @ h, lam)
    num = np.zeros_like(h)
    den = np.zeros_like(h)
    for a in range(0, m, block):
        b = min(m, a + block)
        vb = np.asarray(v[a:b], dtype=np.float64)
        wb = w[a:b]
        whb = wb @ h
        if kind == "eu":
            num += wb.T @ vb
            den += wb.T @ whb
        else:
            num += wb.T @ (vb / (whb + R.EPS))
    if kind == "eu":
        return h * num / (den + lam * h + R.EPS)
    c = h * num
    d = np.broadcast_to(w.sum(axis=0)[:, None], h.shape)
    return 2 * c / (d + np.sqrt(d ** 2 + 4 * lam * c))


def objective(kind, v, w, h, block=2048):
    """nmf/utils.py:18-33 in float64 of (w, h), by row blocks."""
    tot = 0.0
    for a in range(0, v.shape[0], block):
        b = min(v.shape[0], a + block)
        tot += float(R.objective(np.asarray(v[a:b], dtype=np.float64), w[a:b] @ h, kind))
    return tot


# ---- comparator -----------------------------------------------------------------------------------------------------------
def _record(label, worst, bar):
    """NMFX_RECORD_BARS=<file> (tests/conftest.py): the maxima go to the same file as the assert_allclose records."""
    path = os.environ.get("NMFX_RECORD_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0], "step": label,
                                 "worst_rel": float(worst), "bar": bar}) + "\n")


def compare(label, dev, ref, bar, record=True):
    """(worst relative error, message or None).  Where ref is exactly 0 the device value must be exactly 0 (an inf error
    otherwise); elsewhere the error is |dev - ref| / ref (positive inputs: no cancellation, so it is well defined); a
    non-finite device value is an inf error.  The message names the worst element, its 128 x 64 tile, how many elements
    are over the bar and how many of them lie in the last, ragged tile row / tile column."""
    dev = np.asarray(dev, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if dev.shape != ref.shape:
        return np.inf, f"{label}: shape {dev.shape} != {ref.shape}"
    if not np.all(np.isfinite(ref)):
        raise ValueError(f"{label}: the float64 reference is not finite (an input outside the comparator's domain)")
    zero = ref == 0
    with np.errstate(all="ignore"):
        rel = np.abs(dev - ref) / np.where(zero, 1.0, np.abs(ref))
    rel = np.where(zero, np.where(dev == 0, 0.0, np.inf), rel)
    rel = np.where(np.isfinite(dev), rel, np.inf)
    worst = float(rel.max()) if rel.size else 0.0
    if record:
        _record(label, worst, bar)
    if worst <= bar:
        return worst, None
    r, c = np.unravel_index(int(np.argmax(rel)), rel.shape)
    over = rel > bar
    rows, cols = rel.shape
    parts = []
    if rows % TILE_R:
        parts.append(f"{int(over[rows // TILE_R * TILE_R:].sum())} in the last, ragged tile row (rows >= {rows // TILE_R * TILE_R})")
    else:
        parts.append("no ragged tile row")
    if cols % TILE_C:
        parts.append(f"{int(over[:, cols // TILE_C * TILE_C:].sum())} in the last, ragged tile column (cols >= {cols // TILE_C * TILE_C})")
    else:
        parts.append("no ragged tile column")
    msg = (f"{label}: max |dev - ref| / ref = {worst:.3e} > bar {bar:.1e} at (row, col) = ({r}, {c}), 128x64 tile "
           f"({r // TILE_R}, {c // TILE_C}): dev {dev[r, c]!r}, ref {ref[r, c]!r}; {int(over.sum())} of {rel.size} elements over "
           f"the bar ({int((over & zero).sum())} of them should be exact zeros); {', '.join(parts)}")
    return worst, msg


def check_steps(kind, v, w0, h0, runs, lw, lh, bar, obj_rtol=OBJ_RTOL, tag=""):
    """Every half-step of runs {1: (W1, H1, obj), 2: (W2, H2, obj)} against its float64 reference conditioned on the
    device's previous iterate (the s = 1 run's (W1, H1) for step 2), and every recorded objective against the float64
    objective of the device's iterates.  Returns {label: worst}; raises AssertionError naming every failure."""
    fails, worst = [], {}

    def judge(label, err, msg):
        worst[label] = err
        if msg:
            fails.append(msg)

    iterate = {0: (w0, h0)}
    for s in sorted(runs):
        ws, hs, _ = runs[s]
        wp, hp = iterate[s - 1]
        judge(f"{tag}W{s}", *compare(f"{tag}W{s}", ws, ref_w(kind, v, wp, hp, lw), bar))
        judge(f"{tag}H{s}", *compare(f"{tag}H{s}", hs, ref_h(kind, v, ws, hp, lh), bar))
        iterate[s] = (ws, hs)
    # the recorded objective comes from an f32 W H: where the fit is nearly exact (k >= m or n) its error is a few f32 ulps of
    # the data's scale (1/2 sum v^2 for eu, sum v for kl), not of the small residual -- measured up to 1.1e-5 of a KL objective
    # at 1e-3 of sum v (127 x 1, k = 40); the floor makes the bar there 1e-7 of the data's scale
    vv = np.asarray(v, dtype=np.float64)
    scale = OBJ_FLOOR * (0.5 * float(np.sum(vv * vv)) if kind == "eu" else float(np.sum(vv)))
    for s, (_, _, hist) in sorted(runs.items()):
        for i in range(s + 1):                      # entry i of the s-step run's history: the objective of iterate i
            want = objective(kind, v, *iterate[i])
            got = float(hist[i])
            rel = abs(got - want) / max(abs(want), scale)
            label = f"{tag}obj[{i}] of the {s}-step run"
            _record(label, rel, obj_rtol)
            judge(label, rel, None if rel <= obj_rtol else
                  f"{label}: recorded {got!r}, float64 of the iterate {want!r}: rel {rel:.3e} > {obj_rtol:.0e}")
    if fails:
        raise AssertionError("\n".join(fails))
    return worst
