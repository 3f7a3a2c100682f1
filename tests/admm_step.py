"""Element-wise checks of single ADMM and AO-ADMM steps (tests/test_gpu_admm_step.py, tests/test_admm_step_bars.py).

The trajectory tests of this family (tests/test_gpu_admm.py, tests/test_gpu_aoadmm.py) compare ||W H - W_ref H_ref|| / ||V|| after 4 to
12 iterations: a fault confined to one 64-row block of a round kernel, one slab of a Gram by-product or a dual updated from a stale
auxiliary stays under that average.  Here the device runs step 1 and step 2 from the same start on one handle, in two calls with the
state read in between (W, H, w_aux, h_aux, dual_w, dual_h through nmfx_get_matrix), and every half-step is compared with the float64
half-step of oracle/nmf_ref.py fed the exact f32 values the device held before it.  The same two steps in ONE call must meet the same
bars against the same reference (not bit equality: ADMM-KL trusts a by-product of its auxiliaries launch inside one call only).

Everything below is written for problems stored as COLUMNS (as tests/anls_step.py): a half-step is (F, D, x, dual) with one problem
per column c of x (k x problems): (F^T F + rho I) aux_c = F^T D_c + rho (x_c + dual_c); x = prox(aux, dual); dual += x - aux.  The H
half is (F, D) = (w_aux | W, V), the W half is (h_aux^T | H^T, V^T) on the transposed factor (oracle: admm_aux_step, aoadmm_ls_block).

ADMM, per half-step (check_half):
    structure   x >= 0 and finite; an exact 0 where the float64 argument of the prox is negative by more than the value bar times the
                problem's scale; dual_new - dual_old - (x - aux) = 0 to TIE_ULPS f32 ulps of the largest operand (ties x, aux and dual of
                one launch together: a dual updated from a stale auxiliary fails here whatever the conditioning)
    residual    (F^T F + rho I) aux_dev - (F^T D + rho (x_prev + dual_prev)) in float64, per problem its largest entry over the largest
                entry of |F|^T |D| + rho (|x_prev| + |dual_prev|): free of the condition number of the system
    values      aux, x, dual against the float64 half-step, per problem relative to the largest reference magnitude of the three
AO-ADMM, per sub-problem (check_block): the inner count and the "break" bit equal the reference's (aoadmm_ls_block); x and its dual
by values and structure as above; with admm_iter = 1 the auxiliary is dual_0 + x - dual_1 and the residual check applies too.

The value and residual bars are not fixed in advance: the solve amplifies the rounding of the products by the condition number of
F^T F + rho I (at most k + 1 for AO-ADMM's rho = trace / k, whatever the Gram matrix allows for ADMM's fixed rho).  Per case they are
10 x the largest deviation of a numpy emulation of the device arithmetic (emulate) from the float64 step on the case's own inputs,
with a floor of FLOOR_ULPS f32 ulps -- a function of the case alone, never of what the device returns (bars_of; proven by
tests/test_admm_step_bars.py)."""
import functools
import os
from collections import namedtuple

import numpy as np
import scipy.linalg as sla

from mur_step import NEVER, OBJ_FLOOR, OBJ_RTOL, _record, make_inputs, objective
from oracle import nmf_ref as R

F32 = np.float32
ULP = 2.0 ** -23
FLOOR_ULPS = 4              # floor of the value and residual bars
TIE_ULPS = 4                # dual_new - dual_old - (x - aux): (dual_old + x) - aux in f32 is two roundings of at most the largest operand
MARGIN = 10.0               # bar = MARGIN x the emulation's largest deviation (the margin of tests/anls_step.py)
STOP_TOL, STOP_CLEAR = 1e-2, 1e-3       # inner stop (ao_admm.py:33-43); its two ratios stay STOP_CLEAR (relative) away from STOP_TOL
L1INF_CLEAR = 1e-3          # |sum(pos) - upper_bound| / upper_bound of every row / column an l1inf operator tests (admm.py:164, 192)


def f32(a):
    return np.asarray(a, dtype=F32).astype(np.float64)


def kp_of(k):
    """k padded as the engine pads it (16, 32, 64, 128; multiples of 128 beyond)."""
    for kp in (16, 32, 64, 128):
        if k <= kp:
            return kp
    return -(-k // 128) * 128


def paths_of(c, ncu=256):
    """Which kernels the shape of an AO-ADMM case reaches with `ncu` CUs (kernels_aoadmm.hip; m, n padded to multiples of 128):
    fused    the speculative fused rounds: admm_iter >= 2 and k <= 128 (ao_fused_enabled); else one launch per round
    cols64   the 64-column form of the fused H-side kernel: np / 64 >= ncu, i.e. n > 64 (ncu - 1) = 16320 (ao_fused_cols_cb)
    rows128  the 128-row form of the fused W-side kernel: kp = 64 and mp / 128 >= ncu, i.e. m > 128 (ncu - 1) = 32640 (ao_fused_rows_rb)
    wraps    more than 64 blocks of 64 rows / columns: the lane-strided norm sums of nrm_table_kernel / ao_inner_finish_kernel wrap
    composed beyond 128 components: one launch per round up to 512 padded components, rhs / solve / prox launches beyond"""
    mp, np_ = -(-c.m // 128) * 128, -(-c.n // 128) * 128
    return dict(fused=c.admm_iter >= 2 and c.k <= 128, cols64=np_ // 64 >= ncu, rows128=kp_of(c.k) == 64 and mp // 128 >= ncu,
                wraps=max(mp, np_) // 64 > 64, composed=c.k > 128)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# family 'admm' | 'ao'; loss 'eu' | 'kl'; arith 'f32' | 'bf16' (set_precision); rho: ADMM's fixed penalty; prox / lambda per side;
# admm_iter: AO-ADMM's inner rounds; edges: mur_step.make_inputs(edges=True) (ADMM: make_case); warm: float64 AO-ADMM steps before the start
Case = namedtuple("Case", "family loss m n k arith rho prox_w lam_w prox_h lam_h admm_iter edges warm", defaults=(0,))


def case_id(c):
    rho = f"-rho{c.rho:g}" if c.family == "admm" else f"-it{c.admm_iter}"
    return (f"{c.family}-{c.loss}-{c.m}x{c.n}-k{c.k}-{c.arith}{rho}-w.{c.prox_w}{c.lam_w:g}-h.{c.prox_h}{c.lam_h:g}" + ("-edges" if c.edges else "") + (f"-warm{c.warm}" if c.warm else ""))


RANKS = (1, 3, 12, 16, 17, 32, 33, 40, 64, 65, 100, 127, 128)      # the scalar prepare kernel (kp <= 32), the blocked f64-MFMA one (64, 128)
PROX_ROT = [("nn", 0.0, "nn", 0.0), ("l1n", 0.05, "l1n", 0.05), ("l2n", 0.05, "l2n", 0.1), ("nn", 0.0, "l1n", 0.05), ("l1n", 0.05, "l2n", 0.05)]


def _admm(loss, m, n, k, arith, rho=1.0, prox=("nn", 0.0, "nn", 0.0), edges=False):
    return Case("admm", loss, m, n, k, arith, rho, prox[0], prox[1], prox[2], prox[3], 0, edges)


def _ao(loss, m, n, k, arith, admm_iter, prox=("nn", 0.0, "nn", 0.0), edges=False, warm=0):
    return Case("ao", loss, m, n, k, arith, 0.0, prox[0], prox[1], prox[2], prox[3], admm_iter, edges, warm)


# designated cases of the speculative fused rounds (expected_paths; tests/test_admm_step_bars.py proves the counts from the reference):
# a start two / three float64 AO-ADMM steps in, lambda = 0.5: the W sub-problems run (8, break), (9, break) -- the first leg of the second
# is continued and cut back -- and (9, break), (10, no break) -- continued to the end
PATH_CASES = (_ao("eu", 70, 60, 16, "f32", 10, ("l1n", 0.5, "l1n", 0.5), warm=2), _ao("eu", 70, 60, 16, "f32", 10, ("l1n", 0.5, "l1n", 0.5), warm=3))


def _cases():
    out = []
    # 1. ADMM, Euclidean: every padding of k at 257 x 200 (ragged against the 128-row / 64-column tiles and the 64-row blocks of the
    # round kernels), the prox operators rotating, rho 1 and 2, both arithmetic modes where k pads to 64 / 128
    for i, k in enumerate(RANKS):
        prox = PROX_ROT[i % len(PROX_ROT)] if k > 1 else PROX_ROT[1]          # (l2n: a second difference needs k >= 2)
        for arith in (("f32",) if k <= 32 else ("f32", "bf16")):
            out.append(_admm("eu", 257, 200, k, arith, 1.0 + (i % 2), prox, edges=True))
    for k in (12, 40):                                                        # the l1inf operators on either side
        arith = "f32" if k <= 32 else "bf16"
        out.append(_admm("eu", 257, 200, k, arith, 1.0, ("l1inf_transpose", 0.05, "l1inf", 0.05)))
        out.append(_admm("eu", 257, 200, k, arith, 2.0, ("l1inf", 0.05, "l1inf_transpose", 0.1)))
    for m, n, k in ((5, 4, 3), (1, 70, 1), (70, 1, 1), (130, 129, 40)):
        out.append(_admm("eu", m, n, k, "bf16" if k > 32 else "f32", 1.0, PROX_ROT[1]))
    for m, n, k in ((384, 320, 130), (384, 320, 160)):                        # beyond 128 components: the composed steps
        out += [_admm("eu", m, n, k, a, 1.0, PROX_ROT[1]) for a in ("bf16", "f32")]
    for k in (12, 16, 40, 160):                                               # 8. rho = 0: the reference's plain np.linalg.solve ('nn' only)
        m, n = (384, 320) if k > 128 else (257, 200)
        out.append(_admm("eu", m, n, k, "f32" if k <= 32 else "bf16", 0.0))
    # 2. ADMM, KL: k padded to 16, 64, 128; the split-bf16 iteration and the exact-f32 one
    for k, prox in ((12, PROX_ROT[1]), (40, PROX_ROT[3]), (100, PROX_ROT[2])):
        for arith in (("f32",) if k <= 32 else ("f32", "bf16")):
            out.append(_admm("kl", 257, 200, k, arith, 1.0 + (k == 40), prox))
    # 3. AO-ADMM, Euclidean: admm_iter 1 (one launch per round), 5 and 10 (the stop inside a sub-problem), nn / l1n with lambda 0 / 0.05
    ao_prox = [("nn", 0.0, "nn", 0.0), ("l1n", 0.05, "l1n", 0.05), ("l1n", 0.0, "nn", 0.0), ("nn", 0.0, "l1n", 0.05)]
    for i, k in enumerate(RANKS):
        for arith in (("f32",) if k <= 32 else ("f32", "bf16")):
            out.append(_ao("eu", 257, 200, k, arith, (5, 10, 1)[i % 3], ao_prox[i % 4], edges=True))
    for k in (16, 40, 128):                                                   # every admm_iter at one rank per padding
        for it in (1, 5, 10):
            out.append(_ao("eu", 257, 200, k, "f32" if k <= 32 else "bf16", it, ao_prox[1]))
    for m, n, k in ((5, 4, 3), (1, 70, 1), (70, 1, 1), (130, 129, 40)):
        out.append(_ao("eu", m, n, k, "bf16" if k > 32 else "f32", 5, ao_prox[1]))
    out += [_ao("eu", 4161, 72, 16, "f32", 10, ao_prox[1]), _ao("eu", 72, 4161, 16, "f32", 10, ao_prox[1]),       # the norm sums wrap
            _ao("eu", 64, 16400, 16, "f32", 5, ao_prox[1]), _ao("eu", 64, 16400, 40, "bf16", 5, ao_prox[1]),      # 64-column fused H side
            _ao("eu", 32700, 72, 40, "bf16", 5, ao_prox[1])]                                                      # 128-row fused W side
    for m, n, k in ((384, 320, 130), (384, 320, 160), (640, 576, 520)):       # beyond 128 components
        out += [_ao("eu", m, n, k, a, 5, ao_prox[1]) for a in (("bf16", "f32") if k < 520 else ("bf16",))]
    # the speculation outcomes the cold starts above do not reach (PATH_CASES): the inner count rises from one sub-problem of W to the next
    out += list(PATH_CASES)
    # 4. AO-ADMM, KL: kp 16, 64, 128, split bf16 and exact f32
    for k in (12, 40, 100):
        for arith in (("f32",) if k <= 32 else ("f32", "bf16")):
            out.append(_ao("kl", 257, 200, k, arith, 5, ao_prox[1]))
    out += [_ao("kl", 384, 320, 160, a, 5, ao_prox[1]) for a in ("bf16", "f32")]      # the composed KL steps (nmfx_generic_aoadmm_kl_run / _phase)
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()

# per-process knobs: (environment, case) run in child processes, one at a time (tests/test_gpu_admm_step.py)
KNOB_CASES = [
    ({"NMFX_AO_FUSED": "0"}, _ao("eu", 384, 320, 100, "bf16", 5, ("l1n", 0.05, "l1n", 0.05))),
    ({"NMFX_AO_HINT": "0"}, _ao("eu", 384, 320, 100, "bf16", 5, ("l1n", 0.05, "l1n", 0.05))),
    ({"NMFX_AO_IMG": "0"}, _ao("eu", 384, 320, 100, "bf16", 5, ("l1n", 0.05, "l1n", 0.05))),
    ({"NMFX_AO_OVERLAP": "0"}, _ao("eu", 384, 320, 100, "bf16", 5, ("l1n", 0.05, "l1n", 0.05))),
    ({"NMFX_SK_WORKERS": "7"}, _ao("eu", 640, 512, 100, "bf16", 5, ("l1n", 0.05, "l1n", 0.05))),
    ({"NMFX_AO_ROWS_RB": "128"}, _ao("eu", 384, 320, 40, "bf16", 5, ("l1n", 0.05, "l1n", 0.05))),
    ({"NMFX_GX_ROUNDS_F32": "1"}, _ao("eu", 384, 320, 160, "bf16", 5, ("l1n", 0.05, "l1n", 0.05))),
    ({"NMFX_KL_BF16": "0"}, _admm("kl", 384, 320, 100, "bf16", 1.0, PROX_ROT[1])),
    ({"NMFX_KL_GATHER": "0"}, _admm("kl", 384, 320, 100, "bf16", 1.0, PROX_ROT[1])),
    ({"NMFX_KL_FUSE": "0"}, _admm("kl", 384, 320, 100, "bf16", 1.0, PROX_ROT[1])),
]


@functools.lru_cache(maxsize=4)
def make_case(c):
    """(V f32, W0, H0 float64 holding f32 values): mur_step.make_inputs (uniform V: full rank, a large residual, so that one step
    moves every entry), the start scaled so that W0 H0 has the mean of V (from the unscaled start the first AO-ADMM sub-problem
    wipes H out and the next Gram system is singular)."""
    v, w0, h0 = make_inputs(c.m, c.n, c.k, 11 + 7 * c.m + 3 * c.n + c.k, edges=c.edges)
    if c.edges and c.family == "admm":
        # ADMM's rho is fixed: with a row of V at 2^12 the Gram matrix of the next h_aux outweighs it by 1e8 and the f32 inverse
        # resolves nothing (the emulation deviates by O(1) from float64: a bar that checks nothing).  The scaled row and column
        # carry 2^2 and 2^-2 here; AO-ADMM, whose rho follows the trace, keeps 2^12 and 2^-12
        v[c.m - 1, :] *= F32(2.0 ** -10)
        v[:, c.n - 1] *= F32(2.0 ** 10)
    s = np.sqrt(0.525 / (0.3025 * c.k))
    w0, h0 = f32(w0 * s), f32(h0 * s)
    vv = np.asarray(v, dtype=np.float64)
    for _ in range(c.warm):                            # (each from zero duals, the iterate rounded to f32: what a handle would start from)
        b = ref_block(w0, vv, h0, np.zeros_like(h0), c.k, c.prox_h, c.lam_h, c.admm_iter)
        h0 = f32(b.x)
        b = ref_block(np.ascontiguousarray(h0.T), np.ascontiguousarray(vv.T), w0.T, np.zeros_like(w0.T), c.k, c.prox_w, c.lam_w, c.admm_iter)
        w0 = f32(b.x.T)
    return v, w0, h0


def operators(c):
    """(P_w, P_h) of prox 'l2n' as nmf_amd.admm.admm hands them to the device (None for another prox)."""
    from nmf_amd.admm import l2n_operator
    return (l2n_operator(c.k, c.rho, c.lam_w) if c.prox_w == "l2n" else None,
            l2n_operator(c.k, c.rho, c.lam_h) if c.prox_h == "l2n" else None)


# ---- float64 references (problems as columns) -------------------------------------------------------------------------------------
def prox_arg(kind, aux, dual, rho, lam):
    """The float64 argument whose positive part prox `kind` returns (None for the l1inf operators: their threshold is data dependent)."""
    if kind == "nn":
        return aux - dual
    if kind == "l1n":
        return aux - dual - lam / rho
    if kind == "l2n":
        from nmf_amd.admm import l2n_operator
        return l2n_operator(aux.shape[0], rho, lam) @ (aux - dual)
    return None


def ref_half(f, d, x, dual, rho, prox, lam):
    """One ADMM half-step in float64: (aux, x_new, dual_new) of oracle admm_aux_step and prox (admm.py:216-230, 117-210, 321-322)."""
    aux = R.admm_aux_step(x, dual, f, d, None, rho, "eu")
    xn = R.prox(prox, aux, dual, rho=rho, lam=lam)
    return aux, xn, dual + xn - aux


def l1inf_margins(prox, aux, dual, rho, lam, upper_bound=1.0):
    """|sum(pos) - upper_bound| / upper_bound of every vector an l1inf operator tests (oracle prox_l1inf: rows, or columns for
    'l1inf_transpose'); empty for another prox."""
    if prox not in ("l1inf", "l1inf_transpose"):
        return np.zeros(0)
    a, u = (aux.T, dual.T) if prox == "l1inf_transpose" else (aux, dual)
    pos = np.maximum(a + u - lam / rho, 0.0)
    return np.abs(pos.sum(axis=1) - upper_bound) / upper_bound


Block = namedtuple("Block", "x dual ran fired aux rho margins")


def ref_block(f, d, x, dual, k, prox, lam, admm_iter, stop_offset=0):
    """oracle aoadmm_ls_block (ao_admm.py:46-68) in float64, keeping what the checks need: the last auxiliary, rho, whether the
    stop test fired and, per round, how far its two ratios were from the tolerance, |ratio / tol - 1| (inf for a ratio that is not
    finite: it compares False).  stop_offset = 1: the stop decided one round late (a planted fault)."""
    g = f.T @ f
    rho = np.trace(g) / k
    chol = sla.cholesky(g + rho * np.eye(g.shape[0]), lower=True)
    b = f.T @ d
    ran, fired, aux, margins, due = 0, False, None, [], None
    for j in range(admm_iter):
        aux = sla.cho_solve((chol, True), b + rho * (x + dual))
        prev = x
        x = R.prox(prox, aux, dual, rho=rho, lam=lam, ragged_raises=False)
        dual = dual + x - aux
        ran = j + 1
        r, s = R.inner_residuals(x, prev, aux, dual)
        margins.append(min(abs(t / STOP_TOL - 1.0) if np.isfinite(t) else np.inf for t in (r, s)))
        if due is None and bool(r < STOP_TOL and s < STOP_TOL):
            due = j + stop_offset
        if due is not None and j >= due:
            fired = True
            break
    return Block(x, dual, ran, fired, aux, rho, margins)


def kl_aux(v, w_aux, h_aux, dual_v):
    """(v_aux, dual_v) behind an ADMM-KL step in float64 (admm.py:311-314)."""
    wh = w_aux @ h_aux
    v_bar = wh - dual_v
    v_aux = 0.5 * ((v_bar - 1) + np.sqrt((v_bar - 1) ** 2 + 4 * v))
    return v_aux, dual_v + v_aux - wh


# ---- comparators ------------------------------------------------------------------------------------------------------------------
def _col_max(*arrays):
    top = np.zeros(arrays[0].shape[1])
    for a in arrays:
        if a.size:
            top = np.maximum(top, np.abs(a).max(axis=0))
    return top


def _worst(label, what, dev, ref, scale, bar, fails, record, orient):
    """Largest |dev - ref| / scale over all entries (inf for a non-finite device value); a failure names the problem and component."""
    with np.errstate(all="ignore"):
        rel = np.abs(dev - ref) / np.where(scale > 0, scale, 1.0)[None, :]
    rel = np.where((scale == 0)[None, :] & (dev != ref), np.inf, rel)
    rel = np.where(np.isfinite(dev), rel, np.inf)
    worst = float(rel.max()) if rel.size else 0.0
    if record:
        _record(f"{label} {what}", worst, bar)
    if not worst <= bar:
        i, c = np.unravel_index(int(np.argmax(rel)), rel.shape)
        per = rel.max(axis=0)
        fails.append(f"{label} [values, {what}]: {orient} {c} (64-block {c // 64}), component {i}: dev {dev[i, c]!r}, ref {ref[i, c]!r}, "
                     f"scale {scale[c]:.4e}: deviation {rel[i, c]:.3e} > bar {bar:.2e}; {int(np.sum(per > bar))} of {per.size} {orient}s over the bar")
    return worst


def residual(f, d, x_prev, dual_prev, aux, rho):
    """Per problem: max |(F^T F + rho I) aux - (F^T D + rho (x_prev + dual_prev))| / max (|F|^T |D| + rho (|x_prev| + |dual_prev|))."""
    g = f.T @ f + rho * np.eye(f.shape[1])
    res = g @ np.where(np.isfinite(aux), aux, 0.0) - (f.T @ d + rho * (x_prev + dual_prev))
    scale = np.abs(f).T @ np.abs(d) + rho * (np.abs(x_prev) + np.abs(dual_prev))
    top = scale.max(axis=0)
    per = np.abs(res).max(axis=0) / np.where(top > 0, top, 1.0)
    per = np.where((top == 0) & (np.abs(res).max(axis=0) > 0), np.inf, per)
    return np.where(np.isfinite(aux).all(axis=0), per, np.inf)


def structure(label, x, arg, scale, bar_v, fails, orient):
    """x >= 0 and finite; exactly 0 where the float64 argument of the prox is below -bar_v * scale."""
    bad = ~np.isfinite(x) | (x < 0)
    if bad.any():
        i, c = np.argwhere(bad)[0]
        fails.append(f"{label} [structure]: {orient} {c}, component {i}: x = {x[i, c]!r} is negative or not finite ({int(bad.sum())} such entries)")
    if arg is not None:
        must = (arg < -bar_v * scale[None, :]) & (x != 0)
        if must.any():
            i, c = np.argwhere(must)[0]
            fails.append(f"{label} [structure]: {orient} {c}, component {i}: x = {x[i, c]!r} where the prox argument is {arg[i, c]:.4e} "
                         f"(scale {scale[c]:.3e}): must be exactly 0 ({int(must.sum())} such entries)")


def dual_tie(label, dual_new, dual_old, x, aux, fails, orient, record=True):
    """dual_new - dual_old - (x - aux) over the largest operand, in f32 ulps."""
    top = np.maximum.reduce([np.abs(dual_new), np.abs(dual_old), np.abs(x), np.abs(aux)])
    with np.errstate(all="ignore"):
        tie = np.abs(dual_new - dual_old - (x - aux)) / np.where(top > 0, top, 1.0) / ULP
    tie = np.where(np.isfinite(tie), tie, np.inf)
    worst = float(tie.max()) if tie.size else 0.0
    if record:
        _record(f"{label} dual tie (ulps)", worst, TIE_ULPS)
    if not worst <= TIE_ULPS:
        i, c = np.unravel_index(int(np.argmax(tie)), tie.shape)
        fails.append(f"{label} [dual tie]: {orient} {c} (64-block {c // 64}), component {i}: dual_new {dual_new[i, c]!r} - dual_old {dual_old[i, c]!r} - "
                     f"(x {x[i, c]!r} - aux {aux[i, c]!r}) is {tie[i, c]:.1f} f32 ulps of the largest operand > {TIE_ULPS}; "
                     f"{int(np.sum(tie.max(axis=0) > TIE_ULPS))} of {tie.shape[1]} {orient}s")
    return worst


def check_half(label, f, d, x_prev, dual_prev, aux, x, dual, rho, prox, lam, bar_v, bar_r, fails, orient="column", record=True, ref=None):
    """One ADMM half-step of the device (aux, x, dual) against float64; appends to `fails`.  Returns the measured maxima."""
    raux, rx, rdual = ref if ref is not None else ref_half(f, d, x_prev, dual_prev, rho, prox, lam)
    scale = _col_max(raux, rx, rdual)
    out = {}
    structure(label, x, prox_arg(prox, raux, dual_prev, rho, lam) if rho > 0 else raux - dual_prev, scale, bar_v, fails, orient)
    out["tie"] = dual_tie(label, dual, dual_prev, x, aux, fails, orient, record)
    per = residual(f, d, x_prev, dual_prev, aux, rho)
    out["residual"] = float(per.max())
    if record:
        _record(f"{label} residual", out["residual"], bar_r)
    if not out["residual"] <= bar_r:
        c = int(np.argmax(per))
        fails.append(f"{label} [residual]: {orient} {c} (64-block {c // 64}): {per[c]:.3e} > bar {bar_r:.2e}; {int(np.sum(per > bar_r))} of {per.size} {orient}s over the bar")
    for what, dv, rf in (("aux", aux, raux), ("x", x, rx), ("dual", dual, rdual)):
        out[what] = _worst(label, what, dv, rf, scale, bar_v, fails, record, orient)
    return out


def check_block(label, f, d, x_prev, dual_prev, x, dual, word, k, prox, lam, admm_iter, bar_v, bar_r, fails, orient="column", record=True):
    """One AO-ADMM sub-problem of the device (x, dual, the inner-count word) against float64 aoadmm_ls_block.  Returns
    (measured maxima, the reference Block)."""
    ref = ref_block(f, d, x_prev, dual_prev, k, prox, lam, admm_iter)
    ran, fired = int(word) & 0xFFFF, (int(word) >> 16) & 1
    out = {}
    if (ran, fired) != (ref.ran, int(ref.fired)):
        fails.append(f"{label} [inner count]: the device ran {ran} rounds (break bit {fired}), float64 {ref.ran} (break {int(ref.fired)}); the reference's "
                     f"ratios stay |ratio / tol - 1| = {', '.join(f'{t:.2e}' for t in ref.margins)} away from the tolerance")
    scale = _col_max(ref.aux, ref.x, ref.dual)
    dual_before = ref.dual - ref.x + ref.aux                   # (the dual the last round's prox saw)
    structure(label, x, prox_arg(prox, ref.aux, dual_before, ref.rho, lam), scale, bar_v, fails, orient)
    if admm_iter == 1:
        aux = dual_prev + x - dual                             # (exact up to the two roundings of the dual update)
        per = residual(f, d, x_prev, dual_prev, aux, ref.rho)
        out["residual"] = float(per.max())
        if record:
            _record(f"{label} residual", out["residual"], bar_r)
        if not out["residual"] <= bar_r:
            c = int(np.argmax(per))
            fails.append(f"{label} [residual]: {orient} {c} (64-block {c // 64}): {per[c]:.3e} > bar {bar_r:.2e}; {int(np.sum(per > bar_r))} of {per.size} {orient}s over the bar")
    for what, dv, rf in (("x", x, ref.x), ("dual", dual, ref.dual)):
        out[what] = _worst(label, what, dv, rf, scale, bar_v, fails, record, orient)
    return out, ref


def check_objectives(label, loss, v, iterates, hist, fails, record=True):
    """obj[s] of the device against the float64 objective of the returned (W_s, H_s) (mur_step.OBJ_RTOL, OBJ_FLOOR)."""
    vv = np.asarray(v, dtype=np.float64)
    floor = OBJ_FLOOR * (0.5 * float(np.sum(vv * vv)) if loss == "eu" else float(np.sum(vv)))
    worst = 0.0
    for s, (w, h) in sorted(iterates.items()):
        with np.errstate(all="ignore"):
            want = objective(loss, v, w, h)
        rel = abs(float(hist[s]) - want) / max(abs(want), floor)
        worst = max(worst, rel)
        if record:
            _record(f"{label} obj[{s}]", rel, OBJ_RTOL)
        if not rel <= OBJ_RTOL:
            fails.append(f"{label} obj[{s}]: recorded {float(hist[s])!r}, float64 of the iterate {want!r}: rel {rel:.3e} > {OBJ_RTOL:.0e}")
    return worst


# ---- the numpy emulation of the device arithmetic -----------------------------------------------------------------------------------
def split2(a):
    """a = hi + lo (+ what two bf16 do not hold), both bf16 by round to nearest even, as f32 arrays."""
    a = np.ascontiguousarray(a, dtype=F32)

    def bf16(x):
        u = x.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(F32)
    hi = bf16(a)
    return hi, bf16(np.ascontiguousarray(a - hi))


def prod(a, b, terms):
    """a @ b as the device forms it: f32-accumulated ('f32'), or the split-bf16 products hi.hi + lo.hi + hi.lo (+ lo.lo: terms = 4)."""
    if terms == "f32":
        return np.asarray(a, F32) @ np.asarray(b, F32)
    ah, al = split2(a)
    bh, bl = split2(b)
    out = ah @ bh + al @ bh + ah @ bl
    return out + al @ bl if terms == 4 else out


def terms_of(c):
    """(Gram terms, right-hand side terms) of the products of a case.  Exact f32 where k pads to 16 / 32 or the mode is f32; split
    bf16 else: ADMM and the KL right-hand sides carry four terms (their result is fed through a Gram system that is not shifted
    by trace / k), AO-ADMM's V-sized products three, its Gram matrices three as a by-product (kp = 64) and four from the images."""
    if c.arith == "f32" or c.k <= 32:
        return "f32", "f32"
    if c.family == "admm" or c.loss == "kl":
        return 4, 4
    return (3 if kp_of(c.k) == 64 else 4), 3


def _minv(g32, rho):
    """The float64 inverse of the f32 Gram matrix + rho I, rounded to f32 (the prepare kernels eliminate in f64)."""
    return np.linalg.inv(g32.astype(np.float64) + rho * np.eye(g32.shape[0])).astype(F32)


def _prox32(prox, aux, dual, rho, lam, op):
    if prox in ("nn", "l1n"):
        shift = F32(lam / rho) if prox == "l1n" else F32(0)
        return np.maximum((aux - dual) - shift, F32(0))
    if prox == "l2n":
        return np.maximum(np.asarray(op, F32) @ (aux - dual), F32(0))
    return R.prox_l1inf(aux, dual, rho, lam, by_columns=(prox == "l1inf_transpose")).astype(F32)


def emu_half(f, d, x, dual, rho, prox, lam, op, terms):
    """One ADMM half-step in the device's arithmetic: f32 state, the products of `terms`, the f64 inverse rounded to f32, the f32
    product with it, prox and dual update in f32.  Returns (aux, x, dual) as float64 holding f32 values."""
    ft = np.ascontiguousarray(np.asarray(f, F32).T)
    g = prod(ft, np.asarray(f, F32), terms[0]).astype(F32)
    b = prod(ft, np.asarray(d, F32), terms[1]).astype(F32)
    x, dual = np.asarray(x, F32), np.asarray(dual, F32)
    aux = _minv(g, rho) @ (b + F32(rho) * (x + dual))
    xn = _prox32(prox, aux, dual, rho, lam, op)
    return aux.astype(np.float64), xn.astype(np.float64), ((dual + xn) - aux).astype(np.float64)


def emu_block(f, d, x, dual, k, prox, lam, admm_iter, terms):
    """One AO-ADMM sub-problem in the device's arithmetic (rho = trace / k in f64 of the f32 Gram matrix; the stop test on f64 sums
    of the f32 values).  Returns a Block of float64 arrays holding f32 values."""
    ft = np.ascontiguousarray(np.asarray(f, F32).T)
    g = prod(ft, np.asarray(f, F32), terms[0]).astype(F32)
    b = prod(ft, np.asarray(d, F32), terms[1]).astype(F32)
    rho = float(np.trace(g.astype(np.float64))) / k
    minv = _minv(g, rho)
    x, dual = np.asarray(x, F32), np.asarray(dual, F32)
    ran, fired, aux = 0, False, None
    for j in range(admm_iter):
        aux = minv @ (b + F32(rho) * (x + dual))
        prev = x
        x = _prox32(prox, aux, dual, rho, lam, None)
        dual = (dual + x) - aux
        ran = j + 1
        if R.inner_stop(*(a.astype(np.float64) for a in (x, prev, aux, dual))):
            fired = True
            break
    return Block(x.astype(np.float64), dual.astype(np.float64), ran, fired, aux.astype(np.float64), rho, [])


# ---- a whole step: the device's (or the emulation's) state before and after, checked half by half --------------------------------------
State = namedtuple("State", "w h w_aux h_aux dual_w dual_h words")        # words: the (H, W) inner-count words of the step (AO-ADMM)


def start_state(c, w0, h0):
    z = np.zeros_like
    return State(w0, h0, w0.copy(), h0.copy(), z(w0), z(h0), (0, 0))       # (admm.py:27-28: w_aux = w, h_aux = h)


class KL:
    """The m x n auxiliaries of the KL loss in float64, replayed from readable state (they cannot be read back): ADMM's (v_aux,
    dual_v) behind step s from the device's (w_aux_s, h_aux_s) (admm.py:311-314).  The replay adds the f32 rounding of an m x n
    array that the device stores and the float64 replay does not round: relative 2^-24 per entry of S = v_aux + dual_v, which
    enters the right-hand side F^T S like any rounding of the products the emulation models (its S is rounded to f32)."""

    def __init__(self, v):
        self.v = np.asarray(v, dtype=np.float64)
        self.v_aux = np.zeros_like(self.v)
        self.dual_v = np.zeros_like(self.v)

    def data(self):
        return self.v_aux + self.dual_v

    def advance(self, w_aux, h_aux):
        self.v_aux, self.dual_v = kl_aux(self.v, w_aux, h_aux, self.dual_v)


def check_admm_step(c, v, prev, new, kl, bars, fails, tag, record=True):
    """Both halves of one ADMM step: H from (h, dual_h, w_aux) of `prev`, W from (w, dual_w) of `prev` and the NEW h_aux of `new`."""
    vv = np.asarray(v, dtype=np.float64)
    dh = vv if kl is None else kl.data()
    out = {}
    out["H"] = check_half(f"{tag} H", prev.w_aux, dh, prev.h, prev.dual_h, new.h_aux, new.h, new.dual_h, c.rho, c.prox_h, c.lam_h,
                          bars["values"], bars["residual"], fails, "column", record)
    if not np.isfinite(new.h_aux).all():               # (the W half is conditioned on the device's new h_aux)
        fails.append(f"{tag} W: not checked, h_aux holds {int((~np.isfinite(new.h_aux)).sum())} values that are not finite")
        return out
    out["W"] = check_half(f"{tag} W", np.ascontiguousarray(new.h_aux.T), np.ascontiguousarray(dh.T), prev.w.T, prev.dual_w.T, new.w_aux.T, new.w.T,
                          new.dual_w.T, c.rho, c.prox_w, c.lam_w, bars["values"], bars["residual"], fails, "row", record)
    if kl is not None:
        kl.advance(new.w_aux, new.h_aux)
    return out


def check_ao_step(c, v, prev, new, bars, fails, tag, record=True):
    """Both sub-problems of one Euclidean AO-ADMM outer step: H from (W, H, dual_h) of `prev`, W from the device's own new H."""
    vv = np.asarray(v, dtype=np.float64)
    out, refs = {}, {}
    out["H"], refs["H"] = check_block(f"{tag} H", prev.w, vv, prev.h, prev.dual_h, new.h, new.dual_h, new.words[0], c.k, c.prox_h, c.lam_h,
                                      c.admm_iter, bars["values"], bars["residual"], fails, "column", record)
    if not np.isfinite(new.h).all():                   # (the W sub-problem is conditioned on the device's new H)
        fails.append(f"{tag} W: not checked, H holds {int((~np.isfinite(new.h)).sum())} values that are not finite")
        return out, refs
    out["W"], refs["W"] = check_block(f"{tag} W", np.ascontiguousarray(new.h.T), np.ascontiguousarray(vv.T), prev.w.T, prev.dual_w.T, new.w.T,
                                      new.dual_w.T, new.words[1], c.k, c.prox_w, c.lam_w, c.admm_iter, bars["values"], bars["residual"], fails,
                                      "row", record)
    return out, refs


# ---- bars: the emulated two-step trajectory of a case against the float64 step ----------------------------------------------------------
def emulate(c):
    """The emulated states after steps 1 and 2 of a Euclidean or ADMM-KL case: [State, State] (and for KL the emulation's f32 S)."""
    v, w0, h0 = make_case(c)
    pw, ph = operators(c) if c.family == "admm" else (None, None)
    terms = terms_of(c)
    st, out = start_state(c, w0, h0), []
    v32 = np.asarray(v, F32)
    s32, dv32 = np.zeros_like(v32), np.zeros_like(v32)
    for _ in (1, 2):
        data = v32 if c.loss == "eu" else s32
        if c.family == "admm":
            h_aux, h, dual_h = emu_half(st.w_aux, data, st.h, st.dual_h, c.rho, c.prox_h, c.lam_h, ph, terms)
            wa, w, dw = emu_half(h_aux.T, data.T, st.w.T, st.dual_w.T, c.rho, c.prox_w, c.lam_w, pw, terms)
            st = State(w.T.copy(), h, wa.T.copy(), h_aux, dw.T.copy(), dual_h, (0, 0))
            if c.loss == "kl":                           # (admm.py:311-314 in f32, the product w_aux h_aux f32-accumulated)
                wh = np.asarray(st.w_aux, F32) @ np.asarray(st.h_aux, F32)
                vb = wh - dv32
                va = F32(0.5) * ((vb - F32(1)) + np.sqrt((vb - F32(1)) ** 2 + F32(4) * v32))
                dv32 = (dv32 + va) - wh
                s32 = va + dv32
        else:
            bh = emu_block(st.w, data, st.h, st.dual_h, c.k, c.prox_h, c.lam_h, c.admm_iter, terms)
            bw = emu_block(bh.x.T, data.T, st.w.T, st.dual_w.T, c.k, c.prox_w, c.lam_w, c.admm_iter, terms)
            st = State(bw.x.T.copy(), bh.x, st.w_aux, st.h_aux, bw.dual.T.copy(), bh.dual,
                       (bh.ran | (int(bh.fired) << 16), bw.ran | (int(bw.fired) << 16)))
        out.append(st)
    return out


FREE = dict(values=np.inf, residual=np.inf)


def measure(c, states, record=False, bars=FREE, tag=""):
    """Every check of both steps of `states` = [State_1, State_2] (the device's, the emulation's or a planted fault's) from the start
    of case c.  Returns (fails, maxima {step: {half: {check: worst}}}, the float64 reference Blocks of AO-ADMM {step: {half: Block}})."""
    v, w0, h0 = make_case(c)
    fails, maxima, refs = [], {}, {}
    prev = start_state(c, w0, h0)
    kl = KL(v) if c.loss == "kl" else None
    for s, new in enumerate(states, start=1):
        if c.family == "admm":
            maxima[s] = check_admm_step(c, v, prev, new, kl, bars, fails, f"{tag}step {s}", record)
        else:
            maxima[s], refs[s] = check_ao_step(c, v, prev, new, bars, fails, f"{tag}step {s}", record)
        prev = new
    return fails, maxima, refs


def _largest(maxima, keys):
    return max([h[k] for st in maxima.values() for h in st.values() for k in keys if k in h] or [0.0])


@functools.lru_cache(maxsize=None)
def bars_of(c):
    """{'values', 'residual'}: MARGIN x the emulation's largest deviation over both steps, at least FLOOR_ULPS f32 ulps; with the
    emulation's own figures under 'emu' and the conditions the inputs must meet under 'margins' (tests/test_admm_step_bars.py)."""
    if c.family == "ao" and c.loss == "kl":
        raise ValueError("AO-ADMM-KL: see check_ao_kl")
    states = emulate(c)
    fails, maxima, refs = measure(c, states)
    emu_v, emu_r = _largest(maxima, ("aux", "x", "dual")), _largest(maxima, ("residual",))
    stop = [m for st in refs.values() for b in st.values() for m in b.margins]
    l1 = []
    if c.family == "admm":
        prev = start_state(c, *make_case(c)[1:])
        for new in states:
            if "l1inf" in c.prox_h:                      # (the float64 reference's auxiliaries, fed the emulation's previous state)
                aux = R.admm_aux_step(prev.h, prev.dual_h, prev.w_aux, np.asarray(make_case(c)[0], np.float64), None, c.rho, "eu")
                l1 += list(l1inf_margins(c.prox_h, aux, prev.dual_h, c.rho, c.lam_h))
            if "l1inf" in c.prox_w:
                aux = R.admm_aux_step(prev.w.T, prev.dual_w.T, new.h_aux.T, np.asarray(make_case(c)[0], np.float64).T, None, c.rho, "eu")
                l1 += list(l1inf_margins(c.prox_w, aux, prev.dual_w.T, c.rho, c.lam_w))
            prev = new
    return dict(values=max(MARGIN * emu_v, FLOOR_ULPS * ULP), residual=max(MARGIN * emu_r, FLOOR_ULPS * ULP), emu=(emu_v, emu_r), emu_fails=fails,
                emu_tie=_largest(maxima, ("tie",)), stop_margin=min(stop) if stop else np.inf, l1inf_margin=min(l1) if l1 else np.inf,
                counts={s: {h: (b.ran, b.fired) for h, b in st.items()} for s, st in refs.items()})


def expected_paths(counts, admm_iter, hinted=True):
    """The four counters of nmfx_get_inner_paths after the sub-problems `counts` = [(rounds, fired)] of ONE side in order, by the rule
    of fused_plan (kernels_aoadmm.hip): the first launch runs r1 = the rounds of the side's previous sub-problem if that
    one fired (admm_iter else, and for the first).  [0] the first leg stood (it fired at its last round, or r1 = admm_iter without a
    stop), [1] it was cut back (fired before r1), [2] no stop within r1 < admm_iter, the rest ran and stood, [3] ... and was cut back."""
    out, hint = [0, 0, 0, 0], 0
    for ran, fired in counts:
        r1 = hint if hinted and 0 < hint < admm_iter else admm_iter
        if fired and ran <= r1:
            out[0 if ran >= r1 else 1] += 1
        elif r1 == admm_iter:
            out[0] += 1
        else:
            out[2 if ran >= admm_iter else 3] += 1
        hint = ran if fired else admm_iter
    return tuple(out)


# ---- the device -------------------------------------------------------------------------------------------------------------------
def _codes(c):
    from nmf_amd import _lib as L
    return (L.EU if c.loss == "eu" else L.KL), L.PROX[c.prox_w], L.PROX[c.prox_h]


def _read(eng, c, words=(0, 0)):
    w, h = eng.get_factors()
    if c.family == "admm":
        return State(w, h, eng.get_matrix("w_aux"), eng.get_matrix("h_aux"), eng.get_matrix("dual_w"), eng.get_matrix("dual_h"), words)
    return State(w, h, None, None, eng.get_matrix("dual_w"), eng.get_matrix("dual_h"), words)


def _run(eng, c, first, count):
    dist, pw, ph = _codes(c)
    if c.family == "admm":
        eng.admm_run(dist, c.rho, pw, c.lam_w, ph, c.lam_h, NEVER, 0, 0, first, count)
    else:
        eng.aoadmm_run(dist, pw, c.lam_w, ph, c.lam_h, c.admm_iter, NEVER, 0, 0, first, count)
    eng.state()                                        # (raises NmfxError NMFX_E_NOTPD where a prepare kernel refused the system)


def _phase_step(eng, c, j, fused=False):
    """Step j through the row-sharded phase entry points with a world of one (no exchange), in the sequences of tools/entry_digest.py."""
    dist, pw, ph = _codes(c)
    T = (NEVER, 0, 0)
    if c.family == "admm":
        eng.admm_phase_products(dist, c.rho, pw, ph, j)
        eng.admm_phase_update(dist, c.rho, pw, c.lam_w, ph, c.lam_h, *T, j)
    elif c.loss == "eu":
        eng.aoadmm_phase_h_products(j)
        eng.aoadmm_phase_h_solve(ph, c.lam_h, c.admm_iter, *T, j)
        eng.aoadmm_phase_w_products(*T, j)
        if fused:                                      # (all rounds speculatively, then the decision and the repair)
            eng.aoadmm_phase_w_fused(pw, c.lam_w, c.admm_iter)
            eng.aoadmm_phase_w_repair(pw, c.lam_w, c.admm_iter, j)
        else:
            for r in range(c.admm_iter):
                eng.aoadmm_phase_w_round(pw, c.lam_w, r)
            eng.aoadmm_phase_w_close(c.admm_iter, j)
    else:
        for r in range(c.admm_iter):
            eng.aoadmm_kl_phase_h_products(j, r)
            eng.aoadmm_kl_phase_h_round(ph, c.lam_h, r, *T, j)
        eng.aoadmm_kl_phase_h_close(c.admm_iter, *T, j)
        for r in range(c.admm_iter):
            eng.aoadmm_kl_phase_w_round(pw, c.lam_w, r)
        eng.aoadmm_kl_phase_w_close(c.admm_iter, j)
    eng.state()


Device = namedtuple("Device", "states objectives paths single single_objectives single_paths")


def run_device(c, phases=False, single=True):
    """Case c on one handle with the stop rule off: set_factors, run(0, 1), read, run(1, 1) (phases: step 1 through the phase entry
    points instead; phases = 'fused': the W sub-problem through _w_fused / _w_repair), read, finish; then (single) from the same start run(0, 2) in one call.  Returns a Device: the two States, the
    recorded objectives 0 .. 2, the inner-path counters after the second step, and the same of the one-call run (its State only
    after step 2)."""
    from nmf_amd.engine import Engine
    v, w0, h0 = make_case(c)
    with Engine(c.m, c.n, c.k) as eng:
        eng.set_precision(c.arith)
        eng.upload_v(v)
        if c.family == "admm":
            pw, ph = operators(c)
            if pw is not None:
                eng.set_l2n_operator(0, pw)
            if ph is not None:
                eng.set_l2n_operator(1, ph)

        def words():
            return tuple(int(x) for x in eng.inner_counts(0, 2).reshape(-1)) if c.family == "ao" else (0, 0, 0, 0)

        eng.set_factors(w0, h0)
        _run(eng, c, 0, 1)
        first = _read(eng, c)
        if phases:                                     # (closed as nmf_amd.dist closes a row-sharded run)
            _phase_step(eng, c, 1, fused=(phases == "fused"))
            eng.objective_partial()
            eng.mur_finish_b(NEVER, 0, 0, 2)
        else:
            _run(eng, c, 1, 1)
        second = _read(eng, c)
        paths = eng.inner_paths() if c.family == "ao" else (0, 0, 0, 0)
        if not phases:
            eng.aoadmm_finish(NEVER, 0, 0, 2)
        wd = words()
        states = [first._replace(words=wd[0:2]), second._replace(words=wd[2:4])]
        obj = eng.objectives(0, 3)
        one = one_obj = one_paths = None
        if single:
            eng.set_factors(w0, h0)
            _run(eng, c, 0, 2)
            one_paths = eng.inner_paths() if c.family == "ao" else (0, 0, 0, 0)
            eng.aoadmm_finish(NEVER, 0, 0, 2)
            one = _read(eng, c, words()[2:4])
            one_obj = eng.objectives(0, 3)
    return Device(states, obj, paths, one, one_obj, one_paths)


def run_case(c, phases=False, single=True):
    """Run case c on the device and apply every check at the case's bars.  Returns (Device, maxima, reference Blocks); raises
    AssertionError naming every failure."""
    if c.family == "ao" and c.loss == "kl":
        return run_ao_kl(c, phases=phases, single=single)
    bars = bars_of(c)
    dev = run_device(c, phases=phases, single=single)
    tag = case_id(c) + (" phases " if phases else " ")
    fails, maxima, refs = measure(c, dev.states, record=True, bars=bars, tag=tag)
    v, w0, h0 = make_case(c)
    check_objectives(tag.strip(), c.loss, v, {0: (w0, h0), 1: (dev.states[0].w, dev.states[0].h), 2: (dev.states[1].w, dev.states[1].h)},
                     dev.objectives, fails)
    if dev.single is not None:
        # the one-call run: its step 2 against the float64 step fed the two-call form's state after step 1 (step 1 is the same launches)
        f2, m2, _ = measure_second(c, dev.states[0], dev.single, bars, tag + "one call, ")
        fails += f2
        check_objectives(tag + "one call", c.loss, v, {0: (w0, h0), 2: (dev.single.w, dev.single.h)}, dev.single_objectives, fails)
        if c.family == "ao" and dev.single_paths != dev.paths:
            fails.append(f"{tag}inner paths of the one-call run {dev.single_paths} differ from the two calls' {dev.paths}")
    if c.family == "ao" and not fails and not phases:  # (the phase entry points decide from the exchanged table, without the hint)
        fails += path_failures(c, dev, refs, tag)
    if fails:
        raise AssertionError("\n".join(fails))
    return dev, maxima, refs


def measure_second(c, first, second, bars, tag):
    """Step 2 alone: `second` against the float64 step fed `first` (KL: the auxiliaries replayed through step 1)."""
    v, w0, h0 = make_case(c)
    fails = []
    if c.family == "admm":
        kl = None
        if c.loss == "kl":
            kl = KL(v)
            kl.advance(first.w_aux, first.h_aux)
        return fails, {2: check_admm_step(c, v, first, second, kl, bars, fails, tag + "step 2", True)}, {}
    out, refs = check_ao_step(c, v, first, second, bars, fails, tag + "step 2", True)
    return fails, {2: out}, {2: refs}


def path_failures(c, dev, refs, tag):
    """nmfx_get_inner_paths against expected_paths of the reference's counts (the fused rounds only: k <= 128, admm_iter >= 2, and
    not with the knobs that turn them or the hint off)."""
    if not paths_of(c)["fused"] or os.environ.get("NMFX_AO_FUSED") == "0":
        want = (0, 0, 0, 0)
    else:
        hinted = os.environ.get("NMFX_AO_HINT") != "0"
        want = tuple(a + b for a, b in zip(*(expected_paths([(refs[s][side].ran, refs[s][side].fired) for s in (1, 2)], c.admm_iter, hinted)
                                             for side in "HW")))
    if tuple(dev.paths) != want:
        return [f"{tag}inner paths (stood, cut back, continued, continued and cut back) = {tuple(dev.paths)}, the reference's counts "
                f"{ {s: {h: (b.ran, b.fired) for h, b in st.items()} for s, st in refs.items()} } give {want}"]
    return []


# ---- AO-ADMM, KL ------------------------------------------------------------------------------------------------------------------------
KLBlock = namedtuple("KLBlock", "x dual v_aux dual_v ran fired margins")


def ref_kl_block(v, v_aux, dual_v, f, x, dual, k, prox, lam, admm_iter, stall_dual_v=False):
    """oracle aoadmm_kl_block (ao_admm.py:71-101) in float64 with the margins of its stop test.  stall_dual_v: dual_v not advanced (a
    planted fault)."""
    g = f.T @ f
    rho = np.trace(g) / k
    chol = sla.cholesky(g + rho * np.eye(g.shape[0]), lower=True)
    ran, fired, margins = 0, False, []
    for j in range(admm_iter):
        aux = sla.cho_solve((chol, True), f.T @ (v_aux + dual_v) + rho * (x + dual))
        prev = x
        x = R.prox(prox, aux, dual, rho=rho, lam=lam, ragged_raises=False)
        v_bar = f @ aux - dual_v
        v_aux = 0.5 * ((v_bar - 1) + np.sqrt((v_bar - 1) ** 2 + 4 * v))
        dual = dual + x - aux
        if not stall_dual_v:
            dual_v = dual_v + v_aux - f @ aux
        ran = j + 1
        r, s = R.inner_residuals(x, prev, aux, dual)
        margins.append(min(abs(t / STOP_TOL - 1.0) if np.isfinite(t) else np.inf for t in (r, s)))
        if bool(r < STOP_TOL and s < STOP_TOL):
            fired = True
            break
    return KLBlock(x, dual, v_aux, dual_v, ran, fired, margins)


def emu_kl_block(v, v_aux, dual_v, f, x, dual, k, prox, lam, admm_iter, terms):
    """aoadmm_kl_block in f32 (the products of `terms`; F aux f32-accumulated; v_aux, dual_v kept as f32 m x n arrays)."""
    f, x, dual, v = (np.asarray(a, F32) for a in (f, x, dual, v))
    ft = np.ascontiguousarray(f.T)
    g = prod(ft, f, terms[0]).astype(F32)
    rho = float(np.trace(g.astype(np.float64))) / k
    minv = _minv(g, rho)
    ran, fired = 0, False
    for j in range(admm_iter):
        aux = minv @ (prod(ft, v_aux + dual_v, terms[1]).astype(F32) + F32(rho) * (x + dual))
        prev = x
        x = _prox32(prox, aux, dual, rho, lam, None)
        fa = f @ aux
        v_bar = fa - dual_v
        v_aux = F32(0.5) * ((v_bar - F32(1)) + np.sqrt((v_bar - F32(1)) ** 2 + F32(4) * v))
        dual = (dual + x) - aux
        dual_v = (dual_v + v_aux) - fa
        ran = j + 1
        if R.inner_stop(*(a.astype(np.float64) for a in (x, prev, aux, dual))):
            fired = True
            break
    return KLBlock(x.astype(np.float64), dual.astype(np.float64), v_aux, dual_v, ran, fired, [])


def ao_kl_refs(c, v, w0, h0, first):
    """The float64 sub-problems H1, W1, H2 of AO-ADMM-KL conditioned on `first` = the State behind step 1 (the device's or the
    emulation's).  H1 starts from (W0, H0) and the zero v_aux, dual_v.  The m x n auxiliaries cannot be read back, so W1 and H2 take
    them from the float64 replay: W1 = the block on the transposes with the system matrix H_1 of `first` and the auxiliaries the
    float64 H1 left; H2 = the block from (W_1, H_1, dual_h_1) of `first` and the auxiliaries that W1 left.  What the replay adds: the
    device keeps v_aux and dual_v as f32 m x n arrays, the replay in float64 -- 2^-24 relative per entry and round -- and the
    device's auxiliaries behind H1 come from its own aux iterates, within the value bar of the float64 ones; both are part of what
    the emulation (f32 auxiliaries, its own iterates) measures against the same replay, so the bar covers them."""
    vv = np.asarray(v, dtype=np.float64)
    z = np.zeros_like(vv)
    h1 = ref_kl_block(vv, z, z, w0, h0, np.zeros_like(h0), c.k, c.prox_h, c.lam_h, c.admm_iter)
    w1 = ref_kl_block(vv.T, h1.v_aux.T, h1.dual_v.T, np.ascontiguousarray(first.h.T), w0.T, np.zeros_like(w0.T), c.k, c.prox_w, c.lam_w, c.admm_iter)
    h2 = ref_kl_block(vv, w1.v_aux.T, w1.dual_v.T, first.w, first.h, first.dual_h, c.k, c.prox_h, c.lam_h, c.admm_iter)
    return h1, w1, h2


def emulate_ao_kl(c):
    """(State behind step 1, (x, dual, ran, fired) of H2) of the emulation."""
    v, w0, h0 = make_case(c)
    terms = terms_of(c)
    v32 = np.asarray(v, F32)
    z = np.zeros_like(v32)
    h1 = emu_kl_block(v32, z, z, w0, h0, np.zeros_like(h0), c.k, c.prox_h, c.lam_h, c.admm_iter, terms)
    w1 = emu_kl_block(v32.T, h1.v_aux.T, h1.dual_v.T, h1.x.T, w0.T, np.zeros_like(w0.T), c.k, c.prox_w, c.lam_w, c.admm_iter, terms)
    h2 = emu_kl_block(v32, w1.v_aux.T, w1.dual_v.T, w1.x.T, h1.x, h1.dual, c.k, c.prox_h, c.lam_h, c.admm_iter, terms)
    word = lambda b: b.ran | (int(b.fired) << 16)
    first = State(w1.x.T.copy(), h1.x, None, None, w1.dual.T.copy(), h1.dual, (word(h1), word(w1)))
    return first, State(None, h2.x, None, None, None, h2.dual, (word(h2), 0))


def check_ao_kl(c, first, second, bar, fails, tag, record=True):
    """H1, W1 of `first` and H2 of `second` against ao_kl_refs.  Returns (largest deviation, the reference blocks)."""
    v, w0, h0 = make_case(c)
    if not all(np.isfinite(a).all() for a in (first.w, first.h, first.dual_h)):
        fails.append(f"{tag}: not checked, the state behind step 1 holds values that are not finite")
        return np.inf, ()
    refs = ao_kl_refs(c, v, w0, h0, first)
    worst = 0.0
    todo = [("step 1 H", refs[0], first.h, first.dual_h, first.words[0], "column"), ("step 1 W", refs[1], first.w.T, first.dual_w.T, first.words[1], "row")]
    if second is not None:
        todo.append(("step 2 H", refs[2], second.h, second.dual_h, second.words[0], "column"))
    for name, ref, x, d, word, orient in todo:
        ran, fired = int(word) & 0xFFFF, (int(word) >> 16) & 1
        if (ran, fired) != (ref.ran, int(ref.fired)):
            fails.append(f"{tag}{name} [inner count]: {ran} rounds (break bit {fired}), float64 {ref.ran} (break {int(ref.fired)}); the reference's ratios "
                         f"stay {', '.join(f'{t:.2e}' for t in ref.margins)} away from the tolerance")
        scale = _col_max(ref.x, ref.dual)
        structure(f"{tag}{name}", x, None, scale, bar, fails, orient)
        worst = max(worst, _worst(f"{tag}{name}", "x", x, ref.x, scale, bar, fails, record, orient),
                    _worst(f"{tag}{name}", "dual", d, ref.dual, scale, bar, fails, record, orient))
    return worst, refs


@functools.lru_cache(maxsize=None)
def bars_ao_kl(c):
    first, second = emulate_ao_kl(c)
    fails = []
    worst, refs = check_ao_kl(c, first, second, np.inf, fails, "", record=False)
    return dict(values=max(MARGIN * worst, FLOOR_ULPS * ULP), emu=(worst, 0.0), emu_fails=fails, stop_margin=min(m for b in refs for m in b.margins),
                counts=[(b.ran, b.fired) for b in refs])


def run_ao_kl(c, phases=False, single=True):
    """AO-ADMM-KL on the device: outer step 1 checked completely (x, dual, inner count and break bit of both sub-problems), the H
    sub-problem of step 2 with the auxiliaries replayed in float64 (ao_kl_refs), the recorded objectives; the one-call run's H_2 alike."""
    bars = bars_ao_kl(c)
    dev = run_device(c, phases=phases, single=single)
    v, w0, h0 = make_case(c)
    tag = case_id(c) + (" phases " if phases else " ")
    fails = []
    worst, refs = check_ao_kl(c, dev.states[0], dev.states[1], bars["values"], fails, tag)
    check_objectives(tag.strip(), "kl", v, {0: (w0, h0), 1: (dev.states[0].w, dev.states[0].h), 2: (dev.states[1].w, dev.states[1].h)}, dev.objectives, fails)
    if dev.single is not None:
        check_ao_kl(c, dev.states[0], dev.single, bars["values"], fails, tag + "one call, ")
        check_objectives(tag + "one call", "kl", v, {0: (w0, h0), 2: (dev.single.w, dev.single.h)}, dev.single_objectives, fails)
    if fails:
        raise AssertionError("\n".join(fails))
    return dev, worst, refs


# ---- the refusals of the exact-f32 AO-ADMM-KL sections of tools/entry_digest.py ------------------------------------------------------------
DIGEST_KL = dict(prox="l1n", lam=0.1, admm_iter=5, iters=4)     # (admm_family_sections: aoadmm_run(dist, 1, 0.1, 1, 0.1, 5, ...), runs 0..1 and 2..3)


def digest_inputs(k):
    from tools.entry_digest import make_inputs as digest_make_inputs
    v, w0, h0, _, _ = digest_make_inputs(k, seed=5000 + k)
    return v, w0, h0


def kl_refusal_reference(k):
    """The outer iteration at which the float64 AO-ADMM-KL reference raises LinAlgError on the digest's inputs (None: it runs through)."""
    v, w, h = digest_inputs(k)
    vv = np.asarray(v, dtype=np.float64)
    va, dv, dw, dh = np.zeros_like(vv), np.zeros_like(vv), np.zeros_like(w), np.zeros_like(h)
    d = DIGEST_KL
    for i in range(d["iters"]):
        try:
            with np.errstate(all="ignore"):
                b = ref_kl_block(vv, va, dv, w, h, dh, k, d["prox"], d["lam"], d["admm_iter"])
                h, dh = b.x, b.dual
                b = ref_kl_block(vv.T, b.v_aux.T, b.dual_v.T, np.ascontiguousarray(h.T), w.T, dw.T, k, d["prox"], d["lam"], d["admm_iter"])
                w, dw, va, dv = b.x.T.copy(), b.dual.T.copy(), b.v_aux.T.copy(), b.dual_v.T.copy()
        except np.linalg.LinAlgError:
            return i
    return None


def kl_refusal_device(k, precision="f32"):
    """The outer iteration at which the device refuses the same run as not positive definite (None: it runs through), one call per
    outer iteration."""
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    v, w0, h0 = digest_inputs(k)
    d = DIGEST_KL
    with Engine(v.shape[0], v.shape[1], k) as eng:
        eng.set_precision(precision)
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        for i in range(d["iters"]):
            try:
                eng.aoadmm_run(L.KL, L.PROX[d["prox"]], d["lam"], L.PROX[d["prox"]], d["lam"], d["admm_iter"], NEVER, 0, 0, i, 1)
                eng.state()
            except L.NmfxError as e:
                if e.code != L.NMFX_E_NOTPD:
                    raise
                return i
    return None


# ---- large pivots: the Gauss-Jordan kernels on a Gram matrix with entries of 1e7 -----------------------------------------------------
PIVOT_RANKS = (12, 40, 100, 160)   # the scalar kernel (kp 16), the blocked f64-MFMA one (kp 64, 128), its use per diagonal block beyond 128


def pivot_case(k, m=257, n=200, scale=300.0):
    """(V, W0, H0, rho) of one ADMM H half-step whose system W0^T W0 + rho I has diagonal entries of 1e7 and the worst condition
    number AO-ADMM's rho = trace / k allows, k + 1: W0 is rank-1 dominated.  A pivot entry formed as piv - (piv - 1)(1 + 1/piv)
    is wrong by piv^2 eps = 1e-2 here."""
    rng = np.random.default_rng(900 + k)
    v = rng.uniform(0.05, 1.0, (m, n)).astype(F32)
    w0 = f32(scale * (np.outer(rng.uniform(0.5, 1.0, m), rng.uniform(0.5, 1.0, k)) + 1e-3 * rng.uniform(0, 1, (m, k))))
    h0 = f32(rng.uniform(0.1, 1.0, (k, n)))
    return v, w0, h0, float(F32(np.trace(w0.T @ w0) / k))


def gauss_jordan(t, folded=False):
    """The in-place Gauss-Jordan inverse without pivoting in float64, as the prepare kernels eliminate.  folded: row and column p
    folded into the rank-1 update (cv[p] = piv - 1, rv[p] = 1 + 1/piv), the form the kernels had."""
    a = np.array(t, dtype=np.float64)
    for p in range(len(a)):
        piv = a[p, p]
        inv = 1.0 / piv
        rv, cv = a[p] * inv, a[:, p].copy()
        if folded:
            rv[p], cv[p] = 1.0 + inv, piv - 1.0
            a = a - np.outer(cv, rv)
        else:
            new = a - np.outer(cv, rv)
            new[p, :], new[:, p], new[p, p] = rv, -cv * inv, inv
            a = new
    return a


@functools.lru_cache(maxsize=None)
def pivot_bars(k):
    """Value and residual bars of both halves of pivot_case(k) (prox 'nn'): MARGIN x the emulation's deviation, the W half from the
    emulation's own h_aux."""
    v, w0, h0, rho = pivot_case(k)
    vv, zh, zw = np.asarray(v, np.float64), np.zeros_like(h0), np.zeros_like(w0.T)
    terms = ("f32", "f32")
    eh = emu_half(w0, vv, h0, zh, rho, "nn", 0.0, None, terms)
    ew = emu_half(eh[0].T.copy(), vv.T.copy(), w0.T, zw, rho, "nn", 0.0, None, terms)
    fh = check_half("emulation H", w0, vv, h0, zh, *eh, rho, "nn", 0.0, np.inf, np.inf, [], record=False)
    fw = check_half("emulation W", eh[0].T.copy(), vv.T.copy(), w0.T, zw, *ew, rho, "nn", 0.0, np.inf, np.inf, [], "row", record=False)
    worst = lambda key: max(fh[key], fw[key])
    return dict(values=max(MARGIN * max(worst("aux"), worst("x"), worst("dual")), FLOOR_ULPS * ULP), residual=max(MARGIN * worst("residual"), FLOOR_ULPS * ULP))


def check_pivot_half(k, aux, x, dual, tag="", record=True):
    """The H half-step of pivot_case(k) (prox 'nn') against float64 at pivot_bars(k).  Returns (fails, bars)."""
    v, w0, h0, rho = pivot_case(k)
    bars, fails = pivot_bars(k), []
    check_half(f"{tag}pivot k={k} H", w0, np.asarray(v, np.float64), h0, np.zeros_like(h0), aux, x, dual, rho, "nn", 0.0, bars["values"], bars["residual"],
               fails, record=record)
    return fails, bars


def check_pivot_w_half(k, h_aux, aux, x, dual, tag="", record=True):
    """The W half-step behind it (rows as problems; the system h_aux h_aux^T + rho I with the device's h_aux: pivots of rho = 1e7)."""
    v, w0, h0, rho = pivot_case(k)
    bars, fails = pivot_bars(k), []
    check_half(f"{tag}pivot k={k} W", np.ascontiguousarray(h_aux.T), np.ascontiguousarray(np.asarray(v, np.float64).T), w0.T, np.zeros_like(w0.T), aux.T,
               x.T, dual.T, rho, "nn", 0.0, bars["values"], bars["residual"], fails, "row", record)
    return fails


def run_pivot_case(k):
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    v, w0, h0, rho = pivot_case(k)
    with Engine(v.shape[0], v.shape[1], k) as eng:
        eng.set_precision("f32")
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        eng.admm_run(L.EU, rho, L.PROX["nn"], 0.0, L.PROX["nn"], 0.0, NEVER, 0, 0, 0, 1)
        eng.state()
        w, h = eng.get_factors()
        h_aux = eng.get_matrix("h_aux")
        fails, _ = check_pivot_half(k, h_aux, h, eng.get_matrix("dual_h"))
        fails += check_pivot_w_half(k, h_aux, eng.get_matrix("w_aux"), w, eng.get_matrix("dual_w"))
    if fails:
        raise AssertionError("\n".join(fails))
