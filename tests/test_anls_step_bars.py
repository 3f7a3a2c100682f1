"""The bars and the input regimes of the problem-by-problem ANLS checks (tests/anls_step.py), proven on the CPU: a numpy
emulation of the device arithmetic passes check A at a third of its bar and defines check B's bar (10 x its own deviation from
the float64 reference), the faults the norm tests cannot see are rejected and named, and the reference alone shows that every
input regime sends its problems to the NNLS kernels it is meant for.

Emulation of one half-step (F, B, lambda): G = F^T F and r = F^T B through test_mur_step_bars.prod (exact-f32 products, or
the four-term split-bf16 products with f32 accumulation that ANLS runs), 2 lambda added to the f32 diagonal, then every problem's passive-set
system -- the support of the float64 solution -- solved in float32 (LAPACK sgesv) for check B's floor and exactly (float64) for
check A, negative results clamped to zero.  Not
reproduced: the MFMA summation order, the pivot order of the elimination kernels, the f64 inverse of the complement kernels
(more accurate than this) and the 1e-6 feasibility slack; the factor 10 between floor and bar is for those."""
import functools
import json
import os

import numpy as np
import pytest

import anls_step as A
from test_mur_step_bars import prod

F = np.float32


# ---- the emulated half-step ---------------------------------------------------------------------------------------------------
def emu_half_step(f, b, lam, support, terms, solve=F):
    """X (k x problems, float64 holding f32 values) of the emulated device arithmetic on the given supports; solve: the type
    the passive-set systems are solved in (float32: the elimination kernels, check B's floor; float64: an exact solve of the
    same f32 system, as the complement kernels come close to, for check A)."""
    k = f.shape[1]
    ft = np.ascontiguousarray(np.asarray(f, F).T)
    g = (prod(ft, np.asarray(f, F), terms=terms) + F(2 * lam) * np.eye(k, dtype=F)).astype(F)
    r = prod(ft, np.asarray(b, F), terms=terms).astype(F)
    out = np.zeros(r.shape, dtype=F)
    g, r = g.astype(solve), r.astype(solve)
    eye = np.eye(k, dtype=bool)
    for a0 in range(0, r.shape[1], 512):
        pt = support[:, a0:a0 + 512].T
        a = (np.where(pt[:, :, None] & pt[:, None, :], g[None], 0) + (eye[None] & ~pt[:, :, None])).astype(solve)
        rhs = np.where(pt, r[:, a0:a0 + 512].T, 0).astype(solve)[:, :, None]
        out[:, a0:a0 + 512] = np.linalg.solve(a, rhs)[:, :, 0].T
    return np.maximum(out, 0).astype(np.float64)


def terms_of(c):
    """Split-bf16 ANLS products carry four terms (nmfx_bf16_vht / nmfx_bf16_vtw: terms = 4, the Gram by-product with them)."""
    return 4 if c.arith == "bf16" and c.k > 32 else "f32"


@functools.lru_cache(maxsize=None)
def trajectory(c):
    """The emulated two-iteration run of a case: per half-step the float64 solution of every problem (host_bpp) conditioned on
    the emulation's previous f32 iterate, the Lawson-Hanson reference on check B's problems, the emulation's own result and its
    figures.  [(label, dict)]"""
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = A.lam_of(c)
    out = []
    prev = (w0, h0)
    vt = np.ascontiguousarray(v.T)
    for s in (1, 2):
        for side in "WH":
            if side == "W":
                f, b, lam, warm = np.ascontiguousarray(prev[1].T), vt, lw, prev[0].T > 0
            else:
                f, b, lam, warm = prev[0], v, lh, prev[1] > 0
            g, r = A.gram_rhs(f, b, lam)
            full = A.host_bpp(g, r, warm)
            cols = A.b_columns(r.shape[1], c.k)
            xref = A.reference(f, b, lam, g, r, None if len(cols) == r.shape[1] else cols)
            emu = emu_half_step(f, b, lam, full > 0, terms_of(c))
            top = full.max(axis=0)
            dev = np.abs(emu - full).max(axis=0) / np.where(top > 0, top, 1.0)
            exact = emu_half_step(f, b, lam, full > 0, terms_of(c), solve=np.float64)
            kkt_worst, kkt_msg, _ = A.kkt(f"{side}{s}", g, r, exact, bar=A.KKT_BAR / 3, record=False)
            kkt32 = A.kkt(f"{side}{s}", g, r, emu, record=False)[0]
            out.append((f"{side}{s}", dict(g=g, r=r, f=f, b=b, lam=lam, full=full, cols=cols, xref=xref, emu=emu, floor=float(dev.max()),
                                           kkt=kkt_worst, kkt32=kkt32, kkt_msg=kkt_msg, zeros=A.zero_counts(full), cond=float(np.linalg.cond(
                                               g[np.ix_(np.diag(g) > 0, np.diag(g) > 0)])))))
            prev = (emu.T, prev[1]) if side == "W" else (prev[0], emu)
    return out


IDS = [A.case_id(c) for c in A.CASES]


# ---- bars -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.CASES, ids=IDS)
def test_emulation_passes_a_and_defines_b(c):
    """Check A at a third of its bar on every problem of every half-step; the emulation's largest deviation from the float64
    solution is within the floor of the table, and the bar is 10 x that floor (NMFX_WRITE_ANLS_BARS=<file>: append the figures
    instead, to rebuild the table).  Also pins host_bpp to the Lawson-Hanson reference on the problems check B covers."""
    steps = trajectory(c)
    for label, h in steps:
        assert h["kkt_msg"] is None, f"{A.case_id(c)}: {h['kkt_msg']}"
        top = h["xref"].max(axis=0)
        diff = np.abs(h["full"][:, h["cols"]] - h["xref"]).max(axis=0) / np.where(top > 0, top, 1.0)
        assert diff.max() < 1e-9, f"{A.case_id(c)} {label}: host_bpp differs from Lawson-Hanson by {diff.max():.2e} of the column maximum"
    floor = max(h["floor"] for _, h in steps)
    path = os.environ.get("NMFX_WRITE_ANLS_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": A.case_id(c), "floor": floor, "kkt": max(h["kkt"] for _, h in steps), "kkt32": max(h["kkt32"] for _, h in steps),
                                 "cond": max(h["cond"] for _, h in steps)}) + "\n")
        return
    table_floor, bar, _ = A.BARS[A.case_id(c)]
    assert bar == pytest.approx(10 * table_floor, rel=1e-12)
    assert floor <= table_floor, f"{A.case_id(c)}: emulated deviation {floor:.3e} above the table's floor {table_floor:.3e}"
    assert floor >= table_floor / 2, f"{A.case_id(c)}: emulated deviation {floor:.3e}: the table's floor {table_floor:.3e} (and its bar) is stale"


# ---- regimes: the reference alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", A.CASES, ids=IDS)
def test_regimes(c):
    """The zero counts of the float64 solutions of every half-step meet the regime's condition (tests/anls_step.py:make_case).
    mixed at 257 x 200: at least 10 % of the problems of every half-step with <= MC - 4 zeros and 10 % with > MC, for
    k = 33 .. 100.  At k = 127 and 128 the half-step without lambda has 133 (W) or 171 (H) full-weight rows for its 127 / 128
    unknowns (cond(G) 1e5): every solution there is sparse, and the half-step with lambda has nothing between 20 and 80
    zeros; there the condition is asserted over the two half-steps of an iteration together, with 5 % in (36, 56]."""
    mc = A.mc_of(c.k)
    steps = trajectory(c)
    pairs = {}
    for label, h in steps:
        z = h["zeros"]
        pairs.setdefault(label[1:], []).append(z)
        where = f"{A.case_id(c)} {label}: zeros per problem min {z.min()}, median {int(np.median(z))}, max {z.max()}"
        if c.regime in ("settled", "dead"):
            assert z.max() <= mc - 4, where
        elif c.regime == "cold" and c.k >= 64 and label[0] == "W":
            assert z.min() > A.final_workspace(c.k), where
        elif c.regime == "zero" and label[1] == "1":
            assert (z < c.k).all(), where                                  # (no problem's solution is all zero: the passive set must grow)
        elif c.regime == "mixed" and (c.m, c.n) == (257, 200) and 33 <= c.k <= 100:
            small, large = np.mean(z <= mc - 4), np.mean(z > mc)
            assert small >= 0.10 and large >= 0.10, where + f"; {small:.0%} with <= {mc - 4} zeros, {large:.0%} with > {mc}"
    for s, zs in pairs.items():
        z = np.concatenate(zs)
        where = f"{A.case_id(c)} iteration {s}: zeros per problem min {z.min()}, median {int(np.median(z))}, max {z.max()}"
        if c.regime == "mixed" and (c.m, c.n) == (257, 200) and c.k >= 127:
            small, large, second = np.mean(z <= mc - 4), np.mean(z > mc), np.mean((z > 36) & (z <= 56))
            assert small >= 0.10 and large >= 0.10 and second >= 0.05, where + f"; {small:.0%} / {large:.0%} / {second:.0%}"
            assert all(np.mean(zz > mc) >= 0.10 for zz in zs), where
        if A.expects_both_paths(c):
            assert (z <= mc - 4).any() and (z > A.final_workspace(c.k)).any(), where
            if A.kp_of(c.k) == 128:
                assert ((z > 36) & (z <= 52)).any(), where


# ---- faults the norm tests cannot see -------------------------------------------------------------------------------------------
FAULT_CASE = A.Case("mixed", 257, 200, 40, "bf16")
FAULTS = ["stale", "neighbour", "projection", "lambda", "active_up", "passive_zeroed"]


def plant(fault, h, prev, c):
    """The exact float64 solution of a half-step with `fault` in problem c."""
    g, r, lam = h["g"], h["r"], h["lam"]
    x = h["full"].copy()
    k = x.shape[0]
    if fault == "stale":
        x[:, c] = prev[:, c]
    elif fault == "neighbour":
        x[:, c] = x[:, c + 1]
    elif fault == "projection":
        x[:, c] = np.maximum(np.linalg.solve(g, r[:, c]), 0)
    elif fault == "lambda":
        x[:, c] = A.host_bpp(g - lam * np.eye(k), r[:, c:c + 1])[:, 0]
    elif fault == "active_up":
        y = g @ x[:, c] - r[:, c]
        i = int(np.argmax(np.where(x[:, c] == 0, y, -np.inf)))
        x[i, c] = 1e-3 * x[:, c].max()
    elif fault == "passive_zeroed":
        i = int(np.argmax(np.where(x[:, c] > 0, -x[:, c], -np.inf)))          # the smallest passive variable
        x[i, c] = 0
    return x


NORM_LAMS, NORM_ITERS = (0.05, 0.02), 4


def _iterate(v, w, h, first_w=None):
    """One exact ANLS iteration in float64 (host_bpp), f32 iterates; first_w: a given W (m x k) instead of the W half-step."""
    vt = np.ascontiguousarray(v.T)
    if first_w is None:
        first_w = A.host_bpp(*A.gram_rhs(np.ascontiguousarray(h.T), vt, NORM_LAMS[0]), w.T > 0).T
    w = A.f32(first_w)
    return w, A.f32(A.host_bpp(*A.gram_rhs(w, v, NORM_LAMS[1]), h > 0))


@functools.lru_cache(maxsize=None)
def norm_case():
    """The setting of the norm test of tests/test_gpu_anls.py at 257 x 200: planted_matrix, k = 40, lambda = (0.05, 0.02),
    4 iterations (here from a uniform start).  Returns the W half-step of iteration 2 and the fault-free final product."""
    from oracle import nmf_ref as R
    m, n, k = 257, 200, 40
    v = R.planted_matrix(m, n, k, seed=m + k, dtype=np.float32)
    _, w0, h0 = A.make_inputs(m, n, k, seed=1)
    w1, h1 = _iterate(v, w0, h0)
    f, b = np.ascontiguousarray(h1.T), np.ascontiguousarray(v.T)
    g, r = A.gram_rhs(f, b, NORM_LAMS[0])
    full = A.host_bpp(g, r, w1.T > 0)
    half = dict(g=g, r=r, f=f, b=b, lam=NORM_LAMS[0], full=full, cols=np.arange(m), xref=A.reference(f, b, NORM_LAMS[0], g, r),
                zeros=A.zero_counts(full), prev=w1.T)
    return v, h1, half, final_product(v, h1, full)


def final_product(v, h1, w2t):
    w, h = _iterate(v, None, h1, first_w=w2t.T)
    for _ in range(NORM_ITERS - 2):
        w, h = _iterate(v, w, h)
    return w @ h


@pytest.mark.parametrize("fault", FAULTS)
def test_fault_in_one_problem_is_rejected_and_named(fault):
    """One fault in one problem of the W half-step of iteration 2 (warm start: W_1), everything else the exact float64
    solution: check A or check B rejects it and names the problem.
    The norm test of tests/test_gpu_anls.py (||W H - W_ref H_ref|| / ||V|| < 1e-4 on the final pair of 4 iterations) is blind
    to the two faults that move one variable (asserted: 8.7e-7 and 1.9e-5).  The four that replace a whole problem it does see
    in this setting, by a small factor only -- stale 9.5e-4, neighbour 9.7e-4, projection 1.4e-3, lambda 3.4e-4 (the faulty
    half-step alone: 4.0e-3, 1.6e-2, 2.4e-2, 2.1e-4) -- because the early iterates of ANLS are sensitive: one wrong row of W_2
    moves the whole of H_2.  At the 16384 x 8192 of tests/test_gpu_fullsize.py one problem weighs 8 to 64 times less."""
    v, h1, h, good = norm_case()
    zeros = h["zeros"]
    idx = np.arange(len(zeros))
    prob = int(np.argmax((zeros >= 3) & (zeros <= 37) & (idx < len(zeros) - 1)))
    x = plant(fault, h, h["prev"], prob)
    assert not np.array_equal(x[:, prob], h["full"][:, prob])
    _, msg_a, _ = A.kkt("W2", h["g"], h["r"], x, record=False)
    _, msg_b = A.values("W2", h["g"], h["r"], x, h["xref"], h["cols"], A.bar_of(FAULT_CASE), record=False)
    assert msg_a or msg_b, f"{fault} in problem {prob} passed both checks"
    for msg in (msg_a, msg_b):
        if msg:
            assert f"problem {prob}," in msg and ("1 of " in msg), msg
    vn = np.linalg.norm(v.astype(np.float64))
    norm = np.linalg.norm(final_product(v, h1, x) - good) / vn
    print(f"{fault}: final pair {norm:.2e}; the faulty half-step alone {np.linalg.norm(h['f'] @ (x - h['full'])) / vn:.2e}")
    if fault in ("active_up", "passive_zeroed"):
        assert norm < 1e-4, f"{fault}: the norm test would see it ({norm:.2e})"


def test_exact_solution_passes_both_checks():
    c = FAULT_CASE
    h = dict(trajectory(c))["H2"]
    assert A.kkt("H2", h["g"], h["r"], h["full"], bar=1e-12, record=False)[1] is None
    assert A.values("H2", h["g"], h["r"], h["full"], h["xref"], h["cols"], 1e-9, record=False)[1] is None


def test_non_finite_and_negative_values_never_pass():
    h = dict(trajectory(FAULT_CASE))["H2"]
    for bad in (np.nan, np.inf, -1e-30):
        x = h["full"].copy()
        x[2, 5] = bad
        worst, msg, _ = A.kkt("H2", h["g"], h["r"], x, record=False)
        assert worst == np.inf and "problem 5, variable 2" in msg


# ---- references -----------------------------------------------------------------------------------------------------------------
def test_cholesky_reference_equals_the_stacked_reference():
    """nnls on the Cholesky factor of the float64 G (from k = 65 on) = the oracle's stacked form, to 1e-9 of the column maximum."""
    v, w0, h0 = A.make_case("mixed", 130, 64, 100)
    lam = 0.02
    g, r = A.gram_rhs(w0, v, lam)
    cols = np.arange(0, 64, 2)
    a, b = A.ref_chol(g, r, cols), A.ref_stacked(w0, v, lam, cols)
    assert np.abs(a - b).max(axis=0).max() <= 1e-9 * b.max()
    assert (A.zero_counts(a) == A.zero_counts(b)).all() and A.zero_counts(b).max() > 0


def test_b_columns_cover_the_wraps():
    cols = A.b_columns(3100, 33)
    assert {0, 7, 3092, 3099, 3064, 3071, 3072, 3079} <= set(cols.tolist()) and len(cols) >= 128 + 16
    assert len(A.b_columns(257, 17)) == 257
    cols = A.b_columns(1100, 130)
    assert {1016, 1023, 1024, 1031} <= set(cols.tolist())
    assert {504, 511, 512, 519} <= set(A.b_columns(600, 128).tolist())
