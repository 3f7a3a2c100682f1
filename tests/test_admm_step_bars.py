"""The bars and the inputs of the element-wise ADMM / AO-ADMM step checks (tests/admm_step.py), proven on the CPU.

A numpy emulation of the device arithmetic (f32 state, f32-accumulated or split-bf16 products as the path runs them, the float64
inverse rounded to f32, the f32 product with it) is compared with the float64 step per case: 10 x its largest deviation is the
case's value bar, and likewise the residual bar.  Asserted here: the emulation passes every check at those bars, the exact
float64 step passes at the floor, non-finite and negative values never pass, every case's inputs keep the two branch conditions
clear (the inner stop's ratios 1e-3 away from its tolerance at every round of the float64 reference, the row sums of the l1inf
operators 1e-3 away from their bound), and the designated cases reach every outcome of the speculative rounds.  Then nine faults are
planted: the eight of the case table in the exact float64 step 2 of one case each, and the folded pivot update of a Gauss-Jordan
elimination (pivot_case).  Of the eight each must be rejected by the stated check at the planted place, and the
test prints what the trajectory bar of tests/test_gpu_admm.py / test_gpu_aoadmm.py (||W H - W_ref H_ref|| / ||V|| < 1e-4 after the
run) would have seen.  Not reproduced by the emulation: the MFMA summation order and the order of the slab sums; the factor 10 is
for those."""
import re

import numpy as np
import pytest

import admm_step as A
from oracle import nmf_ref as R

IDS = [A.case_id(c) for c in A.CASES]
ALL = A.CASES + [c for _, c in A.KNOB_CASES if c not in A.CASES]
USEFUL = 5e-2               # a value bar above this checks nothing: the inputs of such a case are wrong for it


def bars(c):
    return A.bars_ao_kl(c) if (c.family, c.loss) == ("ao", "kl") else A.bars_of(c)


# ---- the emulation passes; the inputs meet their conditions -------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=[A.case_id(c) for c in ALL])
def test_emulation_passes_and_inputs_are_clear(c):
    b = bars(c)
    assert not b["emu_fails"], "\n".join(b["emu_fails"])                      # (inner counts of the emulation = the reference's among them)
    assert b["values"] <= USEFUL, f"{A.case_id(c)}: value bar {b['values']:.2e}"
    assert b["stop_margin"] >= A.STOP_CLEAR, f"{A.case_id(c)}: a ratio of the inner stop comes within {b['stop_margin']:.2e} of its tolerance"
    if (c.family, c.loss) == ("ao", "kl"):
        first, second = A.emulate_ao_kl(c)
        fails = []
        A.check_ao_kl(c, first, second, b["values"], fails, "", record=False)
    else:
        assert b["l1inf_margin"] >= A.L1INF_CLEAR, f"{A.case_id(c)}: a row sum of an l1inf operator comes within {b['l1inf_margin']:.2e} of its bound"
        assert b["residual"] <= USEFUL and b["emu_tie"] <= A.TIE_ULPS / 2
        fails, _, _ = A.measure(c, A.emulate(c), bars=b)
    assert not fails, "\n".join(fails)
    print(f"{A.case_id(c)}: emulated deviation {b['emu'][0]:.2e}, value bar {b['values']:.2e}, residual bar {b.get('residual', 0):.2e}")


# ---- float64 steps: exact, and with a planted fault -----------------------------------------------------------------------------------
def half64(f, d, x, dual, rho, prox, lam, fault=None):
    """One exact ADMM half-step (columns = problems) with an optional fault."""
    b = f.T @ d
    if fault == "tile":                                 # one 128 x 64 tile of D missing from F^T D: rows 0..127, problems 64..127
        b[:, 64:128] -= f[0:128].T @ d[0:128, 64:128]
    rhs = b + rho * (x + (0 if fault == "no_dual" else dual))
    aux = np.linalg.solve(f.T @ f + rho * np.eye(f.shape[1]), rhs)
    xn = R.prox(prox, aux, dual, rho=rho, lam=lam)
    return aux, xn, dual + xn - aux


def admm64(c, v, st, kl=None, fault=None):
    """One exact ADMM step from State st (kl: A.KL, advanced in place).  Faults: 'stale_dual' (dual_w of rows 64..127 from the w_aux
    before), 'no_dual' (the H right-hand side without the dual), 'old_h_aux' (the W half solved with the h_aux before), 'tile',
    'dual_v' (KL: handled by the caller, who does not advance kl)."""
    d = np.asarray(v, np.float64) if kl is None else kl.data()
    ha, h, dh = half64(st.w_aux, d, st.h, st.dual_h, c.rho, c.prox_h, c.lam_h, fault if fault in ("no_dual", "tile") else None)
    f = (st.h_aux if fault == "old_h_aux" else ha).T.copy()
    wa, w, dw = (a.T.copy() for a in half64(f, d.T.copy(), st.w.T, st.dual_w.T, c.rho, c.prox_w, c.lam_w))
    if fault == "stale_dual":
        dw[64:128] = (st.dual_w + w - st.w_aux)[64:128]
    if kl is not None:
        kl.advance(wa, ha)
    return A.State(w, h, wa, ha, dw, dh, (0, 0))


def block64(f, d, x, dual, k, prox, lam, admm_iter, fault=None):
    """aoadmm_ls_block with an optional fault: 'rho_kp' (rho = trace / padded k), 'lam_block' (lambda / rho dropped for problems
    32..63), 'late_stop' (the stop decided one round late)."""
    if fault == "late_stop":
        return A.ref_block(f, d, x, dual, k, prox, lam, admm_iter, stop_offset=1)
    g = f.T @ f
    rho = np.trace(g) / (A.kp_of(k) if fault == "rho_kp" else k)
    minv = np.linalg.inv(g + rho * np.eye(k))
    b = f.T @ d
    ran, fired, aux = 0, False, None
    for j in range(admm_iter):
        aux = minv @ (b + rho * (x + dual))
        prev = x
        x = R.prox(prox, aux, dual, rho=rho, lam=lam)
        if fault == "lam_block":
            x[:, 32:64] = R.prox("nn", aux, dual)[:, 32:64]
        dual = dual + x - aux
        ran = j + 1
        if R.inner_stop(x, prev, aux, dual):
            fired = True
            break
    return A.Block(x, dual, ran, fired, aux, rho, [])


def ao64(c, v, st, fault=None, side="H"):
    vv = np.asarray(v, np.float64)
    bh = block64(st.w, vv, st.h, st.dual_h, c.k, c.prox_h, c.lam_h, c.admm_iter, fault if side == "H" else None)
    bw = block64(bh.x.T.copy(), vv.T.copy(), st.w.T, st.dual_w.T, c.k, c.prox_w, c.lam_w, c.admm_iter, fault if side == "W" else None)
    return A.State(bw.x.T.copy(), bh.x, None, None, bw.dual.T.copy(), bh.dual, (bh.ran | (int(bh.fired) << 16), bw.ran | (int(bw.fired) << 16)))


def run64(c, fault=None, side="H", total=2):
    """[State_1 .. State_total] of the exact float64 run of case c with `fault` planted in step 2 only."""
    v, w0, h0 = A.make_case(c)
    st, out = A.start_state(c, w0, h0), []
    kl = A.KL(v) if c.loss == "kl" else None
    for s in range(1, total + 1):
        f = fault if s == 2 else None
        if c.family == "admm":
            if f == "dual_v":                           # the m x n dual is not advanced behind step 1: step 2 reads the old one
                kl.dual_v = np.zeros_like(kl.dual_v)
                f = None
            st = admm64(c, v, st, kl, f)
        else:
            st = ao64(c, v, st, f, side)
        out.append(st)
    return out


def find(pred):
    return next(c for c in A.CASES if pred(c))


ADMM_CASE = find(lambda c: (c.family, c.loss, c.k, c.arith, c.prox_h) == ("admm", "eu", 33, "bf16", "l1n") and c.edges)
ADMM_KL_CASE = find(lambda c: (c.family, c.loss, c.k, c.arith) == ("admm", "kl", 40, "bf16"))
AO_CASE = find(lambda c: (c.family, c.loss, c.k, c.arith, c.admm_iter, c.prox_h) == ("ao", "eu", 40, "bf16", 5, "l1n") and c.m == 257)
AO_STOP_CASE = find(lambda c: (c.family, c.loss, c.k, c.arith, c.admm_iter) == ("ao", "eu", 65, "bf16", 5))
TRAJECTORY_ITERS = {"admm": 10, "ao": 4}               # (tests/test_gpu_admm.py runs 6 to 12 iterations, tests/test_gpu_aoadmm.py 4 to 12)

# fault: (case, side of the fault, the check that must name it, the problems (rows of W / columns of H) it may name)
FAULTS = {
    "stale_dual": (ADMM_CASE, "W", "[dual tie]", (64, 128)),
    "rho_kp": (AO_CASE, "H", "[values", None),
    "lam_block": (AO_CASE, "H", "[values, x]", (32, 64)),
    "no_dual": (ADMM_CASE, "H", "[residual]", None),
    "old_h_aux": (ADMM_CASE, "W", "[residual]", None),
    "late_stop": (AO_STOP_CASE, "W", "[inner count]", None),
    "tile": (ADMM_CASE, "H", "[residual]", (64, 128)),
    "dual_v": (ADMM_KL_CASE, "H", "[residual]", None),
}


@pytest.mark.parametrize("c", [ADMM_CASE, ADMM_KL_CASE, AO_CASE, AO_STOP_CASE, A.PATH_CASES[0]], ids=A.case_id)
def test_exact_float64_steps_pass_at_the_floor(c):
    floor = dict(values=1e-9, residual=1e-9)
    fails, maxima, _ = A.measure(c, run64(c), bars=floor)
    assert not fails, "\n".join(fails)
    assert A._largest(maxima, ("tie",)) <= 1e-3        # (float64 duals: no f32 rounding at all)


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_is_rejected_and_named(fault):
    c, side, check, where = FAULTS[fault]
    good, bad = run64(c), run64(c, fault, side)
    fails, _, _ = A.measure(c, bad, bars=A.bars_of(c))
    hits = [f for f in fails if f"step 2 {side} {check}" in f]
    if where and hits:
        named = int(re.search(r"(?:row|column) (\d+)", hits[0]).group(1))
        assert where[0] <= named < where[1], f"{fault}: {check} names problem {named}, planted in {where}: {hits[0]}"
    assert hits, f"{fault}: not rejected by {check} of step 2 {side}:\n" + "\n".join(fails)
    assert not [f for f in fails if "step 1" in f]
    v = np.asarray(A.make_case(c)[0], np.float64)
    n = TRAJECTORY_ITERS[c.family]
    g, b = run64(c, total=n)[-1], run64(c, fault, side, total=n)[-1]
    seen = np.linalg.norm(b.w @ b.h - g.w @ g.h) / np.linalg.norm(v)
    now = np.linalg.norm(bad[1].w @ bad[1].h - good[1].w @ good[1].h) / np.linalg.norm(v)
    print(f"{fault} ({A.case_id(c)}): rejected by {check} of step 2 {side}: {hits[0][:160]} ...; the trajectory bar (1e-4) would have seen "
          f"{seen:.2e} after {n} iterations ({now:.2e} right behind the faulty step)")


def test_non_finite_and_negative_values_never_pass():
    for c in (ADMM_CASE, AO_CASE):
        for bad in (np.nan, np.inf, -1e-30):
            states = run64(c)
            states[1].h[2, 5] = bad
            fails, _, _ = A.measure(c, states, bars=A.bars_of(c))
            assert any("step 2 H [structure]: column 5, component 2" in f for f in fails), (c, bad, fails)
            if not np.isfinite(bad):
                assert any("step 2 H [values, x]: column 5" in f for f in fails), (c, bad, fails)


# ---- references and rules ------------------------------------------------------------------------------------------------------------
def test_reference_blocks_are_the_oracles():
    c = AO_STOP_CASE
    v, w0, h0 = A.make_case(c)
    vv = np.asarray(v, np.float64)
    dual = 0.01 * h0
    b = A.ref_block(w0, vv, h0, dual, c.k, "l1n", 0.05, 5)
    x, d, ran = R.aoadmm_ls_block(vv, w0, h0, dual, c.k, "l1n", admm_iter=5, lam=0.05)
    assert np.array_equal(b.x, x) and np.array_equal(b.dual, d) and b.ran == ran
    z = np.zeros_like(vv)
    kb = A.ref_kl_block(vv, z, z, w0, h0, dual, c.k, "l1n", 0.05, 3)
    x, d, va, dv, ran = R.aoadmm_kl_block(vv, z, z, w0, h0, dual, c.k, "l1n", admm_iter=3, lam=0.05)
    assert np.array_equal(kb.x, x) and np.array_equal(kb.dual, d) and np.array_equal(kb.v_aux, va) and np.array_equal(kb.dual_v, dv) and kb.ran == ran
    a1, x1, d1 = A.ref_half(w0, vv, h0, dual, 2.0, "l1n", 0.05)
    assert np.array_equal(a1, R.admm_aux_step(h0, dual, w0, vv, None, 2.0, "eu"))


def test_split_products_are_those_of_the_mur_emulation():
    from test_mur_step_bars import prod
    rng = np.random.default_rng(3)
    a, b = rng.uniform(0.1, 1, (40, 257)).astype(np.float32), rng.uniform(0.05, 1, (257, 70)).astype(np.float32)
    for terms in (3, 4, "f32"):
        assert np.array_equal(A.prod(a, b, terms), prod(a, b, terms=terms))


def test_expected_paths_rule():
    """fused_plan (kernels_aoadmm.hip): by hand for admm_iter = 10."""
    assert A.expected_paths([(10, False), (10, False)], 10) == (2, 0, 0, 0)
    assert A.expected_paths([(3, True), (3, True)], 10) == (1, 1, 0, 0)          # cut back from 10 to 3; then the hint 3 stands
    assert A.expected_paths([(3, True), (2, True)], 10) == (0, 2, 0, 0)
    assert A.expected_paths([(8, True), (9, True)], 10) == (0, 1, 0, 1)          # no stop within 8: continued, and cut back to 9
    assert A.expected_paths([(9, True), (10, False)], 10) == (0, 1, 1, 0)
    assert A.expected_paths([(9, True), (10, True)], 10) == (0, 1, 1, 0)
    assert A.expected_paths([(8, True), (9, True)], 10, hinted=False) == (0, 2, 0, 0)
    assert A.expected_paths([(10, True), (4, True)], 10) == (1, 1, 0, 0)         # a stop at the last round: the hint is 10, the full leg


def test_the_case_table_reaches_every_outcome_of_the_speculative_rounds():
    total = np.zeros(4, dtype=int)
    for c in A.CASES:
        if (c.family, c.loss) != ("ao", "eu") or not A.paths_of(c)["fused"] or max(c.m, c.n) > 5000:
            continue
        counts = A.bars_of(c)["counts"]
        for side in "HW":
            total += np.array(A.expected_paths([counts[s][side] for s in (1, 2)], c.admm_iter))
    assert (total > 0).all(), total
    want = {A.PATH_CASES[0]: (2, 1, 0, 1), A.PATH_CASES[1]: (2, 1, 1, 0)}
    for c, paths in want.items():
        counts = A.bars_of(c)["counts"]
        got = tuple(sum(x) for x in zip(*(A.expected_paths([counts[s][side] for s in (1, 2)], c.admm_iter) for side in "HW")))
        assert got == paths, (A.case_id(c), counts, got)
    print("outcomes over the table (stood, cut back, continued, continued and cut back):", tuple(int(t) for t in total))


def test_case_table_covers_the_kernel_variants():
    ao = [c for c in A.CASES if (c.family, c.loss) == ("ao", "eu")]
    assert any(A.paths_of(c)["cols64"] for c in ao) and any(A.paths_of(c)["rows128"] and c.arith == "bf16" for c in ao)
    assert sum(A.paths_of(c)["wraps"] and not A.paths_of(c)["cols64"] and not A.paths_of(c)["rows128"] for c in ao) >= 2
    assert any(c.k > 512 for c in ao) and {1, 5, 10} <= {c.admm_iter for c in ao}
    assert {A.kp_of(c.k) for c in ao} >= {16, 32, 64, 128, 256, 640}
    admm = [c for c in A.CASES if c.family == "admm"]
    assert {"nn", "l1n", "l2n", "l1inf", "l1inf_transpose"} <= {c.prox_w for c in admm} & {c.prox_h for c in admm}
    assert {0.0, 1.0, 2.0} <= {c.rho for c in admm} and {c.k for c in admm if c.rho == 0} == {12, 16, 40, 160}
    assert len(set(IDS)) == len(IDS)


def test_float64_reference_of_the_exact_f32_kl_refusals():
    """The exact-f32 AO-ADMM-KL sections of tools/entry_digest.py at k = 100 and 160 are refused as not positive definite.  The float64
    reference on the same inputs: the first outer iteration wipes W out (every column zero), and the Cholesky factorisation of the H
    sub-problem of outer iteration 1 raises; at k = 40 four iterations run.  (tests/test_gpu_admm_step.py holds the device to it.)"""
    for k, want in ((40, None), (100, 1), (160, 1)):
        assert A.kl_refusal_reference(k) == want


@pytest.mark.parametrize("k", A.PIVOT_RANKS)
def test_folded_pivot_update_is_rejected_at_large_pivots(k):
    """pivot_case: with the clean Gauss-Jordan inverse (rounded to f32, f32 product) the half-step passes; with row and column p folded
    into the rank-1 update the checks reject it.  This shows that an error of piv^2 eps is caught at these inputs, in a float64
    numpy elimination; that the device kernels produced it is the GPU observation recorded in DESIGN.md 2."""
    v, w0, h0, rho = A.pivot_case(k)
    f = np.float32
    g = (w0.astype(f).T @ w0.astype(f)).astype(np.float64) + rho * np.eye(k)
    rhs = (w0.astype(f).T @ v + f(rho) * h0.astype(f)).astype(f)
    seen = {}
    for folded in (False, True):
        aux = (A.gauss_jordan(g, folded).astype(f) @ rhs).astype(np.float64)
        x = np.maximum(aux, 0)
        fails, bars = A.check_pivot_half(k, aux, x, x - aux, record=False)
        seen[folded] = fails
    assert not seen[False], "\n".join(seen[False])
    assert any("[residual]" in m for m in seen[True]), seen[True]
    print(f"k = {k}: folded pivot update rejected: {seen[True][0][:150]}")
