"""The bars of the stacked HALS checks (tests/hals_stack_step.py), proven on the CPU.

The float32 emulation of a stacked half-step -- products as the device forms them on the STACKED factors, the Gram matrix masked
and 2 lambda_p put on its diagonal in float32, the sweep in the kernel's kept-residual form over all components -- equals the
emulation run problem by problem BIT FOR BIT (a masked term is res - 0 d); its deviation from the float64 masked sweep defines
each case's bar, as in tests/test_hals_step_bars.py.  The emulation of the objective decomposition defines the objective's bar.
Planted faults the comparator must reject: the Gram matrix left unmasked, problem 0's lambda applied to all problems, a stopped
problem swept anyway."""
import functools
import json
import os

import numpy as np
import pytest

import anls_step as A
import hals_step as HS
import hals_stack_step as ST
from mur_step import OBJ_FLOOR, OBJ_RTOL
from test_hals_step_bars import sweep_kept_residual
from test_mur_step_bars import prod

F = np.float32
IDS = [c.name for c in ST.CASES]


def terms_of(c):
    return 4 if ST.arith_of(c) == "bf16" else "f32"


def emu_products(f, b, terms):
    ft = np.ascontiguousarray(np.asarray(f, F).T)
    return prod(ft, np.asarray(f, F), terms=terms).astype(F), prod(ft, np.asarray(b, F), terms=terms).astype(F)


def emu_half_step(c, side, f, b, prev, fault=None, stopped=()):
    """The stacked half-step in float32, the kernel's form.  fault: 'unmasked' | 'lambda0'; stopped: problems left as they are."""
    g, r = emu_products(f, b, terms_of(c))
    lams = [l[side] for l in c.lams]
    if fault == "lambda0":
        lams = [lams[0]] * len(lams)
    if fault == "unmasked":
        lam = np.array([lams[p] if p != ST.NONE else 0.0 for p in ST.comp2prob(c.ks, g.shape[0])])
        gm = (g + np.diag((2 * lam).astype(F))).astype(F)
    else:
        gm = ST.mask_gram(g, c.ks, lams).astype(F)
    c2p = ST.comp2prob(c.ks, g.shape[0])
    frozen = np.isin(c2p, list(stopped)) | (c2p == ST.NONE)
    gs = gm.copy()
    gs[frozen, frozen] = 0                               # not live: the kernel makes a step of zero there
    out = sweep_kept_residual(gs, r, prev, c.sweeps).astype(np.float64)
    return out


def emu_per_problem(c, side, f, b, prev):
    """The same half-step, every problem on its own: its own products' block, its own lambda, its own sweep."""
    g, r = emu_products(f, b, terms_of(c))
    off = ST.offsets(c.ks)
    out = np.array(prev, dtype=np.float64)
    for p in range(len(c.ks)):
        sl = slice(off[p], off[p + 1])
        gp = (g[sl, sl] + F(2 * c.lams[p][side]) * np.eye(c.ks[p], dtype=F)).astype(F)
        out[sl] = sweep_kept_residual(gp, r[sl], np.asarray(prev)[sl], c.sweeps)
    return out


def emu_objective(c, v, w, h):
    """[obj_p] by the device's decomposition: A = V H^T in the device's product arithmetic, the rest float64."""
    v64 = np.asarray(v, np.float64)
    a = prod(np.asarray(v, F), np.ascontiguousarray(np.asarray(h, F).T), terms=terms_of(c)).astype(np.float64)
    half_vv = 0.5 * float(np.sum(v64 * v64))
    off = ST.offsets(c.ks)
    out = []
    for p in range(len(c.ks)):
        sl = slice(off[p], off[p + 1])
        out.append(half_vv - float(np.sum(w[:, sl] * a[:, sl])) + 0.5 * float(np.sum((w[:, sl].T @ w[:, sl]) * (h[sl] @ h[sl].T))))
    return out


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """The emulated two-iteration run of a case: [(label, dict)] per half-step, and the objective deviations."""
    c = ST.BY_NAME[name]
    v, starts = ST.make_case(c)
    w, h = ST.stack(starts, c.k_handle)
    vt = np.ascontiguousarray(v.T)
    scale = OBJ_FLOOR * 0.5 * float(np.sum(v.astype(np.float64) ** 2))
    out, obj_dev = [], 0.0

    def objective_deviation():
        want = ST.objective_parts(v, w, h, c.ks)
        return max(abs(g - t) / max(abs(t), scale) for g, t in zip(emu_objective(c, v, w, h), want))

    for s in (1, 2):
        obj_dev = max(obj_dev, objective_deviation())
        for label in (f"W{s}", f"H{s}"):
            side = 0 if label[0] == "W" else 1
            f, b, prev = (np.ascontiguousarray(h.T), vt, np.ascontiguousarray(w.T)) if side == 0 else (w, v, h)
            g, r = A.gram_rhs(f, b, 0.0)
            gm = ST.mask_gram(g, c.ks, [l[side] for l in c.lams])
            xref, numer = HS.sweep(gm, r, prev, c.sweeps)
            emu = emu_half_step(c, side, f, b, prev)
            out.append((label, dict(side=side, f=f, b=b, r=r, prev=prev, xref=xref, numer=numer, emu=emu)))
            if side == 0:
                w = np.ascontiguousarray(emu.T)
            else:
                h = emu
    obj_dev = max(obj_dev, objective_deviation())
    return out, obj_dev


def floor_of(c):
    off = ST.offsets(c.ks)
    worst = 0.0
    for label, hh in trajectory(c.name)[0]:
        for p in range(len(c.ks)):
            sl = slice(off[p], off[p + 1])
            worst = max(worst, HS.values(label, hh["r"][sl], hh["emu"][sl], hh["xref"][sl], np.zeros_like(hh["numer"][sl]), np.inf, record=False)[0])
    return worst


@pytest.mark.parametrize("c", ST.CASES, ids=IDS)
def test_emulation_defines_the_bars(c):
    """Half-step and objective floors of the table hold the emulation's deviations, the bars are 10 x the floors
    (NMFX_WRITE_HALS_STACK_BARS=<file>: append the figures instead, to rebuild the table)."""
    floor, obj_floor = floor_of(c), trajectory(c.name)[1]
    path = os.environ.get("NMFX_WRITE_HALS_STACK_BARS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps({"id": c.name, "floor": floor, "obj_floor": obj_floor}) + "\n")
        return
    tf, bar, tof, obar = ST.BARS[c.name][:4]
    assert bar == pytest.approx(10 * tf, rel=1e-12) and obar == pytest.approx(10 * tof, rel=1e-12)
    assert tf / 2 <= floor <= tf, f"{c.name}: emulated half-step deviation {floor:.3e}, table floor {tf:.3e}"
    assert tof / 2 <= obj_floor <= tof, f"{c.name}: emulated objective deviation {obj_floor:.3e}, table floor {tof:.3e}"


def test_objective_bars_above_obj_rtol_are_the_documented_ones():
    """DESIGN.md 4.11 explains every case whose objective bar is wider than the residual objective's OBJ_RTOL."""
    wide = sorted(c.name for c in ST.CASES if ST.obj_bar_of(c) > OBJ_RTOL)
    assert wide == sorted(ST.OBJ_BAR_ABOVE_RTOL), wide


@pytest.mark.parametrize("c", ST.CASES, ids=IDS)
def test_stacked_emulation_equals_per_problem_bit_for_bit(c):
    for label, hh in trajectory(c.name)[0]:
        each = emu_per_problem(c, hh["side"], hh["f"], hh["b"], hh["prev"])
        diff = int(np.sum(hh["emu"] != each))
        assert diff == 0, f"{c.name} {label}: {diff} elements differ between the stacked sweep and the per-problem sweeps"


# ---- planted faults -----------------------------------------------------------------------------------------------------------
FAULT_CASE = ST.BY_NAME["lambdas"]


def _rejected(c, label, x, stopped=()):
    """Problems the comparator rejects when the half-step's device result is x (float64 reference: stopped problems keep prev)."""
    hh = dict(trajectory(c.name)[0])[label]
    off = ST.offsets(c.ks)
    bad = []
    for p in range(len(c.ks)):
        sl = slice(off[p], off[p + 1])
        ref = np.asarray(hh["prev"])[sl] if p in stopped else hh["xref"][sl]
        numer = np.zeros_like(hh["numer"][sl]) if p in stopped else hh["numer"][sl]
        _, msg, _ = HS.values(f"{label} problem {p}", hh["r"][sl], x[sl], ref, numer, ST.bar_of(c), record=False)
        if msg:
            assert f"problem {p}" in msg
            bad.append(p)
    return bad


@pytest.mark.parametrize("label", ["W2", "H2"])
def test_faults_are_rejected(label):
    c = FAULT_CASE
    hh = dict(trajectory(c.name)[0])[label]
    assert _rejected(c, label, hh["emu"]) == []                                        # the emulation itself passes
    unmasked = emu_half_step(c, hh["side"], hh["f"], hh["b"], hh["prev"], fault="unmasked")
    assert len(_rejected(c, label, unmasked)) >= len(c.ks) - 1, "the Gram matrix left unmasked"
    lam0 = emu_half_step(c, hh["side"], hh["f"], hh["b"], hh["prev"], fault="lambda0")
    want = [p for p in range(len(c.ks)) if c.lams[p][hh["side"]] != c.lams[0][hh["side"]]]
    assert want and _rejected(c, label, lam0) == want, "problem 0's lambda applied to all problems"
    assert _rejected(c, label, hh["emu"], stopped=(1,)) == [1], "a stopped problem swept anyway"
    frozen = emu_half_step(c, hh["side"], hh["f"], hh["b"], hh["prev"], stopped=(1,))
    assert _rejected(c, label, frozen, stopped=(1,)) == []
    off = ST.offsets(c.ks)
    assert np.array_equal(frozen[off[1]:off[2]], np.asarray(hh["prev"])[off[1]:off[2]])


def test_cases_cover_what_the_kernel_branches_on():
    by = ST.BY_NAME
    assert [sum(by[n].ks) for n in ("kp16", "kp32", "kp64", "kp128")] == [16, 32, 64, 128]
    off = ST.offsets(by["lane64"].ks)
    assert off[1] < 64 < off[2]
    assert sum(by["tail"].ks) < by["tail"].k_handle == 16
    assert max(by["tall"].m, by["wide"].n) > HS.wrap_stride()
    lams = by["lambdas"].lams
    assert len(set(lams)) == len(lams) and any(a == 0.0 and b == 0.5 for a, b in zip([l[0] for l in lams], [l[0] for l in lams][1:]))
    assert any(ST.PLANTED_K in c.ks for c in ST.CASES)
    p, j = by["dead"].dead
    hh = dict(trajectory("dead")[0])["W1"]
    o = ST.offsets(by["dead"].ks)[p] + j
    assert not hh["xref"][o].any() and not np.asarray(hh["prev"])[o].any()
