"""Every ADMM half-step and AO-ADMM sub-problem of the device, element by element, against float64 (tests/admm_step.py).

The trajectory tests compare norms after 4 to 12 iterations; a fault in one 64-row block of a round kernel, one slab of a Gram
by-product or a dual updated from a stale auxiliary stays under them.  Here steps 1 and 2 run on one handle in two calls, the state
(W, H, w_aux, h_aux, dual_w, dual_h) is read in between, and every half-step is checked against the float64 step fed the device's own
previous state: structure (signs, exact zeros, the dual tied to x and aux of the same launch), the residual of the shifted Gram system,
the values, the inner counts and break bits, the recorded objectives, and -- for the fused speculative rounds -- the four outcome
counters of nmfx_get_inner_paths against the rule of fused_plan applied to the reference's counts.  The same two steps in one call
meet the same bars.  The bars come from the CPU emulation (tests/test_admm_step_bars.py), per case.

    ADMM, Euclidean        every padding of k, nn / l1n / l2n / l1inf / l1inf_transpose on either side, rho 0, 1, 2, f32 and split bf16
    ADMM, KL               kp 16 / 64 / 128, the split-bf16 iteration and the exact-f32 one; step 2 with v_aux, dual_v replayed in float64
    AO-ADMM, Euclidean     admm_iter 1 (one launch per round), 5, 10 (fused speculative rounds), the 64-column and 128-row fused kernels,
                           norm sums that wrap, beyond 128 and beyond 512 padded components
    AO-ADMM, KL            outer step 1 completely, the H sub-problem of step 2 with the auxiliaries replayed in float64
    phase protocol         step 2 through the row-sharded phase entry points with a world of one
    knobs                  read once per process: child processes, one at a time"""
import json
import os
import subprocess
import sys

import pytest

import admm_step as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases(pred):
    sel = [c for c in A.CASES if pred(c)]
    assert sel
    return pytest.mark.parametrize("c", sel, ids=[A.case_id(c) for c in sel])


def device_cus():
    """CUs of the device the engine sizes its grids by (the cases of the wide fused kernels are built for 256)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def big(c):
    return max(c.m, c.n) > 4000 or c.k > 128


# ---- ADMM ---------------------------------------------------------------------------------------------------------------------------
@cases(lambda c: (c.family, c.loss) == ("admm", "eu") and c.rho > 0 and c.k <= 128)
def test_admm_eu(c):
    A.run_case(c)


@cases(lambda c: (c.family, c.loss) == ("admm", "eu") and c.rho > 0 and c.k > 128)
def test_admm_eu_beyond_128(c):
    A.run_case(c)


@cases(lambda c: c.family == "admm" and c.rho == 0)
def test_admm_rho_zero(c):
    """rho = 0 with 'nn' on both sides is the reference's plain np.linalg.solve of the Gram system (admm.py:230): the padded
    variables of k = 12, 40, 160 must not make the prepare kernels report "not positive definite"."""
    A.run_case(c)


@pytest.mark.parametrize("k", A.PIVOT_RANKS)
def test_prepare_kernels_with_pivots_of_1e7(k):
    """One ADMM step (H half: a system with diagonal entries of 1e7 and condition number k + 1; W half: pivots of rho = 1e7): a pivot
    entry formed as piv - (piv - 1)(1 + 1/piv) is wrong by piv^2 eps = 1e-2 there.  k = 160: the same 16 x 16 pivots inside the
    128 x 128 diagonal blocks of the blocked inversion beyond 128 components."""
    A.run_pivot_case(k)


@cases(lambda c: (c.family, c.loss) == ("admm", "kl"))
def test_admm_kl(c):
    A.run_case(c)


# ---- AO-ADMM ------------------------------------------------------------------------------------------------------------------------
@cases(lambda c: (c.family, c.loss) == ("ao", "eu") and not big(c) and not c.warm)
def test_aoadmm_eu(c):
    """The cases with the 2^12 row (edges) leave H H^T with entries of 1e6: at kp = 64 / 128 they found the pivot entry of the
    Gauss-Jordan kernels formed as piv - (piv - 1)(1 + 1/piv), an error of piv^2 eps."""
    A.run_case(c)


@cases(lambda c: (c.family, c.loss) == ("ao", "eu") and max(c.m, c.n) > 4000)
def test_aoadmm_eu_wraps_and_wide_blocks(c):
    """More than 64 norm blocks (the lane-strided sums that decide the inner stop wrap), the 64-column fused H-side kernel
    (64 x 16400) and the 128-row fused W-side kernel (32700 x 72, k = 40, split bf16) -- thresholds for 256 CUs (admm_step.paths_of)."""
    p = A.paths_of(c, ncu=device_cus())
    assert p["wraps"] and p["fused"]
    assert p["cols64"] == (c.n == 16400) and p["rows128"] == (c.m == 32700), f"{A.case_id(c)} on {device_cus()} CUs: {p}"
    A.run_case(c)


@cases(lambda c: (c.family, c.loss) == ("ao", "eu") and c.k > 128)
def test_aoadmm_eu_beyond_128(c):
    A.run_case(c)


@pytest.mark.parametrize("c,want", [(A.PATH_CASES[0], (2, 1, 0, 1)), (A.PATH_CASES[1], (2, 1, 1, 0))], ids=["continued-and-cut-back", "continued"])
def test_aoadmm_speculation_outcomes(c, want):
    """The designated cases of the two outcomes a cold start does not reach (the H side stands twice; W: cut back, then continued)."""
    dev, _, _ = A.run_case(c)
    assert tuple(dev.paths) == want and tuple(dev.single_paths) == want


@cases(lambda c: (c.family, c.loss) == ("ao", "kl"))
def test_aoadmm_kl(c):
    A.run_case(c)


@pytest.mark.parametrize("k", [40, 100, 160])
def test_exact_f32_aoadmm_kl_refuses_where_the_reference_raises(k):
    """On the inputs of tools/entry_digest.py the float64 reference's first outer iteration wipes W out at k = 100 and 160 and the
    Cholesky factorisation of outer iteration 1 raises; the exact-f32 device run must refuse at the same outer iteration."""
    assert A.kl_refusal_device(k, "f32") == A.kl_refusal_reference(k)


# ---- the row-sharded phase protocol with a world of one ---------------------------------------------------------------------------------
def _phase_pick(c):
    if (c.edges and c.family == "ao" and c.admm_iter != 5) or c.warm or (c.family == "admm" and c.rho == 0) or "l1inf" in c.prox_w + c.prox_h or (c.m, c.n) not in ((257, 200), (384, 320)):
        return False
    if c.family == "admm":
        return (c.loss == "eu" and c.k in (40, 128, 160) and c.arith == "bf16") or (c.loss == "kl" and c.k in (40, 100) and c.arith == "f32")
    if c.loss == "eu":
        return c.k in (40, 128, 160) and c.arith == "bf16" and c.admm_iter == 5
    return c.k in (40, 100, 160) and c.arith == "f32"         # (k = 160: nmfx_generic_aoadmm_kl_phase)


@cases(_phase_pick)
def test_phase_protocol(c):
    """admm_phase_products / _update (both losses); aoadmm_phase_h_products / _h_solve / _w_products / _w_round x r / _w_close; the
    aoadmm_kl_phase_* set: step 2 through them passes the same checks.  One case per row of the table of DESIGN.md 4.9 at kp = 64
    and at kp = 128 (the KL losses: k = 100), and at k = 160 where the row has a generic phase (ADMM and AO-ADMM Euclidean, AO-ADMM KL)."""
    A.run_case(c, phases=True, single=False)


@cases(lambda c: _phase_pick(c) and (c.family, c.loss) == ("ao", "eu") and c.k <= 128)
def test_phase_protocol_fused_w(c):
    """The W sub-problem through aoadmm_phase_w_fused / _w_repair (all rounds speculatively, one decision)."""
    A.run_case(c, phases="fused", single=False)


# ---- knobs read once per process: child processes --------------------------------------------------------------------------------------
CHILD = r'''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import admm_step as A
c = A.Case(*json.loads(sys.argv[1]))
try:
    out = A.run_case(c)
    print(json.dumps({"ok": True, "paths": list(out[0].paths)}))
except AssertionError as e:
    print(json.dumps({"ok": False, "msg": str(e)}))
'''


@pytest.mark.parametrize("env,c", A.KNOB_CASES, ids=["=".join(*e.items()) for e, _ in A.KNOB_CASES])
def test_knobs(env, c):
    child_env = dict(os.environ)
    child_env.update(env)
    child_env["NMF_AMD_NO_TORCH"] = "1"
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, json.dumps(list(c))], env=child_env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"], out["msg"]
    if env.get("NMFX_AO_FUSED") == "0":
        assert out["paths"] == [0, 0, 0, 0]
