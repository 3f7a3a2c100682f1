"""Every ANLS half-step of the device, problem by problem, against float64 NNLS (tests/anls_step.py).

The trajectory tests compare norms after several iterations; a problem that kept its warm start, was solved with its
neighbour's right-hand side or was merely projected stays under those (tests/test_anls_step_bars.py shows it).  Here W_1, H_1,
W_2, H_2 are each checked against the float64 problem fed the device's own previous iterate: the KKT conditions of every
problem (check A) and the values against Lawson-Hanson (check B), and the fall-back counters of each run must show the NNLS
kernels the input regime is built for (csrc/kernels_anls.hip, gx_nnls_kernel in csrc/kernels_generic.hip):

    complement pass, kp 16 / 32 / 64 / 128     cold and zero at k <= 32, settled at 40 .. 128: no fall-back
    second complement pass (kp 128)            mixed at 100, 127, 128: fewer fall-backs than solutions beyond 36 zeros
    elimination kernels (kp <= 64, kp 128)     cold at k >= 64, zero at 29 / 32, mixed: fall-backs counted
    refused inverse                            dead: every half-step counted, evictions
    gx_nnls                                    k = 129, 160, 257 and 130
    grid-stride wraps                          test_grid_stride_wraps"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import anls_step as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cases(pred):
    sel = [c for c in A.CASES if pred(c)]
    return pytest.mark.parametrize("c", sel, ids=[A.case_id(c) for c in sel])


# ---- ranks at every padding and workspace edge ----------------------------------------------------------------------------------
@cases(lambda c: (c.m, c.n) == (257, 200) and c.k <= 32)
def test_ranks_kp16_kp32(c):
    A.run_case(c)


@cases(lambda c: (c.m, c.n) == (257, 200) and c.regime == "mixed" and 33 <= c.k <= 128)
def test_ranks_kp64_kp128(c):
    A.run_case(c)


# ---- regimes ----------------------------------------------------------------------------------------------------------------------
@cases(lambda c: c.regime in ("settled", "cold", "dead") and c.k >= 40)
def test_regimes(c):
    A.run_case(c)


# ---- shapes: problem counts of 4 q + 1 and 6 q + 1, single rows and columns ------------------------------------------------------
@cases(lambda c: c.regime == "mixed" and c.k <= 128 and (c.m, c.n) != (257, 200) and max(c.m, c.n) < 600)
def test_shapes(c):
    A.run_case(c)


# ---- more problems than one round of the grid-stride loops ----------------------------------------------------------------------
@cases(lambda c: max(c.m, c.n) >= 600)
def test_grid_stride_wraps(c):
    assert max(c.m, c.n) > A.wrap_stride(c.k)
    A.run_case(c)


# ---- the row-sharded protocol with a world of one --------------------------------------------------------------------------------
@cases(lambda c: c.regime == "mixed" and (((c.m, c.n) == (257, 200) and c.k in (40, 128) and c.arith == "bf16")
                                          or (c.k == 160 and c.arith == "f32")))
def test_phase_protocol(c):
    """anls_phase_objective / anls_phase_w / anls_phase_h pass the same checks, and W_1 read after anls_phase_w alone is the
    W_1 of the one-iteration run within the two bars (beyond 128 components the phase form runs the exact-f32 products, the
    run the split-bf16 ones)."""
    out = A.run_case(c, phases=True)
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = A.lam_of(c)
    runs, arith = A.run_anls(v, w0, h0, lw, lh, "eu", c.arith if c.k <= 128 else None, steps=(1,))
    other = A.Case(c.regime, c.m, c.n, c.k, arith)
    w_run, w_mid = runs[1].w, out["w_mid"]
    dev = np.abs(w_run - w_mid).max(axis=1) / np.maximum(w_run.max(axis=1), 1e-300)
    A._record("W1 phase vs run", float(dev.max()), A.bar_of(c) + A.bar_of(other))
    assert dev.max() <= A.bar_of(c) + A.bar_of(other), f"row {int(np.argmax(dev))}: {dev.max():.3e}"
    assert ((w_run == 0) == (w_mid == 0)).mean() > 0.999


# ---- determinism: the only atomics are the counters ------------------------------------------------------------------------------
@cases(lambda c: c.regime == "mixed" and (c.m, c.n) == (257, 200) and c.k in (64, 128) and c.arith == "bf16")
def test_two_runs_bit_identical(c):
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = A.lam_of(c)
    a, _ = A.run_anls(v, w0, h0, lw, lh, steps=(2,))
    b, _ = A.run_anls(v, w0, h0, lw, lh, steps=(2,))
    for x, y, name in zip(a[2][:3], b[2][:3], ("W2", "H2", "objective history")):
        assert np.array_equal(x, y), f"{name}: {int(np.sum(x != y))} elements differ between two identical runs"
    assert a[2].fallbacks == b[2].fallbacks and a[2].diagnostics == b[2].diagnostics


# ---- knobs read once per process: child processes --------------------------------------------------------------------------------
CHILD = r'''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import anls_step as A
c = A.Case(*json.loads(sys.argv[1]))
try:
    out = A.run_case(c)
    print(json.dumps({"ok": True, "fallbacks": [list(out["eu"][0][s].fallbacks) for s in (1, 2)]}))
except AssertionError as e:
    print(json.dumps({"ok": False, "msg": str(e)}))
'''


def run_child(c, env):
    child_env = dict(os.environ)
    child_env.update(env)
    child_env["NMF_AMD_NO_TORCH"] = "1"
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, json.dumps(list(c))], env=child_env, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"], out["msg"]
    return out


@cases(lambda c: c.k > 128 and c.k != 130)
def test_ranks_beyond_128(c):
    """gx_nnls; the default arithmetic in this process, NMFX_GX_ANLS_BF16=0 (exact-f32 products) in a child."""
    if c.arith == "f32":
        run_child(c, {"NMFX_GX_ANLS_BF16": "0"})
    else:
        A.run_case(c)


@cases(lambda c: c.regime == "mixed" and (c.m, c.n) == (257, 200) and c.k in (40, 100) and c.arith == "bf16")
def test_elimination_kernels_alone(c):
    """NMFX_NNLS_CINV=0: every problem of the mixed launches on the elimination kernels."""
    out = run_child(c, {"NMFX_NNLS_CINV": "0"})
    assert out["fallbacks"] == [[0, 0], [0, 0]]
