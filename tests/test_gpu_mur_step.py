"""Every MUR half-step of the device, element by element, against the float64 step of the oracle (tests/mur_step.py).

The trajectory tests compare norms over the whole matrix after many iterations; a fault confined to a row, a tile or a split
range of one launch stays under those.  Here W_1, H_1, W_2, H_2 are each compared with oracle/nmf_ref.py:mur_w_step /
mur_h_step fed the device's own previous iterate, and a failure names the element and its 128 x 64 tile.

Split counts in the comments: (bf_wsplit, bt_split) of the split-bf16 W / H phase and (wsplit, hsplit) of the exact-f32
phases, from mur_step.split_counts with 256 CUs (engine.hip nmfx_create, kernels_bf16.hip nmfx_bf16_prepare)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import mur_step as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMS = [(0.0, 0.0), (0.1, 0.0), (0.0, 0.2)]       # lambda = 0, and lambda > 0 on one side


def run_case(m, n, k, kind, precision=None, lam=(0.0, 0.0), seed=0):
    edges = m >= 8 and n >= 8        # (m or n = 1: no scattered zeros either -- a zero column sum makes the KL reference 0 / 0)
    v, w0, h0 = S.make_inputs(m, n, k, seed=seed + m + n + k, edges=edges, dead=kind == "eu" and k >= 2, zeros=edges and k >= 2)
    runs, arith = S.run_dense(v, w0, h0, kind, lam[0], lam[1], precision=precision)
    if precision == "bf16" and k > 32:
        assert arith == "bf16"
    return S.check_steps(kind, v, w0, h0, runs, lam[0], lam[1], S.BARS[(arith, kind)]), runs


# ---- ranks: every padding boundary at a shape ragged in both directions ------------------------------------------------------
# 257 x 200 (mp 384, np 256): split-bf16 (1, 1), exact-f32 (1, 6); kp 16 / 32 run the exact-f32 kernels only
@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("k", [1, 16, 17, 32])
def test_ranks_kp16_kp32(k, kind):
    run_case(257, 200, k, kind, lam=LAMS[k % 3])


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("k", [33, 63, 64, 65, 127, 128, 129, 160, 256, 257, 400])       # kp 64, 128; composed 256, 384, 512
def test_ranks_kp64_kp128_composed(k, kind, precision):
    run_case(257, 200, k, kind, precision=precision, lam=LAMS[k % 3])


# ---- shapes straddling the 128-row / 64-column tiles, the 256 x 256 and 256 x 128 composed tiles ----------------------------
# every (m, n) here has split-bf16 (1, 1); exact-f32 (1, 2) for m <= 128, (1, 4) for 129..256, (1, 6) for 257
SMALL = [(1, 257), (63, 129), (64, 64), (65, 255), (127, 1), (128, 256), (129, 63), (255, 65), (256, 128), (257, 127)]


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("k", [40, 100, 160])
@pytest.mark.parametrize("shape", SMALL, ids=[f"{m}x{n}" for m, n in SMALL])
def test_edge_shapes(shape, k, kind, precision):
    run_case(*shape, k, kind, precision=precision, lam=LAMS[(shape[0] + k) % 3])


# n = 64 * 37 + 1 (np 2432 = 38 column groups): split-bf16 (9, 2) -- 38 groups over 9 W slabs --, exact-f32 (9, 8);
# NMFX_WBLOCKS=24 NMFX_HBLOCKS=100: split-bf16 (3, 2), exact-f32 (3, 3) -- 38 groups over 3 slabs
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("forced", [False, True])
def test_odd_column_groups_over_the_slabs(forced, kind, precision, monkeypatch):
    if forced:
        monkeypatch.setenv("NMFX_WBLOCKS", "24")
        monkeypatch.setenv("NMFX_HBLOCKS", "100")
    run_case(512, 64 * 37 + 1, 64, kind, precision=precision, lam=(0.05, 0.0) if kind == "eu" else (0.0, 0.05))


# 512 x 512 at k = 160: whole 256 x 256 tiles of the composed path; split-bf16 (2, 2), exact-f32 (2, 8)
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_composed_whole_tiles(kind, precision):
    run_case(512, 512, 160, kind, precision=precision, lam=(0.1, 0.0))


# ... with lambda > 0 on both sides: both fused update launches (update + images behind the denominator product) carry their lambda
def test_composed_whole_tiles_both_lambdas():
    run_case(512, 512, 160, "eu", precision="bf16", lam=(0.1, 0.05))


# m = 128 * 257 + 1, n = 384: 258 row blocks of 128, more than the 256 CUs; split-bf16 (1, 85) -- 514 groups of 64 rows over
# 85 H slabs --, exact-f32 (1, 85)
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_more_row_blocks_than_cus(kind, precision):
    run_case(128 * 257 + 1, 384, 64, kind, precision=precision)


# ---- full size: the bench problem and the k = 128 matrix-bound kernel; non-temporal V (V + V^T > 192 MiB) --------------------
# 16384 x 8192: split-bf16 (2, 4), exact-f32 (2, 4)
@pytest.mark.parametrize("k,kind,precision", [(64, "eu", "bf16"), (64, "eu", "f32"), (64, "kl", None), (128, "eu", None)])
def test_full_size(k, kind, precision):
    run_case(16384, 8192, k, kind, precision=precision)


# ---- determinism: a race in an epilogue or a slab sum shows as a difference between two identical runs ----------------------
@pytest.mark.parametrize("m,n,k,kind", [(16384, 8192, 64, "eu"), (1539, 1285, 64, "eu"), (1539, 1285, 100, "kl"),
                                        (1539, 1285, 160, "eu")])
def test_two_runs_bit_identical(m, n, k, kind):
    v, w0, h0 = S.make_inputs(m, n, k, seed=5, edges=True, zeros=True)
    a, _ = S.run_dense(v, w0, h0, kind, steps=(2,))
    b, _ = S.run_dense(v, w0, h0, kind, steps=(2,))
    for x, y, name in zip(a[2], b[2], ("W2", "H2", "objective history")):
        assert np.array_equal(x, y), f"{name}: {int(np.sum(x != y))} elements differ between two identical runs"


# ---- pair mode: two Euclidean problems in the halves of one k = 128 handle ----------------------------------------------------
@pytest.mark.parametrize("ks,lws,lhs", [((40, 24), (0.1, 0.0), (0.0, 0.05)), ((5, 64), (0.0, 0.2), (0.1, 0.0))])
def test_pair_mode(ks, lws, lhs):
    m, n = 300, 257
    v, _, _ = S.make_inputs(m, n, 1, seed=9, edges=True)
    starts = [S.make_inputs(m, n, kk, seed=20 + p, zeros=True)[1:] for p, kk in enumerate(ks)]
    out = S.run_pair(v, starts, lws, lhs)
    fails = []
    for p in (0, 1):
        try:
            S.check_steps("eu", v, *starts[p], out[p], lws[p], lhs[p], S.BARS[("bf16", "eu")], tag=f"problem {p}: ")
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


# ---- sparse V: every sparse kp (4, 8, 16, 32, 64, 128, 256), rows and columns beyond the 256-entry unit, empty rows / columns --
def sparse_input(m, n, density, seed):
    rng = np.random.default_rng(seed)
    x = sp.random(m, n, density=density, format="lil", random_state=seed,
                  data_rvs=lambda s: rng.uniform(0.05, 1.0, s).astype(np.float32))
    x[7, :] = rng.uniform(0.05, 1.0, (1, n)).astype(np.float32)            # a row of n > 256 entries
    x[:, 11] = rng.uniform(0.05, 1.0, (m, 1)).astype(np.float32)           # a column of m > 256 entries
    x[2, :] = 0                                                             # an empty row and an empty column
    x[:, 3] = 0
    return sp.csr_matrix(x, dtype=np.float32)


@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("k", [1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256])
def test_sparse(k, kind):
    m, n = 700, 600
    x = sparse_input(m, n, 0.02, seed=k)
    v = x.toarray()
    _, w0, h0 = S.make_inputs(m, n, k, seed=k + 1, zeros=k >= 2)
    lam = LAMS[k % 3]
    runs = S.run_sparse(x, w0, h0, kind, lam[0], lam[1])
    S.check_steps(kind, v, w0, h0, runs, lam[0], lam[1], S.BARS[("f32", kind)])


# ---- knobs read once per process: child processes ----------------------------------------------------------------------------
CHILD = r'''
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import mur_step as S
spec = json.loads(sys.argv[1])
m, n, k = spec["shape"]
kind = spec["kind"]
lw, lh = spec["lam"]
v, w0, h0 = S.make_inputs(m, n, k, seed=m + n + k, edges=True, dead=kind == "eu", zeros=True)
runs, arith = S.run_dense(v, w0, h0, kind, lw, lh)
try:
    worst = S.check_steps(kind, v, w0, h0, runs, lw, lh, S.BARS[(arith, kind)])
    print(json.dumps({"ok": True, "worst": max(val for key, val in worst.items() if not key.startswith("obj")), "arith": arith}))
except AssertionError as e:
    print(json.dumps({"ok": False, "msg": str(e)}))
'''

KNOBS = [
    # (environment, shape, kind, (lambda_w, lambda_h)) -- one small shape per knob where it changes the path
    ({"NMFX_BF16_TERMS": "4"}, (384, 256, 40), "eu", (0.1, 0.0)),          # four split terms
    ({"NMFX_BF16_TERMS": "4"}, (384, 256, 100), "kl", (0.0, 0.1)),
    ({"NMFX_TEMPORAL": "0"}, (640, 384, 64), "eu", (0.0, 0.0)),            # small V is temporal by default
    ({"NMFX_TEMPORAL": "1"}, (5120, 5121, 64), "eu", (0.0, 0.0)),          # V + V^T > 192 MiB: non-temporal by default
    ({"NMFX_GXT2": "0"}, (512, 512, 160), "eu", (0.0, 0.0)),               # composed path: whole 256 x 256 tiles, taken by default here
    ({"NMFX_GX_DEN_BF16": "0"}, (512, 256, 400), "eu", (0.05, 0.0)),       # k pads to 512: exact-f32 denominator
    ({"NMFX_GXB_NOFIT": "1"}, (384, 256, 160), "kl", (0.0, 0.1)),          # the exact-f32 product kernel beyond 128 components
]


@pytest.mark.parametrize("env,shape,kind,lam", KNOBS, ids=[f"{'-'.join(f'{a}={b}' for a, b in e.items())}-{s[0]}x{s[1]}x{s[2]}-{kd}"
                                                           for e, s, kd, _ in KNOBS])
def test_knob_paths(env, shape, kind, lam):
    child_env = dict(os.environ)
    child_env.update(env)
    child_env["NMF_AMD_NO_TORCH"] = "1"
    spec = json.dumps({"shape": list(shape), "kind": kind, "lam": list(lam)})
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, spec], env=child_env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"], out["msg"]
    S._record("knob child worst", out["worst"], S.BARS[(out["arith"], kind)])
