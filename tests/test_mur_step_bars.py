"""The bars of the element-wise MUR step checks (tests/mur_step.py), proven on the CPU: a numpy emulation of the device
arithmetic passes them with margin, and the faults the trajectory tests cannot see fail them, named by their tile.

Emulation: every f32 operand split into a bf16 hi part and a bf16 lo part, both rounded to nearest even (what split2 does
with v_cvt_pk_bf16_f32, kernels_bf16.hip); the bf16 x bf16 products are exact in f32 and accumulated in f32 (a float32
matmul: the order differs from the MFMA chains, the magnitude does not); the update ratio in f32."""
import numpy as np
import pytest

import mur_step as S
from oracle import nmf_ref as R

F = np.float32


def bf16(x):
    """Round f32 to the nearest bf16, ties to even (returned as f32)."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F)


def split2(x):
    x = np.asarray(x, dtype=F)
    hi = bf16(x)
    return hi, bf16(x - hi)


def prod(a, b, terms=3, drop=None):
    """a @ b as the device forms it: hi.hi + lo.hi + hi.lo (+ lo.lo with terms=4); terms='f32': the exact-f32 kernels.
    drop='lohi' | 'hilo' leaves that cross term out."""
    if terms == "f32":
        return np.asarray(a, F) @ np.asarray(b, F)
    ah, al = split2(a)
    bh, bl = split2(b)
    out = ah @ bh
    if drop != "lohi":
        out = out + al @ bh
    if drop != "hilo":
        out = out + ah @ bl
    if terms == 4:
        out = out + al @ bl
    return out


def emu_w(kind, v, w, h, lam, **kw):
    """One W half-step in the device's arithmetic (Euclidean: V H^T over W (H H^T); KL: W (V / (W H + eps)) H^T over the
    row sums of H, in the square-root form)."""
    v, w, h = (np.asarray(a, F) for a in (v, w, h))
    if kind == "eu":
        num = prod(v, h.T, **kw)
        den = prod(w, prod(h, h.T, **kw), **kw) + F(lam) * w + F(R.EPS)
        return (w * num / den).astype(np.float64)
    a = w * prod(v / (prod(w, h, **kw) + F(R.EPS)), h.T, **kw)
    b = h.sum(axis=1)[None, :]
    return (F(2) * a / (b + np.sqrt(b * b + F(4 * lam) * a))).astype(np.float64)


def emu_h(kind, v, w, h, lam, **kw):
    """The H half-step is the W half-step of the transposed problem."""
    return emu_w(kind, np.asarray(v).T, np.asarray(h).T, np.asarray(w).T, lam, **kw).T


def worst_and_msg(label, dev, ref, bar):
    return S.compare(label, dev, ref, bar, record=False)


# ---- the emulated device arithmetic passes, with margin -------------------------------------------------------------------
@pytest.mark.parametrize("kind,lam", [("eu", 0.0), ("eu", 0.1), ("kl", 0.0), ("kl", 0.1)])
@pytest.mark.parametrize("shape", [(4096, 2048, 64), (1539, 1285, 40), (257, 200, 128), (129, 130, 17)])
@pytest.mark.parametrize("terms", [3, 4, "f32"])
def test_emulated_step_passes_with_margin(kind, lam, shape, terms):
    """Both half-steps of the emulation (H from the emulated W) sit at least 3x under their bar."""
    m, n, k = shape
    v, w0, h0 = S.make_inputs(m, n, k, seed=m + k, edges=True, dead=kind == "eu", zeros=True)
    bar = S.BARS[("f32" if terms == "f32" else "bf16", kind)]
    w1 = emu_w(kind, v, w0, h0, lam, terms=terms)
    ew, msg = worst_and_msg("W1", w1, S.ref_w(kind, v, w0, h0, lam), bar / 3)
    assert msg is None, msg
    w1 = w1.astype(F).astype(np.float64)
    eh, msg = worst_and_msg("H1", emu_h(kind, v, w1, h0, 0.0, terms=terms), S.ref_h(kind, v, w1, h0, 0.0), bar / 3)
    assert msg is None, msg


# ---- faults the norm tests cannot see are rejected, and named --------------------------------------------------------------
M, N, K = 1539, 1285, 64          # ragged in both directions: 12 whole 128-row blocks + 3 rows, 20 whole 64-column groups + 5


@pytest.fixture(scope="module")
def case():
    v, w0, h0 = S.make_inputs(M, N, K, seed=11, edges=True)
    return v, w0, h0, S.ref_w("eu", v, w0, h0, 0.0)


def tile_of(msg):
    at = msg.index("128x64 tile (") + len("128x64 tile (")
    return tuple(int(t) for t in msg[at:msg.index(")", at)].split(", "))


@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("drop", ["lohi", "hilo"])
@pytest.mark.parametrize("blk", [0, 5])
def test_rejects_dropped_cross_term_in_one_row_block(kind, drop, blk, case):
    """One cross term of the split product lost for one 128-row block only.  It costs up to 2^-9 relative per partial
    product; over a long contraction of random data the losses average down (about 2e-4 for KL in a block of plain rows),
    the short contractions show it whole: the k-long Gram products, and row 3 of block 0 with its single non-zero."""
    v, w0, h0, _ = case
    w1 = emu_w(kind, v, w0, h0, 0.0)
    rows = slice(128 * blk, 128 * (blk + 1))
    w1[rows] = emu_w(kind, v[rows], w0[rows], h0, 0.0, drop=drop)
    ref = S.ref_w(kind, v, w0, h0, 0.0)
    worst, msg = worst_and_msg("W1", w1, ref, S.BARS[("bf16", kind)])
    assert msg is not None, f"a lost {drop} term in row block {blk} passed: worst {worst:.2e}"
    assert tile_of(msg)[0] == blk, msg


def test_rejects_missing_column_group_in_one_row_block(case):
    """The exact step with one 64-column group's contribution to one 128-row block of V H^T left out."""
    v, w0, h0, ref = case
    blk, grp = 7, 13
    rows, cols = slice(128 * blk, 128 * (blk + 1)), slice(64 * grp, 64 * (grp + 1))
    vht = np.asarray(v, np.float64) @ h0.T
    vht[rows] -= np.asarray(v[rows, cols], np.float64) @ h0[:, cols].T
    w1 = w0 * vht / ((w0 @ h0) @ h0.T + R.EPS)
    worst, msg = worst_and_msg("W1", w1, ref, S.BARS[("bf16", "eu")])
    assert msg is not None, f"a missing column group passed: worst {worst:.2e}"
    assert tile_of(msg)[0] == blk, msg
    assert "0 in the last, ragged tile row" in msg, msg


def test_rejects_ragged_last_column_copied_from_its_neighbour(case):
    """H1 exact except that the last (ragged) column is a copy of the one before it."""
    v, w0, h0, ref_w1 = case
    w1 = ref_w1.astype(F).astype(np.float64)
    ref = S.ref_h("eu", v, w1, h0, 0.0)
    h1 = ref.copy()
    h1[:, N - 1] = h1[:, N - 2]
    worst, msg = worst_and_msg("H1", h1, ref, S.BARS[("bf16", "eu")])
    assert msg is not None, f"a copied ragged column passed: worst {worst:.2e}"
    assert tile_of(msg)[1] == (N - 1) // 64, msg
    assert f"{K} in the last, ragged tile column (cols >= {N // 64 * 64})" in msg, msg


def test_rejects_one_tile_scaled_by_1e_3(case):
    """W1 = the float64 step, except one 64 x 64 tile scaled by (1 + 1e-3)."""
    v, w0, h0, ref = case
    w1 = ref.copy()
    w1[64 * 9:64 * 10, :] *= 1 + 1e-3
    worst, msg = worst_and_msg("W1", w1, ref, S.BARS[("bf16", "eu")])
    assert msg is not None, f"a scaled tile passed: worst {worst:.2e}"
    assert tile_of(msg) == (64 * 9 // 128, 0), msg
    assert f"{64 * 64} of {M * K} elements over the bar" in msg, msg


def test_exact_zeros_and_non_finite_values():
    """Where the reference is exactly 0 the device value must be 0 too; NaN / inf never pass."""
    ref = np.array([[0.0, 1.0], [2.0, 3.0]])
    assert worst_and_msg("X", ref.copy(), ref, 1e-4) == (0.0, None)
    for bad in (1e-30, np.nan):
        dev = ref.copy()
        dev[0, 0] = bad
        worst, msg = worst_and_msg("X", dev, ref, 1e-4)
        assert worst == np.inf and "(1 of them should be exact zeros)" in msg.replace("1 of 4 elements over the bar (", "(")
    dev = ref.copy()
    dev[1, 1] = np.inf
    assert worst_and_msg("X", dev, ref, 1e-4)[0] == np.inf


@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_blocked_references_equal_the_oracle_functions(kind):
    """ref_w / ref_h by row blocks (the full-size cases) = oracle mur_w_step / mur_h_step on the whole matrix."""
    v, w0, h0 = S.make_inputs(700, 300, 20, seed=3, edges=True)
    vv = v.astype(np.float64)
    np.testing.assert_allclose(S.ref_w(kind, v, w0, h0, 0.1, block=128), R.mur_w_step(kind, vv, w0, h0, w0 @ h0, 0.1), rtol=1e-12)
    np.testing.assert_allclose(S.ref_h(kind, v, w0, h0, 0.1, block=128), R.mur_h_step(kind, vv, w0, h0, w0 @ h0, 0.1), rtol=1e-12)


def test_split_counts_of_the_bench_shape():
    """The split configuration of 16384 x 8192, k = 64 with 256 CUs (the counts the GPU test comments quote)."""
    assert S.split_counts(16384, 8192, 64) == dict(wsplit=2, hsplit=4, bf_wsplit=2, bt_split=4, gram_ng_w=8, gram_ng_h=4)
