"""The bars, sweep caps and inputs of the device top-k SVD checks (tests/svd_ref.py, tests/test_gpu_svd.py), proven on the CPU.

Per case the numpy statement of the algorithm (svd_ref.emulate_topk) runs with seeds 0 to 3; a bar is the documented one or 10 x
the worst deviation of the four runs from LAPACK, whichever is larger, and the sweep cap 2 x the most sweeps + 2 (svd_ref.TABLE,
held here to a fresh measurement).  Asserted: LAPACK's own triplets pass every case at the documented bars (the inputs lie in
the comparator's domain), the emulation passes at the table's bars, and of eight planted faults -- three in the returned triplets,
five inside the iteration -- seven are each rejected by check_triplets or by the sweep cap; the eighth (padded rows of the start
block not zero) is cleared by the first sweep itself and costs one sweep, which is what is asserted of it.  Not reproduced by the emulation: the
threshold Jacobi solver (numpy.linalg.eigh stands for it), the MFMA summation order and the mt19937_64 start block; the factor
10 is for those."""
import numpy as np
import pytest

import svd_ref as S

ALL = S.CASES + [S.WIDE_BLOCK]
IDS = [c.id for c in ALL]
_MEASURED = {}


def measured(c):
    if c.id not in _MEASURED:
        _MEASURED[c.id] = S.measure_bars(c)
    return _MEASURED[c.id]


def emulate(c, **over):
    kw = dict(c.kw)
    kw.update(over)
    return S.emulate_topk(S.make_input(c), c.k, **kw)


# ---- the table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_table_holds_the_measured_bars(c):
    fresh, worst, sweeps = measured(c)
    table = S.bars_of(c)
    for q in S.DOC:
        if fresh[q] is None or table[q] is None:
            assert fresh[q] is None and table[q] is None, (c.id, q, fresh[q], table[q])
        elif fresh[q] == S.DOC[q] and table[q] == S.DOC[q]:
            continue
        else:       # a bar above the documented one: the table's is the fresh one rounded up, never below 10 x the emulation
            assert fresh[q] <= table[q] <= 2.0 * fresh[q], (c.id, q, fresh[q], table[q])
    assert fresh["sweep_cap"] <= table["sweep_cap"] <= fresh["sweep_cap"] + 4, (c.id, fresh["sweep_cap"], table["sweep_cap"])
    assert S.block_width(c.k, dict(c.kw).get("block", 0)) == S.emulate_topk(S.make_input(c), c.k, max_sweeps=1, **{k: v for k, v in c.kw if k == "block"})[5]
    print(f"{c.id}: emulation worst values {worst['values']:.1e} orth {worst['orth']:.1e} vectors {worst['vectors']:.1e} recon {worst['recon']:.1e} "
          f"resid {worst['resid']:.1e}, {sweeps} sweeps; bars {table}")


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_emulation_passes_at_the_table(c):
    u, s, vt, sweeps, resid, _ = emulate(c)
    fails, _ = S.check_triplets(S.make_input(c), u, s, vt, resid, c.k, S.bars_of(c))
    assert not fails, "\n".join(fails)
    assert sweeps <= S.bars_of(c)["sweep_cap"]


@pytest.mark.parametrize("c", ALL + [S.TWO_SWEEPS], ids=IDS + [S.TWO_SWEEPS.id])
def test_lapack_passes_at_the_documented_bars(c):
    v = S.make_input(c)
    _, ur, sr, vtr = S.lapack(v)
    u, s, vt = ur[:, :c.k], sr[:c.k], vtr[:c.k]
    fails, dev = S.check_triplets(v, u, s, vt, S.recompute_resid(v, u, s, vt), c.k, S.DOC)
    assert not fails, "\n".join(fails)


def test_case_table_covers_every_block_width_and_edge():
    widths = [S.block_width(c.k, dict(c.kw).get("block", 0)) for c in S.CASES]
    assert set(widths) == set(S.SIZES)
    assert [S.block_width(k) for k in S.WIDTHS] == list(S.WIDTHS_L)
    for a, b in ((16, 17), (32, 33), (43, 44), (64, 65), (85, 86), (107, 108)):
        assert a in S.WIDTHS and b in S.WIDTHS and S.block_width(a) < S.block_width(b)
    by = S.BY_ID
    assert S.block_width(by["L>n-700x40-k20"].k) > by["L>n-700x40-k20"].n
    assert S.block_width(by["L>np-300x100-k100"].k) > 128 >= by["L>np-300x100-k100"].n
    assert all(by[i].k == min(by[i].m, by[i].n) for i in ("k=n-300x24", "k=m-24x300", "1x300", "300x1"))
    for cid, rank in (("rank6-k10", 6), ("tiled8-k12", 8)):
        sr = S.lapack(S.make_input(by[cid]))[2]
        assert int(np.sum(sr > S.RANK_REL * sr[0])) == rank < by[cid].k
    sr = S.lapack(S.make_input(by["repeated-k6"]))[2]
    assert sr[5] - sr[6] > 0.5 and abs(sr[4] - sr[5]) < S.EQUAL * sr[0] and abs(sr[1] - sr[3]) < S.EQUAL * sr[0]     # k on a cluster boundary
    assert len(set(IDS)) == len(IDS)


# ---- planted faults ----------------------------------------------------------------------------------------------------------
K64, K85, K70, WIDE, K_N = (S.BY_ID[i] for i in ("L96-k64", "L128-k85", "k70-seed0", "wide-130x1000-k64", "k=n-300x24"))


def _zeroed(u, s, vt, j):
    u[:, j] = 0
    s[j] = 0


def _swapped(u, s, vt, j):
    s[[j, j + 1]] = s[[j + 1, j]]


def _negated(u, s, vt, j):
    vt[j] = -vt[j]


# fault: (how it is planted, the triplet, the check that must name the triplet).  Of the planted matrices only triplet 0 is
# separated by GAP sr_0, so a negated vt[0] is named by the vector check and a negated vt[5] by the residual taken again.
OUTPUT_FAULTS = {"zeroed triplet": (_zeroed, 7, "[orthonormality]"), "values swapped": (_swapped, 7, "[values]"),
                 "vt[0] negated": (_negated, 0, "[vectors, vt]"), "vt[5] negated": (_negated, 5, "[residual]")}


@pytest.mark.parametrize("fault", list(OUTPUT_FAULTS))
def test_fault_in_the_returned_triplets_is_rejected_and_named(fault):
    plant, j, check = OUTPUT_FAULTS[fault]
    c = K70
    u, s, vt, sweeps, resid, _ = emulate(c)
    plant(u, s, vt, j)
    fails, _ = S.check_triplets(S.make_input(c), u, s, vt, resid, c.k, S.bars_of(c))
    hits = [f for f in fails if f.startswith(check)]
    assert hits, f"{fault}: not rejected by {check}:\n" + "\n".join(fails)
    assert any(f"triplet {j}" in h or f"[{j}, {j}]" in h for h in hits), (j, hits)
    if fault == "vt[5] negated":
        assert any(f.startswith("[reconstruction]") for f in fails)
    print(f"{fault} (triplet {j} of {c.id}): {hits[0][:170]}")


# fault of emulate_topk: (case, what it is)
ITERATION_FAULTS = {
    "gram_tile4": (K85, "tile column 4 (columns 64 to 79) missing from the Gram of Y: the second pass of the waves"),
    "stale_block": (K64, "rows 64 to 127 of U left from the sweep before"),
    "drop_chunk": (WIDE, "the last 32-column chunk of the contraction missing from V Q"),
    "no_deflation": (K64, "the locked pairs not deflated from the filtered operator"),
}


@pytest.mark.parametrize("fault", list(ITERATION_FAULTS))
def test_fault_inside_the_iteration_is_rejected(fault):
    c, what = ITERATION_FAULTS[fault]
    bars = S.bars_of(c)
    seen = []
    for seed in (0, 1):
        u, s, vt, sweeps, resid, _ = emulate(c, seed=seed, fault=fault, max_sweeps=bars["sweep_cap"] + 1)
        fails, _ = S.check_triplets(S.make_input(c), u, s, vt, resid, c.k, bars)
        over = sweeps > bars["sweep_cap"]
        assert fails or over, f"{fault} ({what}), seed {seed}: passes every check in {sweeps} sweeps"
        seen.append(f"seed {seed}: " + (f"{sweeps} sweeps against a cap of {bars['sweep_cap']}" if over else "") + ("; " if over and fails else "")
                    + (fails[0][:150] if fails else ""))
    print(f"{fault} ({c.id}; {what}): " + " | ".join(seen))


def test_nonzero_padding_of_the_start_block_costs_one_sweep_and_nothing_else():
    """The one planted fault that neither check_triplets nor the sweep cap can reject: padded rows of the start block that are
    not zero.  V's padded columns are zero, so V Q never reads them, and the next block orth(V^T U) has zero padded rows again:
    the fault is gone behind the first sweep.  What it leaves is one more sweep at 300 x 24, k = n = 24, where the clean run needs a single one (the
    block spans the whole row space): the first Ritz vectors carry weight in the padding and miss the stop test."""
    for c in (K_N, S.BY_ID["L>np-300x100-k100"], K64):
        clean, bad = emulate(c), emulate(c, fault="pad_start")
        fails, _ = S.check_triplets(S.make_input(c), *bad[:3], bad[4], c.k, S.bars_of(c))
        assert not fails, "\n".join(fails)
        assert clean[3] <= bad[3] <= (clean[3] + 1 if clean[3] == 1 else S.bars_of(c)["sweep_cap"]), (c.id, clean[3], bad[3])
    assert emulate(K_N)[3] == 1 and emulate(K_N, fault="pad_start")[3] == 2


def test_stale_block_is_placed_in_its_rows():
    c = K64
    u, s, vt, sweeps, resid, _ = emulate(c, fault="stale_block", max_sweeps=S.bars_of(c)["sweep_cap"] + 1)
    fails, _ = S.check_triplets(S.make_input(c), u, s, vt, resid, c.k, S.bars_of(c))
    named = [f for f in fails if "64-row block 1)" in f or "64-row block 1 " in f or f.rstrip().endswith("64-row block 1")]
    assert named, "\n".join(fails)


# ---- null triplets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["rank6-k10", "tiled8-k12"])
def test_rank_below_k_gives_orthonormal_null_triplets_and_a_finite_nndsvd(cid):
    from nmf_amd import utils
    c = S.BY_ID[cid]
    v = S.make_input(c)
    u, s, vt, sweeps, resid, _ = emulate(c)
    sr = S.lapack(v)[2]
    r = int(np.sum(sr > S.RANK_REL * sr[0]))
    assert np.all(s[r:] <= S.NULL_ABS * sr[0]) and resid <= 1e-11
    assert np.max(np.abs(u.T @ u - np.eye(c.k))) < 1e-10 and np.max(np.abs(vt @ vt.T - np.eye(c.k))) < 1e-10
    x = v.astype(np.float64)
    for variant in ("zero", "mean"):
        w, h = utils._nndsvd_from_triplets(x, u, s, vt, c.k, variant)
        wr, hr = utils.nndsvd(x, c.k, variant=variant)
        assert np.isfinite(w).all() and np.isfinite(h).all() and w.min() >= 0 and h.min() >= 0
        np.testing.assert_allclose(w[:, :r], wr[:, :r], rtol=0, atol=1e-7 * wr.max())
        np.testing.assert_allclose(h[:r], hr[:r], rtol=0, atol=1e-7 * hr.max())
        # W0 H0: with 'mean' the host's own product depends on the signs LAPACK happens to give its null vectors (their
        # zero parts are what the mean fills), so there it is compared over the r columns that are defined
        c0 = c.k if variant == "zero" else r
        np.testing.assert_allclose(w[:, :c0] @ h[:c0], wr[:, :c0] @ hr[:c0], rtol=0, atol=1e-7 * (wr @ hr).max())
        if variant == "mean":
            assert np.all(w[:, r:] == np.mean(x)) and np.all(h[r:] == np.mean(x))


def test_nndsvd_gives_a_zero_column_for_a_zero_part_norm():
    """A triplet whose vectors are zero (what the device returned for a null triplet before it completed them) or whose value is
    zero: the column of W0 and the row of H0 are zero, not 0 / 0."""
    from nmf_amd import utils
    rs = np.random.RandomState(3)
    x = rs.rand(9, 7)
    ur, sr, vtr = np.linalg.svd(x, full_matrices=False)
    u, s, vt = ur[:, :4].copy(), sr[:4].copy(), vtr[:4].copy()
    u[:, 2], vt[2], s[2] = 0, 0, 0
    s[3] = 0
    with np.errstate(all="raise"):
        w, h = utils._nndsvd_from_triplets(x, u, s, vt, 4, "zero")
    assert np.isfinite(w).all() and np.isfinite(h).all()
    assert not w[:, 2:].any() and not h[2:].any() and w[:, 1].any() and h[1].any()
    wr, hr = utils._nndsvd_from_triplets(x, ur, sr, vtr, 4, "zero")
    assert np.array_equal(w[:, :2], wr[:, :2]) and np.array_equal(h[:2], hr[:2])
