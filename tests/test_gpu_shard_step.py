"""The row-sharded MUR phases over several shards, element by element against the float64 step (tests/shard_step.py).

Several engine handles in ONE process, one per row shard, the collective done on the host between the phase calls: the
sharded-only device code -- nmfx_launch_pack_from, the chunk product and mur_pack_cols_kernel, the objective digits in the
tail of the f32 buffer, the sliced H update that overwrites its own B^T tile, mur_h_unpack_bf16_kernel, the k = 128 Gram
matrix behind `rest` -- goes through the checks of tests/mur_step.py that the single-handle path has.  Every case takes two
steps: step 2 reads the images and leftovers the sharded epilogues of step 1 wrote.  All cases:

  (a) every half-step and every recorded objective against float64 fed the device's previous iterate (rank 0's H);
  (b) H, the objective history and the state are bit-identical on every rank;
  (c) after phase A of step 1 each shard's exchange buffer holds its own partial products, in the documented layout;
  (d) the recorded objectives are the float64 sums of the shards' partials in rank order, bit for bit, and with the
      objective inside the f32 buffer slot r of its tail holds rank r's digits and every other slot +0.0.

Not covered here: RCCL, more than one device, hipGraph replay (tests/test_gpu_dist.py)."""
import numpy as np
import pytest

import mur_step as S
import shard_step as X
from nmf_amd import dist as nd
from test_gpu_mur_step import LAMS

pytestmark = pytest.mark.gpu

CUTS4 = [0, 1, 128, 257, 557]                   # 1, 127, 129 and 300 rows: one row, a ragged tile, a tile and a row, several tiles
INPUTS = {}


def inputs(m, n, k, kind):
    key = (m, n, k, kind)
    if key not in INPUTS:
        INPUTS[key] = S.make_inputs(m, n, k, seed=m + n + k, edges=True, dead=kind == "eu", zeros=True)
    return INPUTS[key]


def balanced(m, world):
    return [nd.row_range(m, r, world)[0] for r in range(world)] + [m]


def sharded(m, n, k, kind, cuts, form, lam=None, snapshot=True, **kw):
    """Runs the case and applies (a) - (d); returns (inputs, runs, lambdas)."""
    v, w0, h0 = inputs(m, n, k, kind)
    lw, lh = LAMS[k % 3] if lam is None else lam
    runs = X.run_sharded(v, w0, h0, kind, lw, lh, cuts, form, snapshot=snapshot, **kw)
    bar = S.BARS[(runs[1].arith, kind)]
    fails = []
    for what in (lambda: X.check(kind, v, w0, h0, runs, lw, lh, bar),                                    # (a)
                 lambda: X.check_partials(kind, v, runs[1], runs[1].w, h0, bar) if snapshot else None,   # (c)
                 lambda: [X.check_objective_sums(r) for r in runs.values()]):                            # (d)
        try:
            what()
        except AssertionError as e:
            fails.append(str(e))
    for s, r in sorted(runs.items()):                                                                   # (b)
        fails += [f"{s}-step run: {d}" for d in X.ranks_differ(r)]
        if any(st != (0, -1, s + 1) for st in r.states):
            fails.append(f"{s}-step run: states {r.states}, expected (0, -1, {s + 1}) everywhere")
    assert not fails, "\n".join(fails)
    return (v, w0, h0), runs, (lw, lh)


def same_results(a, b, what):
    for s in a:
        assert np.array_equal(a[s].w, b[s].w), f"{what}: W_{s} differs in {int(np.sum(a[s].w != b[s].w))} elements"
        assert np.array_equal(a[s].hs[0], b[s].hs[0]), f"{what}: H_{s} differs in {int(np.sum(a[s].hs[0] != b[s].hs[0]))} elements"
        assert np.array_equal(a[s].objs[0], b[s].objs[0]), f"{what}: objective history of the {s}-step run differs: {a[s].objs[0]} / {b[s].objs[0]}"


# ---- all-reduce form: every width of the factor, both losses, four ragged shards ------------------------------------------------
# n = 200 (np 256).  k = 12: kp 16, 20: kp 32 (exact f32 whatever the mode); 40, 64: kp 64; 100, 128: kp 128; 160: composed
@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("k", [12, 20, 40, 64, 100, 128, 160])
def test_allreduce_four_ragged_shards(k, kind):
    _, runs, _ = sharded(557, 200, k, kind, CUTS4, "allreduce")
    assert runs[1].form == "allreduce"
    split = runs[1].arith == "bf16" and 32 < k <= 128          # the split-bf16 kernels of k padded to 64 / 128
    assert runs[1].merged == (kind == "eu" and split)
    assert runs[1].layouts[0]["transposed"] == (kind == "eu" and split)


@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("k", [40, 100, 160])
def test_allreduce_four_ragged_shards_f32(k, kind):
    _, runs, _ = sharded(557, 200, k, kind, CUTS4, "allreduce", precision="f32")
    assert runs[1].arith == "f32" and not runs[1].merged and not runs[1].layouts[0]["transposed"]


# ---- the objective inside the f32 buffer against the separate f64 sum: the same partials in the same order ----------------------
@pytest.mark.parametrize("k", [40, 100])
def test_merge_on_equals_merge_off(k):
    _, on, _ = sharded(557, 200, k, "eu", CUTS4, "allreduce")
    _, off, _ = sharded(557, 200, k, "eu", CUTS4, "allreduce", merge=False)
    assert on[1].merged and not off[1].merged
    same_results(on, off, "merge on / off")


# ---- five shards at ranks 0, 31, 32, 62, 63 of a world of 64: the absent ranks contribute zeros -------------------------------
def test_sparse_world_of_64():
    _, runs, _ = sharded(300, 200, 40, "eu", balanced(300, 5), "allreduce", ranks=[0, 31, 32, 62, 63], world=64)
    assert runs[2].merged and runs[2].world == 64 and runs[2].cuts[-1] == 300


# ---- phase A in column chunks ------------------------------------------------------------------------------------------------
CHUNKS = [(400, 1100, [(0, 512), (512, 1152)]),               # the second chunk is the larger one: its slab buffer is reallocated
          (400, 1600, [(0, 512), (512, 1024), (1024, 1664)]),
          (400, 1024, [(0, 1024)]),
          (1600, 1100, [(0, 512), (512, 1152)])]              # 534 rows per shard (mp 640): two reduction splits per chunk launch


@pytest.mark.parametrize("k", [40, 100])
@pytest.mark.parametrize("m,n,ranges", CHUNKS, ids=[f"{m}x{n}" for m, n, _ in CHUNKS])
def test_chunks(m, n, ranges, k):
    _, runs, _ = sharded(m, n, k, "eu", balanced(m, 3), "chunks", ranges=ranges)
    assert runs[1].form == "chunks" and runs[1].merged


# ---- reduce-scatter / all-gather form: bit-identical to the all-reduce on the same cuts -----------------------------------------
RSAG = [(2, 200, 128), (3, 330, 128), (4, 500, 128)]           # (world, n, columns per rank)


@pytest.mark.parametrize("k", [40, 100])
@pytest.mark.parametrize("world,n,cols", RSAG, ids=[f"world{w}" for w, _, _ in RSAG])
def test_rsag_equals_allreduce(world, n, cols, k):
    cuts = balanced(300, world)
    _, sliced, _ = sharded(300, n, k, "eu", cuts, "rsag")
    assert sliced[1].form == "rsag" and sliced[1].merged
    assert -(-n // 128) * 128 == world * cols
    _, plain, _ = sharded(300, n, k, "eu", cuts, "allreduce", snapshot=False)
    same_results(sliced, plain, "rsag / allreduce")


def test_rsag_without_slices_takes_the_allreduce():
    _, runs, _ = sharded(300, 257, 40, "eu", balanced(300, 4), "rsag")      # np 384: six column blocks over four ranks
    assert runs[1].requested == "rsag" and runs[1].form == "allreduce"


# ---- a world of one through the phase calls against the plain handle ------------------------------------------------------------
@pytest.mark.parametrize("k", [40, 100, 12])
def test_world_of_one_against_the_plain_handle(k):
    (v, w0, h0), runs, (lw, lh) = sharded(557, 200, k, "eu", [0, 557], "allreduce")
    plain, arith = S.run_dense(v, w0, h0, "eu", lw, lh)
    assert arith == runs[1].arith
    bar = S.BARS[(arith, "eu")]
    fails = []
    for s in (1, 2):                                           # (no bit equality: fused_pack changes the summation)
        for name, got, want in (("W", runs[s].w, plain[s][0]), ("H", runs[s].hs[0], plain[s][1])):
            _, msg = S.compare(f"phase calls against the plain handle, {name}{s}", got, want, bar)
            if msg:
                fails.append(msg)
    assert not fails, "\n".join(fails)


# ---- the stop rule: fires in iteration 2 on every rank, the rest of the run changes nothing --------------------------------------
@pytest.mark.parametrize("form", ["allreduce", "rsag"])
def test_stop_rule(form):
    m, n, k = 300, 330, 40
    v, w0, h0 = inputs(m, n, k, "eu")
    obj, w, h = [S.objective("eu", v, w0, h0)], w0, h0
    for _ in range(2):                                         # the float64 run from the same start
        w = S.ref_w("eu", v, w, h, 0.0)
        h = S.ref_h("eu", v, w, h, 0.0)
        obj.append(S.objective("eu", v, w, h))
    drop = obj[1] - obj[2]
    assert drop >= 1000 * S.OBJ_RTOL * obj[1], f"the yardstick's decrease {drop!r} of {obj[1]!r} makes the decision marginal"
    cuts = balanced(m, 3)
    stopped = X.run_sharded(v, w0, h0, "eu", 0.0, 0.0, cuts, form, steps=(4,), stop=(0, 0.0, 2 * drop))[4]
    free = X.run_sharded(v, w0, h0, "eu", 0.0, 0.0, cuts, form, steps=(2,))[2]
    assert stopped.form == form and free.form == form
    assert [st[:2] for st in stopped.states] == [(2, 1)] * 3, stopped.states
    assert X.ranks_differ(stopped) == []
    assert np.array_equal(stopped.w, free.w), f"W moved after the stop: {int(np.sum(stopped.w != free.w))} elements"
    for r in range(3):
        assert np.array_equal(stopped.hs[r], free.hs[r]), f"rank {r}: H moved after the stop: {int(np.sum(stopped.hs[r] != free.hs[r]))} elements"
    assert np.array_equal(stopped.objs[0][:2], free.objs[0][:2]) and len(stopped.objs[0]) == 3


# ---- determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,k,form", [("eu", 100, "chunks"), ("kl", 40, "allreduce")])
def test_two_sharded_runs_bit_identical(kind, k, form):
    m, n = 400, 1100
    v, w0, h0 = inputs(m, n, k, kind)
    kw = dict(ranges=CHUNKS[0][2]) if form == "chunks" else {}
    a = X.run_sharded(v, w0, h0, kind, 0.1, 0.0, balanced(m, 3), form, steps=(2,), **kw)
    b = X.run_sharded(v, w0, h0, kind, 0.1, 0.0, balanced(m, 3), form, steps=(2,), **kw)
    same_results(a, b, "two identical runs")
    assert np.array_equal(a[2].hs[2], b[2].hs[2])
