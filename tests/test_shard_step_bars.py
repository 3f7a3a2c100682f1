"""CPU proof of the lock-step shard driver (tests/shard_step.py) and of the checks the GPU test feeds with it
(tests/test_gpu_shard_step.py), on the numpy stand-ins of tests/host_shard.py:

  * N stand-in shards driven in every exchange form agree with the float64 step on the whole V;
  * for a world of one the driver issues the phase calls nmf_amd.dist.run_iterations / finish issue, call by call;
  * each planted fault -- a sum that leaves a shard out, a shifted slice, stale columns, a lost row, a dropped objective
    partial, a Gram part missing on one rank -- is rejected, and the message names its tile or its objective entry;
  * the digit codec of the objective tail round-trips bit for bit."""
import os
import re
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mur_step as S  # noqa: E402
import shard_step as X  # noqa: E402
from host_shard import ChunkedHostShard, HostShard, SlicedHostShard  # noqa: E402
from nmf_amd import dist as nd  # noqa: E402
from oracle import nmf_ref as R  # noqa: E402

BAR = 1e-11


def host_nodes(cls, per_rank=None):
    """make_engine for run_sharded: stand-in `cls` on every rank, `per_rank[rank]` where given."""
    def make(rank, v_local, k, w_local, h):
        c = (per_rank or {}).get(rank, cls)
        shard = c(v_local, k, w_local, h)
        shard.rank = rank
        return X.HostNode(shard, transposed=issubclass(c, ChunkedHostShard))
    return make


# ---- agreement with one handle ------------------------------------------------------------------------------------------------
M, N, K = 41, 60, 4
CUTS = {1: [0, 41], 2: [0, 1, 41], 3: [0, 1, 17, 41], 5: [0, 1, 9, 10, 30, 41]}
RANGES = [(0, 24), (24, 60)]
COMBOS = [(HostShard, "allreduce", "eu"), (HostShard, "allreduce", "kl"), (ChunkedHostShard, "allreduce", "eu"),
          (ChunkedHostShard, "chunks", "eu"), (SlicedHostShard, "allreduce", "eu"), (SlicedHostShard, "chunks", "eu"),
          (SlicedHostShard, "rsag", "eu")]


def agree(runs, kind, v, w0, h0, lw, lh):
    X.check(kind, v, w0, h0, runs, lw, lh, BAR, obj_rtol=BAR)
    assert X.ranks_differ(runs[1]) == [] and X.ranks_differ(runs[2]) == []
    vv = np.asarray(v, dtype=np.float64)
    w, h = w0, h0
    for s in (1, 2):                              # the whole-V float64 step, chained from the start
        w = R.mur_w_step(kind, vv, w, h, w @ h, lw)
        h = R.mur_h_step(kind, vv, w, h, w @ h, lh)
        np.testing.assert_allclose(runs[s].w, w, rtol=1e-12, atol=0)
        np.testing.assert_allclose(runs[s].hs[0], h, rtol=1e-12, atol=0)


@pytest.mark.parametrize("world", [1, 2, 3, 5])
@pytest.mark.parametrize("cls,form,kind", COMBOS, ids=[f"{c.__name__}-{f}-{kd}" for c, f, kd in COMBOS])
def test_stand_in_shards_agree_with_one_handle(cls, form, kind, world):
    v, w0, h0 = S.make_inputs(M, N, K, seed=3, edges=True, dead=kind == "eu", zeros=True)
    lw, lh = (0.1, 0.0) if kind == "eu" else (0.0, 0.2)
    runs = X.run_sharded(v, w0, h0, kind, lw, lh, CUTS[world], form, make_engine=host_nodes(cls), ranges=RANGES, snapshot=True)
    assert runs[1].form == form and not runs[1].merged
    agree(runs, kind, v, w0, h0, lw, lh)
    X.check_partials(kind, v, runs[1], runs[1].w, h0, BAR)          # the buffers after phase A, in the stand-in's layout
    for run in runs.values():
        X.check_objective_sums(run)


def test_sparse_world_and_missing_slice_form():
    v, w0, h0 = S.make_inputs(M, N, K, seed=4, edges=True, dead=True, zeros=True)
    runs = X.run_sharded(v, w0, h0, "eu", 0.0, 0.1, CUTS[3], "allreduce", ranks=[0, 3, 4], world=6, make_engine=host_nodes(HostShard))
    assert runs[2].ranks == (0, 3, 4) and runs[2].world == 6
    agree(runs, "eu", v, w0, h0, 0.0, 0.1)
    # n = 60 is no multiple of a world of 7: the stand-in has no slices, the driver says so and takes the all-reduce
    cuts7 = [0, 1, 9, 10, 17, 30, 35, 41]
    runs = X.run_sharded(v, w0, h0, "eu", 0.0, 0.1, cuts7, "rsag", make_engine=host_nodes(SlicedHostShard))
    assert runs[1].requested == "rsag" and runs[1].form == "allreduce"
    agree(runs, "eu", v, w0, h0, 0.0, 0.1)
    with pytest.raises(ValueError, match="every rank"):
        X.run_sharded(v, w0, h0, "eu", 0.0, 0.1, CUTS[3], "rsag", ranks=[0, 3, 4], world=6, make_engine=host_nodes(SlicedHostShard))


# ---- the sequence of phase calls, world of one ---------------------------------------------------------------------------------
PHASES = ("mur_phase_a", "mur_phase_a_head", "mur_phase_a_cols", "mur_phase_b", "mur_phase_b_slice", "mur_phase_b_rest",
          "mur_finish_a", "mur_finish_b")


def recording(cls):
    class Recorded(cls):
        def __init__(self, *args):
            super().__init__(*args)
            self.calls = []

    def wrap(name):
        def method(self, *args):
            self.calls.append((name,) + tuple(args))
            return getattr(cls, name)(self, *args)
        return method

    for name in PHASES:
        if hasattr(cls, name):
            setattr(Recorded, name, wrap(name))
    return Recorded


class QuietComm:
    """A communicator for a world of one that leaves the buffers alone (a sum over one rank is the identity)."""
    rank, world, stage, scatters, async_all_reduce = 0, 1, True, True, True

    def all_reduce(self, *tensors):
        pass

    def all_reduce_async(self, tensor):
        return None

    def reduce_scatter(self, tensor, elems):
        pass

    def all_gather(self, tensor, elems):
        pass


@pytest.mark.parametrize("cls,form,kind", COMBOS, ids=[f"{c.__name__}-{f}-{kd}" for c, f, kd in COMBOS])
def test_driver_issues_the_calls_of_run_iterations(cls, form, kind, monkeypatch):
    for key in ("NMFX_DIST_CHUNKS", "NMFX_DIST_EXCHANGE", "NMFX_DIST_GRAPH"):
        monkeypatch.delenv(key, raising=False)
    if form == "rsag":
        monkeypatch.setenv("NMFX_DIST_EXCHANGE", "rsag")
    v, w0, h0 = S.make_inputs(M, N, K, seed=5, edges=True, dead=kind == "eu", zeros=True)
    code, lw, lh, iters = (0 if kind == "eu" else 1), 0.05, 0.1, 2
    rec = recording(cls)
    # the product's loop
    ref = rec(v, K, w0, h0)
    ranges = ref.chunk_ranges(code, 2) if form == "chunks" else None
    nd.run_iterations(ref, QuietComm(), code, lw, lh, S.NEVER, 0.0, 0.0, 0, iters, chunks=2 if form == "chunks" else 1)
    nd.finish(ref, QuietComm(), code, S.NEVER, 0.0, 0.0, iters)
    # the driver
    made = []

    def make(rank, v_local, k, w_local, h):
        made.append(rec(v_local, k, w_local, h))
        return X.HostNode(made[-1], transposed=issubclass(cls, ChunkedHostShard))

    runs = X.run_sharded(v, w0, h0, kind, lw, lh, [0, M], form, steps=(iters,), make_engine=make,
                         ranges=[(c0, c1) for c0, c1, _, _ in ranges] if ranges else None)
    assert runs[iters].form == form
    assert made[0].calls == ref.calls
    assert len(ref.calls) >= 2 * iters + 2
    np.testing.assert_array_equal(runs[iters].w, ref.w)
    np.testing.assert_array_equal(runs[iters].hs[0], ref.h)
    np.testing.assert_array_equal(runs[iters].objs[0], ref.objectives(0, iters + 1))


# ---- planted faults -------------------------------------------------------------------------------------------------------------
FM, FN, FK = 300, 192, 4                       # three 128-row tiles, three 64-column blocks
FCUTS = [0, 100, 229, 300]
FRANGES = [(0, 64), (64, 128), (128, 192)]
FLW, FLH = 0.1, 0.0


def fault_inputs():
    return S.make_inputs(FM, FN, FK, seed=8, edges=True, dead=True, zeros=True)


def run_fault(cls, form, per_rank=None, collective=None):
    v, w0, h0 = fault_inputs()
    runs = X.run_sharded(v, w0, h0, "eu", FLW, FLH, FCUTS, form, make_engine=host_nodes(cls, per_rank), ranges=FRANGES,
                         collective=collective)
    return (v, w0, h0), runs


def rejected(inp, runs, rank_index=0):
    with pytest.raises(AssertionError) as e:
        X.check("eu", *inp, runs, FLW, FLH, BAR, rank_index=rank_index, obj_rtol=BAR)
    return str(e.value)


def test_the_unfaulted_runs_pass():
    for cls, form in ((HostShard, "allreduce"), (ChunkedHostShard, "chunks"), (SlicedHostShard, "rsag")):
        inp, runs = run_fault(cls, form)
        X.check("eu", *inp, runs, FLW, FLH, BAR, obj_rtol=BAR)
        assert X.ranks_differ(runs[2]) == []


class ChunkWithoutRankOne(X.HostCollective):
    """Rank 1's contribution to the second column chunk is left out of the sum."""

    def all_reduce(self, bufs, a, b, what):
        if what == "x32" and a == 64 * FK:
            acc = self.total([p for i, p in enumerate(self._parts(bufs, a, b)) if i != 1])
            for t in bufs:
                self._put(t, a, acc)
            return
        super().all_reduce(bufs, a, b, what)


def test_fault_chunk_contribution_left_out():
    inp, runs = run_fault(ChunkedHostShard, "chunks", collective=ChunkWithoutRankOne())
    msg = rejected(inp, runs)
    assert re.search(r"^H1: .*128x64 tile \(0, 1\)", msg, re.M), msg
    assert not re.search(r"^W1: ", msg, re.M), msg


class ShiftedSlice(SlicedHostShard):
    """Updates the 64-column block behind its own."""

    def mur_phase_b_slice(self, kind, lambda_h, min_iter, tol1, tol2, j, c0, c1):
        super().mur_phase_b_slice(kind, lambda_h, min_iter, tol1, tol2, j, c0 + 64, c1 + 64)


def test_fault_slice_shifted_by_one_block():
    inp, runs = run_fault(SlicedHostShard, "rsag", per_rank={1: ShiftedSlice})
    msg = rejected(inp, runs)
    assert re.search(r"^H1: .*128x64 tile \(0, 1\)", msg, re.M), msg
    assert X.ranks_differ(runs[1]) != []


class StaleLastBlock(SlicedHostShard):
    """`rest` skips the last foreign 64-column block: its columns keep the previous iterate."""

    def mur_phase_b_rest(self, kind, c0, c1):
        before = self.h.copy()
        super().mur_phase_b_rest(kind, c0, c1)
        foreign = [b for b in range(self.h.shape[1] // 64) if not c0 <= 64 * b < c1]
        self.h[:, 64 * foreign[-1]:64 * foreign[-1] + 64] = before[:, 64 * foreign[-1]:64 * foreign[-1] + 64]


def test_fault_rest_leaves_stale_columns():
    inp, runs = run_fault(StaleLastBlock, "rsag")
    msg = rejected(inp, runs)
    assert re.search(r"^H1: .*128x64 tile \(0, 2\)", msg, re.M), msg          # rank 0's last foreign block
    assert X.ranks_differ(runs[1]) != []


class LastRowLost(HostShard):
    """The last row of the shard never reached the engine."""

    def __init__(self, v_local, k, w0_local, h0):
        super().__init__(v_local, k, w0_local, h0)
        self.v[-1, :] = 0


def test_fault_last_row_of_a_shard_not_uploaded():
    inp, runs = run_fault(HostShard, "allreduce", per_rank={1: LastRowLost})
    msg = rejected(inp, runs)
    assert re.search(r"^W1: .*\(row, col\) = \(228, \d+\), 128x64 tile \(1, 0\)", msg, re.M), msg
    assert re.search(r"^W1: .* [1-4] of 1200 elements over the bar", msg, re.M), msg     # that row alone (k = 4, one dead component)


class ObjectiveWithoutRankOne(X.HostCollective):
    def all_reduce(self, bufs, a, b, what):
        if what == "x64":
            acc = self.total([p for i, p in enumerate(self._parts(bufs, a, b)) if i != 1])
            for t in bufs:
                self._put(t, a, acc)
            return
        super().all_reduce(bufs, a, b, what)


def test_fault_objective_partial_dropped():
    inp, runs = run_fault(HostShard, "allreduce", collective=ObjectiveWithoutRankOne())
    msg = rejected(inp, runs)
    assert re.search(r"^obj\[0\] of the 1-step run", msg, re.M) and re.search(r"^obj\[2\] of the 2-step run", msg, re.M), msg
    assert not re.search(r"^[WH][12]: ", msg, re.M), msg


class GramWithoutRankZeroOnRankOne(X.HostCollective):
    """Rank 1 receives a W^T W that lacks rank 0's part."""

    def all_reduce(self, bufs, a, b, what):
        parts = self._parts(bufs, a, b) if what == "x32" else None
        super().all_reduce(bufs, a, b, what)
        if parts is not None:
            g0, g1 = FK * FN - a, FK * FN + FK * FK - a
            self._put(bufs[1], a + g0, self.total([p[g0:g1] for p in parts[1:]]))


def test_fault_gram_part_missing_on_one_rank():
    inp, runs = run_fault(HostShard, "allreduce", collective=GramWithoutRankZeroOnRankOne())
    msg = rejected(inp, runs, rank_index=1)
    assert re.search(r"^rank 1: H1: .*128x64 tile", msg, re.M), msg
    assert "W2" in rejected(inp, runs)             # rank 0's H is right; the rows of rank 1 in W_2 come from its own, wrong H_1
    differ = X.ranks_differ(runs[1])
    assert differ and "H of rank 1" in differ[0]


# ---- the digit codec ------------------------------------------------------------------------------------------------------------
def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


WITH_FFFF = struct.unpack("<d", struct.pack("<Q", 0x3FF0FFFF0000FFFF))[0]


@pytest.mark.parametrize("x", [0.0, 5e-324, 1.0, 1e300, WITH_FFFF, 123456.789e-7])
def test_digits_round_trip(x):
    d = X.encode_digits(x)
    assert d.dtype == np.float32 and d.shape == (4,)
    assert bits_of(X.decode_digits(d)) == bits_of(x)
    assert [int(t) for t in d] == [(bits_of(x) >> (16 * i)) & 0xFFFF for i in range(4)]


def test_digits_survive_a_sum_over_64_slots():
    owner, x = 37, WITH_FFFF * 1e-200
    tails = [np.zeros(4 * X.XTAIL_RANKS, dtype=np.float32) for _ in range(X.XTAIL_RANKS)]
    tails[owner][4 * owner:4 * owner + 4] = X.encode_digits(x)
    total = X.HostCollective().total(tails)
    assert total.dtype == np.float32
    assert bits_of(X.decode_digits(total[4 * owner:4 * owner + 4])) == bits_of(x)
    assert not np.any(np.delete(total, range(4 * owner, 4 * owner + 4)))
    with pytest.raises(ValueError):
        X.decode_digits(np.array([0.5, 0, 0, 0], dtype=np.float32))
    with pytest.raises(ValueError):
        X.decode_digits(np.array([65535.0 + 3.0, 0, 0, 0], dtype=np.float32))
