"""The sequence of collectives of every row-sharded solver (nmf_amd/dist.py), pinned call by call.

Two ranks that disagree about that sequence hang or pair the wrong reductions, and a redundant collective or two swapped
ones that commute numerically pass every comparison of results.  So: a communicator for a world of one that only notes
(kind, (dtype, first element, element count) of each buffer) -- a sum over one rank is the identity, the buffers are left
alone -- under the product's loops, with the numpy stand-in engine of tests/host_shard.py.  CPU, no process group."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from host_shard import ChunkedHostShard, HostShard, SlicedHostShard  # noqa: E402
from nmf_amd import dist as nd  # noqa: E402
from oracle import nmf_ref as R  # noqa: E402

M, N, K, ITERS, ROUNDS = 24, 16, 3, 3, 4
N32 = K * N + K * K + K            # HostShard's "f32" exchange buffer: [W^T V | W^T W | column sums]


class RecordingComm:
    rank, world = 0, 1
    stage = True

    def __init__(self, scatters=True, async_all_reduce=True):
        self.scatters, self.async_all_reduce = scatters, async_all_reduce
        self.log = []

    @staticmethod
    def _note(t):
        return str(t.dtype).replace("torch.", ""), int(t.storage_offset()), int(t.numel())

    def all_reduce(self, *tensors):
        self.log.append(("all_reduce",) + tuple(self._note(t) for t in tensors))

    def all_reduce_async(self, tensor):
        self.log.append(("all_reduce_async", self._note(tensor)))
        return None

    def reduce_scatter(self, tensor, elems):
        self.log.append(("reduce_scatter", self._note(tensor), elems))

    def all_gather(self, tensor, elems):
        self.log.append(("all_gather", self._note(tensor), elems))


def buf(first, count):
    return ("float64", first, count)           # (the stand-in keeps both exchange buffers in float64)


X32, OBJ, NORMS, TABLE = buf(0, N32), buf(0, 8), buf(1, 4), buf(8, 4 * ROUNDS)
CLOSING = [("all_reduce", OBJ)]


def inputs(svd):
    v = R.planted_matrix(M, N, K, seed=51, dtype=np.float64)
    if svd:
        return (v,) + tuple(R.svd_init(v, K, "zero"))
    rs = np.random.RandomState(52)
    return v, np.abs(rs.randn(M, K)), np.abs(rs.randn(K, N))


def check(res, ref, rtol_obj, rtol, atol):
    assert res.i == ref.i == ITERS - 1
    np.testing.assert_allclose(res.obj_history, ref.obj_history, rtol=rtol_obj)
    np.testing.assert_allclose(res.h, ref.h, rtol=rtol, atol=atol)
    np.testing.assert_allclose(res.w, ref.w, rtol=rtol, atol=atol)


MUR_KW = dict(min_iter=ITERS, max_iter=ITERS, lambda_w=0.05, lambda_h=0.1)
MUR_REF = {}


def mur_ref(loss):
    if loss not in MUR_REF:
        v, w0, h0 = inputs(False)
        MUR_REF[loss] = R.mur(v, K, w0=w0, h0=h0, distance_type=loss, **MUR_KW)
    return MUR_REF[loss]


PLAIN = [("all_reduce", X32, OBJ)]
CHUNKS_2 = [("all_reduce_async", buf(0, 8 * K)), ("all_reduce_async", buf(8 * K, N32 - 8 * K)), ("all_reduce", OBJ)]
RSAG = [("reduce_scatter", X32, N * K), ("all_reduce", buf(N * K, N32 - N * K), OBJ), ("all_gather", X32, N * K)]
MUR_CASES = {
    "plain": (HostShard, "eu", {}, {}, PLAIN),
    "plain_kl": (HostShard, "kl", {}, {}, PLAIN),
    "2_chunks": (ChunkedHostShard, "eu", {"NMFX_DIST_CHUNKS": "2"}, {}, CHUNKS_2),
    "chunks_kl_one_piece": (ChunkedHostShard, "kl", {"NMFX_DIST_CHUNKS": "2"}, {}, PLAIN),
    "chunks_shard_without_them": (HostShard, "eu", {"NMFX_DIST_CHUNKS": "2"}, {}, PLAIN),
    "chunks_comm_without_async": (ChunkedHostShard, "eu", {"NMFX_DIST_CHUNKS": "2"}, dict(async_all_reduce=False), PLAIN),
    "rsag": (SlicedHostShard, "eu", {"NMFX_DIST_EXCHANGE": "rsag"}, {}, RSAG),
    "rsag_wins_over_chunks": (SlicedHostShard, "eu", {"NMFX_DIST_EXCHANGE": "rsag", "NMFX_DIST_CHUNKS": "2"}, {}, RSAG),
    "rsag_kl_all_reduce": (SlicedHostShard, "kl", {"NMFX_DIST_EXCHANGE": "rsag"}, {}, PLAIN),
    "rsag_shard_without_it": (HostShard, "eu", {"NMFX_DIST_EXCHANGE": "rsag"}, {}, PLAIN),
    "rsag_comm_without_it": (SlicedHostShard, "eu", {"NMFX_DIST_EXCHANGE": "rsag"}, dict(scatters=False), PLAIN),
}


@pytest.mark.parametrize("name", list(MUR_CASES))
def test_mur_collective_sequence(name, monkeypatch):
    cls, loss, env, caps, per_iteration = MUR_CASES[name]
    for key in ("NMFX_DIST_CHUNKS", "NMFX_DIST_EXCHANGE", "NMFX_DIST_GRAPH"):
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    v, w0, h0 = inputs(False)
    comm = RecordingComm(**caps)
    res = nd.mur_sharded(cls(v, K, w0, h0), comm, distance_type=loss, batch=2, **MUR_KW)
    assert comm.log == per_iteration * ITERS + CLOSING
    check(res, mur_ref(loss), 1e-10, 1e-9, 1e-300)


AO_KW = dict(reg_w=(0.1, "l1n"), reg_h=(0.05, "l1n"), min_iter=ITERS, max_iter=ITERS, admm_iter=ROUNDS)
ADMM_KW = dict(rho=2, reg_w=(0.05, "l1n"), reg_h=(0.3, "l2n"), min_iter=ITERS, max_iter=ITERS)
ANLS_KW = dict(lambda_w=0.1, lambda_h=0.05, min_iter=ITERS, max_iter=ITERS)
SOLVER_CASES = {
    "ao_admm_fused": (nd.aoadmm_sharded, R.ao_admm, AO_KW, {}, [("all_reduce", X32, OBJ), ("all_reduce", TABLE)]),
    "ao_admm_unfused": (nd.aoadmm_sharded, R.ao_admm, AO_KW, dict(fused=False),
                        [("all_reduce", X32, OBJ)] + [("all_reduce", NORMS)] * ROUNDS),
    "ao_admm_kl": (nd.aoadmm_sharded, R.ao_admm, dict(AO_KW, distance_type="kl"), {},
                   [("all_reduce", X32, OBJ)] + [("all_reduce", X32)] * (ROUNDS - 1) + [("all_reduce", NORMS)] * ROUNDS),
    "admm_eu": (nd.admm_sharded, R.admm, dict(ADMM_KW, distance_type="eu"), {}, [("all_reduce", X32, OBJ)]),
    "admm_kl": (nd.admm_sharded, R.admm, dict(ADMM_KW, distance_type="kl"), {}, [("all_reduce", X32, OBJ)]),
    "anls": (nd.anls_sharded, R.anls, ANLS_KW, {}, [("all_reduce", OBJ), ("all_reduce", X32)]),
}


@pytest.mark.parametrize("name", list(SOLVER_CASES))
def test_solver_collective_sequence(name):
    run, oracle, kw, extra, per_iteration = SOLVER_CASES[name]
    v, w0, h0 = inputs(True)
    comm = RecordingComm()
    res = run(HostShard(v, K, w0, h0), comm, batch=2, **kw, **extra)
    assert comm.log == per_iteration * ITERS + CLOSING
    check(res, oracle(v, K, w0=w0, h0=h0, **kw), 1e-8, 1e-6, 1e-9)


@pytest.mark.parametrize("run", [nd.mur_sharded, nd.aoadmm_sharded, nd.admm_sharded, nd.anls_sharded])
def test_no_iterations_raises_before_any_collective(run):
    """max_iter <= 0 ends as the reference's loops do, on every rank, with no rank left inside a collective."""
    v, w0, h0 = inputs(False)
    comm = RecordingComm()
    with pytest.raises(UnboundLocalError):
        run(HostShard(v, K, w0, h0), comm, max_iter=0)
    assert comm.log == []


def test_only_rank_zero_prints(capsys, monkeypatch):
    """The `[i]: objective` lines and the convergence message come from rank 0 alone; history and stop index do not depend on it."""
    from nmf_amd import utils
    monkeypatch.setattr(utils, "QUIET", False)
    v, w0, h0 = inputs(False)
    kw = dict(distance_type="eu", min_iter=1, max_iter=9, tol1=1e-9, tol2=1e30, batch=2)     # rule 2 at the first tested index
    out = []
    for rank in (0, 1):
        comm = RecordingComm()
        comm.rank = rank
        res = nd.mur_sharded(HostShard(v, K, w0, h0), comm, **kw)
        out.append((res, capsys.readouterr().out.splitlines()))
    (first, said), (second, silence) = out
    assert first.i == second.i == 2 and len(first.obj_history) == 4
    np.testing.assert_array_equal(first.obj_history, second.obj_history)
    assert [line.split(":")[0] for line in said] == ["[0]", "[1]", "[2]", "Algorithm converged (2)."] and silence == []
