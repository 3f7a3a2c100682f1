"""Digest of what the row-sharded drivers (nmf_amd/dist.py) return, print and exchange: one SHA-256 per case and rank.

    python tools/dist_digest.py > profiles/dist_digest_parent.txt                                  # host part: two gloo ranks, CPU
    python tools/dist_digest.py --device --backend nccl   >  profiles/dist_digest_device_parent.txt      # device part, world of one
    python tools/dist_digest.py --device --backend native >> profiles/dist_digest_device_parent.txt

Every line hashes w, h, i, obj_history, the experiment tuple, the lines printed and the log of collectives of one run on one
rank.  The log is the ordered list of (kind, dtype, first element, element count) of every call of the communicator, noted by a
TorchComm subclass that then calls super() (calls that TorchComm makes on itself -- the all-reduce that stands in for a
reduce-scatter on gloo -- are noted like any other: the class is the same text on both sides of a comparison).  The device part
notes, in the same list, every Engine call that queues device work or a collective (mur_*, *_phase_*, comm_*, objective_partial,
set_l2n_operator, anls_set_distance) with its scalar arguments: the collectives of the native path are Engine.comm_all_reduce
calls, and the order of phase calls and collectives is what a capture or a batch replays.  Log records are not hashed.

The script imports nmf_amd.dist's public surface (row_range, TorchComm, DeviceShard, NativeShard, NativeComm, the four *_sharded
functions, factorize) and the HostShard family of its own checkout's tests/host_shard.py only, so it runs unmodified in a checkout
of another commit: two commits that print the same lines drive the engine and the communicator identically.

Host part: the cases of tests/test_dist_gloo.py, all in one pair of rank processes.  Device part: DeviceShard over RCCL through
torch.distributed ("nccl") or NativeShard / NativeComm ("native"), world of one, at the shapes of tests/test_gpu_dist.py."""
import argparse
import contextlib
import hashlib
import io
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

# ---- host cases: tests/test_dist_gloo.py ----------------------------------------------------------------------------
EU_LAMBDA = dict(distance_type="eu", min_iter=12, max_iter=12, lambda_w=0.05, lambda_h=0.1)
EU_CONVERGE = dict(distance_type="eu", min_iter=5, max_iter=400, tol1=1e-9, tol2=2e-4)
KL = dict(distance_type="kl", min_iter=9, max_iter=9, lambda_w=0.0, lambda_h=0.02)
AO_EARLY = dict(reg_w=(0, "nn"), reg_h=(0, "nn"), min_iter=2, max_iter=60, admm_iter=10, tol1=1e-3, tol2=1e-2)
HOST_CASES = [
    ("mur eu_lambda", dict(solver="mur", m=150, n=90, k=5, seed=3, batch=7, kw=EU_LAMBDA)),
    ("mur eu_converge", dict(solver="mur", m=131, n=77, k=4, seed=4, batch=16, kw=EU_CONVERGE)),
    ("mur kl", dict(solver="mur", m=96, n=64, k=3, seed=5, batch=5, kw=KL)),
    ("mur eu_lambda 3 chunks", dict(solver="mur", m=150, n=90, k=5, seed=3, batch=7, chunks=3, kw=EU_LAMBDA)),
    ("mur eu_converge 2 chunks", dict(solver="mur", m=131, n=77, k=4, seed=4, batch=16, chunks=2, kw=EU_CONVERGE)),
    ("mur eu_lambda rsag", dict(solver="mur", m=150, n=90, k=5, seed=3, batch=7, exchange="rsag", kw=EU_LAMBDA)),
    ("mur eu_converge rsag", dict(solver="mur", m=131, n=80, k=4, seed=4, batch=16, exchange="rsag", kw=EU_CONVERGE)),
    ("mur kl rsag falls back", dict(solver="mur", m=96, n=64, k=3, seed=5, batch=5, exchange="rsag", kw=KL)),
    ("mur eu odd n rsag falls back", dict(solver="mur", m=150, n=91, k=5, seed=3, batch=7, exchange="rsag", kw=EU_LAMBDA)),
    ("ao_admm l1n fused", dict(solver="ao_admm", m=120, n=84, k=6, seed=11, batch=3, svd=True,
                               kw=dict(reg_w=(0.1, "l1n"), reg_h=(0.05, "l1n"), min_iter=6, max_iter=6, admm_iter=10))),
    ("ao_admm early exit fused", dict(solver="ao_admm", m=96, n=70, k=5, seed=12, batch=2, svd=True, uniform=True, kw=AO_EARLY)),
    ("anls", dict(solver="anls", m=60, n=44, k=4, seed=13, batch=3, svd=True,
                  kw=dict(lambda_w=0.1, lambda_h=0.05, min_iter=3, max_iter=40, tol1=1e-3, tol2=1e-3))),
    ("ao_admm round by round", dict(solver="ao_admm", m=96, n=70, k=5, seed=12, batch=2, svd=True, uniform=True,
                                    extra=dict(fused=False), kw=AO_EARLY)),
    ("admm eu l1n l2n", dict(solver="admm", m=110, n=80, k=5, seed=21, batch=4, svd=True,
                             kw=dict(rho=2, distance_type="eu", reg_w=(0.05, "l1n"), reg_h=(0.3, "l2n"), min_iter=8, max_iter=8))),
    ("admm kl", dict(solver="admm", m=90, n=66, k=4, seed=22, batch=3, svd=True,
                     kw=dict(rho=1, distance_type="kl", reg_w=(0, "nn"), reg_h=(0, "nn"), min_iter=6, max_iter=6))),
    ("admm l1inf on h", dict(solver="admm", m=90, n=66, k=4, seed=23, batch=3, svd=True,
                             kw=dict(rho=1, distance_type="eu", reg_w=(0.05, "l1n"), reg_h=(0.05, "l1inf"), min_iter=3, max_iter=3))),
    ("ao_admm kl", dict(solver="ao_admm", m=90, n=66, k=4, seed=24, batch=2, svd=True,
                        kw=dict(distance_type="kl", reg_w=(0.02, "l1n"), reg_h=(0, "nn"), min_iter=4, max_iter=4, admm_iter=6))),
    ("ao_admm kl long inner", dict(solver="ao_admm", m=96, n=70, k=5, seed=12, batch=2, svd=True, uniform=True,
                                   kw=dict(distance_type="kl", reg_w=(0, "nn"), reg_h=(0, "nn"), min_iter=2, max_iter=12, admm_iter=25,
                                           tol1=1e-3, tol2=1e-1))),
    ("factorize mur eu", dict(api=True, solver="mur", m=101, n=63, k=4, seed=31,
                              kw=dict(distance_type="eu", min_iter=9, max_iter=9, lambda_w=0.02))),
    ("factorize mur default kl", dict(api=True, solver="mur", m=64, n=48, k=3, seed=32, kw=dict(min_iter=7, max_iter=7))),
    ("factorize ao_admm", dict(api=True, solver="ao_admm", m=90, n=70, k=4, seed=33,
                               kw=dict(reg_w=(0.05, "l1n"), reg_h=(0.05, "l1n"), min_iter=4, max_iter=4))),
    ("factorize admm", dict(api=True, solver="admm", m=90, n=70, k=4, seed=34, kw=dict(reg_h=(0.2, "l2n"), min_iter=5, max_iter=5))),
    ("factorize anls kl", dict(api=True, solver="anls", m=50, n=40, k=3, seed=35,
                               kw=dict(distance_type="kl", min_iter=3, max_iter=3, lambda_h=0.05))),
    ("factorize ao_admm kl", dict(api=True, solver="ao_admm", m=70, n=50, k=3, seed=36,
                                  kw=dict(distance_type="kl", reg_w=(0, "nn"), reg_h=(0.02, "l1n"), min_iter=3, max_iter=3, admm_iter=5))),
]

# ---- device cases: the shapes of tests/test_gpu_dist.py, max_iter <= 14 -----------------------------------------------
MUR_KW = dict(distance_type="eu", min_iter=14, max_iter=14, lambda_w=0.01, lambda_h=0.02)
MUR_STOP = dict(distance_type="eu", min_iter=3, max_iter=14, tol1=1e-5, tol2=1e30)     # rule 2 fires at the first tested index
AO_KW = dict(reg_w=(0.1, "l1n"), reg_h=(0.05, "l1n"), min_iter=8, max_iter=8, admm_iter=10)
AO_KL_KW = dict(distance_type="kl", reg_w=(0.02, "l1n"), reg_h=(0, "nn"), min_iter=4, max_iter=4, admm_iter=6)
ADMM_KW = dict(rho=1.0, distance_type="eu", reg_w=(0.05, "l1n"), reg_h=(0.2, "l2n"), min_iter=6, max_iter=6)
ADMM_KL_KW = dict(rho=1.0, distance_type="kl", reg_w=(0.05, "l1n"), reg_h=(0.05, "l1n"), min_iter=6, max_iter=6)
ANLS_KW = dict(lambda_w=0.1, lambda_h=0.05, min_iter=3, max_iter=12, tol1=1e-3, tol2=1e-3)
DEVICE_CASES = [(f"mur eu k={k}", dict(solver="mur", k=k, batch=5, kw=MUR_KW)) for k in (12, 40, 100, 160)] + [
    ("mur kl k=12", dict(solver="mur", k=12, batch=5, kw=dict(MUR_KW, distance_type="kl"))),
    ("mur eu k=40 stops", dict(solver="mur", k=40, batch=5, kw=MUR_STOP)),
    ("mur eu k=40 2 chunks", dict(solver="mur", k=40, batch=5, wide=True, chunks=2, kw=MUR_KW)),
    ("mur eu k=100 2 chunks", dict(solver="mur", k=100, batch=5, wide=True, chunks=2, kw=MUR_KW)),
    ("mur eu k=12 rsag falls back", dict(solver="mur", k=12, batch=5, exchange="rsag", kw=MUR_KW)),
    ("mur eu k=40 rsag", dict(solver="mur", k=40, batch=5, exchange="rsag", kw=MUR_KW)),
    ("mur eu k=100 rsag", dict(solver="mur", k=100, batch=5, exchange="rsag", kw=MUR_KW)),
    ("mur eu k=12 graph", dict(solver="mur", k=12, batch=7, extra=dict(graph=True), kw=MUR_KW)),
    ("mur eu k=40 graph", dict(solver="mur", k=40, batch=7, extra=dict(graph=True), kw=MUR_KW)),
    ("mur eu k=40 graph stops", dict(solver="mur", k=40, batch=7, extra=dict(graph=True), kw=MUR_STOP)),
    ("mur eu k=40 rsag graph", dict(solver="mur", k=40, batch=7, exchange="rsag", extra=dict(graph=True), kw=MUR_KW)),
    ("mur kl k=12 graph", dict(solver="mur", k=12, batch=7, extra=dict(graph=True), kw=dict(MUR_KW, distance_type="kl"))),
    ("ao_admm eu fused", dict(solver="ao_admm", m=520, n=300, k=12, seed=31, batch=16, kw=AO_KW)),
    ("ao_admm eu unfused", dict(solver="ao_admm", m=520, n=300, k=12, seed=31, batch=16, extra=dict(fused=False), kw=AO_KW)),
    ("ao_admm eu k=40", dict(solver="ao_admm", m=520, n=300, k=40, seed=31, batch=3, kw=AO_KW)),
    ("ao_admm kl", dict(solver="ao_admm", m=320, n=200, k=8, seed=35, batch=16, kw=AO_KL_KW)),
    ("admm eu", dict(solver="admm", m=520, n=300, k=12, seed=33, batch=3, kw=ADMM_KW)),
    ("admm kl", dict(solver="admm", m=520, n=300, k=12, seed=33, batch=3, kw=ADMM_KL_KW)),
    ("anls", dict(solver="anls", m=200, n=150, k=6, seed=31, batch=3, kw=ANLS_KW)),
]


def inputs(case):
    from oracle import nmf_ref as R
    m, n, k = case["m"], case["n"], case["k"]
    if case.get("uniform"):
        v = np.random.RandomState(case["seed"]).rand(m, n)
    else:
        v = R.planted_matrix(m, n, k, seed=case["seed"], dtype=np.float64)
    if case.get("svd"):
        w0, h0 = R.svd_init(v, k, "zero")
    else:
        rs = np.random.RandomState(case["seed"] + 1)
        w0, h0 = np.abs(rs.randn(m, k)), np.abs(rs.randn(k, n))
    return v, w0, h0


def device_inputs(case):
    from oracle import nmf_ref as R
    k = case["k"]
    if case["solver"] != "mur":
        v = R.planted_matrix(case["m"], case["n"], k, seed=case["seed"], dtype=np.float32)
        return (v,) + tuple(R.svd_init(v.astype(np.float64), k, "zero"))
    m, n, rank, seed = (520, 1400, min(k, 32), 23) if case.get("wide") else (700, 330, k, 21)
    v = R.planted_matrix(m, n, rank, seed=seed, dtype=np.float32)
    rs = np.random.RandomState(seed + 1)
    return v, np.abs(rs.randn(m, k)), np.abs(rs.randn(k, n))


def note_of(t):
    """(dtype, first element, element count) of a torch tensor or of an ExRef (which = 0: f32, 1: f64)."""
    if hasattr(t, "which"):
        return ("f64" if t.which else "f32", int(t.first), int(t.count))
    return (str(t.dtype), int(t.storage_offset()), int(t.numel()))


def recording_comm(nd, log):
    class RecordingComm(nd.TorchComm):
        def all_reduce(self, *tensors):
            log.append(("all_reduce",) + tuple(note_of(t) for t in tensors))
            return super().all_reduce(*tensors)

        def all_reduce_async(self, tensor):
            log.append(("all_reduce_async", note_of(tensor)))
            return super().all_reduce_async(tensor)

        def reduce_scatter(self, tensor, elems):
            log.append(("reduce_scatter", note_of(tensor), int(elems)))
            return super().reduce_scatter(tensor, elems)

        def all_gather(self, tensor, elems):
            log.append(("all_gather", note_of(tensor), int(elems)))
            return super().all_gather(tensor, elems)
    return RecordingComm


DEVICE_WORK = ("mur_", "comm_", "objective_partial", "set_l2n_operator", "anls_set_distance", "shift_iteration_base", "reserve_objectives")


def record_engine_calls(log):
    """Wrap every Engine method that queues device work or a collective: its name and scalar arguments go to `log`."""
    from nmf_amd.engine import Engine

    def arg_note(a):
        if isinstance(a, np.ndarray):
            return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
        return repr(a) if isinstance(a, (bool, int, float, str, type(None))) else type(a).__name__

    def wrap(name, fn):
        def noted(self, *args, **kw):
            log.append((name,) + tuple(arg_note(a) for a in args) + tuple(sorted((key, arg_note(val)) for key, val in kw.items())))
            return fn(self, *args, **kw)
        return noted
    for name, fn in list(vars(Engine).items()):
        if callable(fn) and not name.startswith("_") and not isinstance(fn, (staticmethod, classmethod)) and \
                ("_phase_" in name or name.startswith(DEVICE_WORK)) and name not in ("comm_unique_id", "comm_info", "comm_get_exchange",
                                                                                      "comm_graph_replays", "mur_chunk_info", "mur_slice_info"):
            setattr(Engine, name, wrap(name, fn))


def as_bytes(v):
    if isinstance(v, (np.ndarray, list)):
        return np.asarray(v, dtype=None if isinstance(v, np.ndarray) else np.float64).tobytes()
    return repr(v).encode()


def digest(run, log):
    """One run with its prints caught; everything observable hashed.  An exception is hashed as its class and message."""
    del log[:]
    printed = io.StringIO()
    try:
        with contextlib.redirect_stdout(printed):
            res = run()
        parts = [as_bytes(np.asarray(res.w)), as_bytes(np.asarray(res.h)), as_bytes(int(res.i)), as_bytes(list(res.obj_history)),
                 repr(tuple(res.experiment) if res.experiment is not None else None).encode()]
        note = f"i={res.i} obj[-1]={res.obj_history[-1]!r}"
    except Exception as e:  # noqa: BLE001
        parts, note = [type(e).__name__.encode(), str(e).encode()], f"{type(e).__name__}: {e}"
    text = printed.getvalue()
    parts += [text.encode(), repr(log).encode()]
    sha = hashlib.sha256()
    for p in parts:
        sha.update(len(p).to_bytes(8, "little") + p)
    return sha.hexdigest(), f"{note} lines={text.count(chr(10))} calls={len(log)}"


def set_exchange_env(case):
    for key, name in (("chunks", "NMFX_DIST_CHUNKS"), ("exchange", "NMFX_DIST_EXCHANGE")):
        if case.get(key):
            os.environ[name] = str(case[key])
        else:
            os.environ.pop(name, None)


def host_worker(rank, world, rdzv, outdir):
    for key in ("NMF_AMD_QUIET", "NMFX_DIST_GRAPH", "NMFX_DIST_NATIVE", "NMFX_DIST_MERGE"):
        os.environ.pop(key, None)
    os.environ["NMFX_DIST_INIT_METHOD"] = rdzv
    os.environ["RANK"], os.environ["WORLD_SIZE"], os.environ["LOCAL_RANK"] = str(rank), str(world), str(rank)
    import torch.distributed as tdist
    tdist.init_process_group("gloo", init_method=rdzv, rank=rank, world_size=world)
    from host_shard import ChunkedHostShard, HostShard, SlicedHostShard
    from nmf_amd import dist as nd
    log = []
    nd.TorchComm = recording_comm(nd, log)               # (factorize makes its own communicator: it finds this class)
    solvers = {"mur": nd.mur_sharded, "ao_admm": nd.aoadmm_sharded, "admm": nd.admm_sharded, "anls": nd.anls_sharded}
    lines = []
    for name, case in HOST_CASES:
        v, w0, h0 = inputs(case)
        set_exchange_env(case)
        if case.get("api"):
            def run(case=case, v=v):
                np.random.seed(case["seed"])
                return nd.factorize(v.copy(), case["k"], method=case["solver"], backend="gloo", shard_factory=HostShard, **case["kw"])
        else:
            def run(case=case, v=v, w0=w0, h0=h0):
                r0, r1 = nd.row_range(case["m"], rank, world)
                cls = ChunkedHostShard if case.get("chunks") else SlicedHostShard if case.get("exchange") else HostShard
                shard = cls(v[r0:r1], case["k"], w0[r0:r1], h0)
                return solvers[case["solver"]](shard, nd.TorchComm(), batch=case["batch"], experiment=("digest", case["solver"]),
                                               **case["kw"], **case.get("extra", {}))
        sha, note = digest(run, log)
        lines.append(f"{name:<30} rank {rank}  {sha}  {note}")
    with open(os.path.join(outdir, f"rank{rank}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    tdist.barrier()
    tdist.destroy_process_group()


def host_main():
    import torch.multiprocessing as mp
    world = 2
    d = tempfile.mkdtemp(prefix="nmfx_digest_")
    try:
        mp.spawn(host_worker, args=(world, "file://" + os.path.join(d, "store"), d), nprocs=world, join=True)
        per_rank = [open(os.path.join(d, f"rank{r}.txt")).read().splitlines() for r in range(world)]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    for group in zip(*per_rank):
        for line in group:
            print(line)


def device_main(backend):
    for key in ("NMF_AMD_QUIET", "NMFX_DIST_GRAPH", "NMFX_DIST_NATIVE", "NMFX_DIST_MERGE"):
        os.environ.pop(key, None)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as tdist
    torch.cuda.set_device(0)
    d = tempfile.mkdtemp(prefix="nmfx_digest_")
    try:
        tdist.init_process_group("gloo" if backend == "native" else "nccl", init_method="file://" + os.path.join(d, "store"),
                                 rank=0, world_size=1, **({} if backend == "native" else {"device_id": torch.device("cuda:0")}))
        from nmf_amd import dist as nd
        log = []
        record_engine_calls(log)
        Comm = recording_comm(nd, log)
        solvers = {"mur": nd.mur_sharded, "ao_admm": nd.aoadmm_sharded, "admm": nd.admm_sharded, "anls": nd.anls_sharded}
        for name, case in DEVICE_CASES:
            v, w0, h0 = device_inputs(case)
            set_exchange_env(case)
            made = []

            def run(case=case, v=v, w0=w0, h0=h0):
                shard = (nd.NativeShard if backend == "native" else nd.DeviceShard)(v, case["k"], w0, h0, 0)
                made.append(shard)
                comm = nd.NativeComm.create(shard) if backend == "native" else Comm()
                made.append(comm)
                return solvers[case["solver"]](shard, comm, batch=case["batch"], experiment=("digest", case["solver"]),
                                               **case["kw"], **case.get("extra", {}))
            sha, note = digest(run, log)
            print(f"{backend:<6} {name:<30} {sha}  {note}", flush=True)
            if len(made) > 1 and backend == "native":
                made[1].close()
            if made:
                made[0].close()
        tdist.barrier()
        tdist.destroy_process_group()
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true", help="the device part: world of one on the GPU")
    ap.add_argument("--backend", choices=["nccl", "native"], default="nccl")
    args = ap.parse_args()
    if args.device:
        device_main(args.backend)
    else:
        host_main()
