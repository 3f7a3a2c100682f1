"""Several row shards of one MUR problem in lock step, in one process (tests/test_gpu_shard_step.py,
tests/test_shard_step_bars.py).

One engine per row shard, all on one device; the phase calls of the row-sharded protocol (include/nmfx.h) are issued shard by
shard, and the collective between them is done here on the host, in rank order, after a stream synchronise.  What comes out
-- the shards' rows of W stacked, every rank's H, objective history and state -- feeds the float64 step checks of
tests/mur_step.py, so the sharded-only device code (the pack of the exchange buffers, the chunked product, the objective
digits, the sliced H update and its unpack) is compared element by element like the single-handle path.

The driver does not care what it drives: a node is anything with `eng` (the phase methods under nmf_amd.engine.Engine's
names), the two exchange buffers as torch tensors, the padded k and n, and `slice_info` -- DeviceNode for the HIP engine,
HostNode for the numpy stand-ins of tests/host_shard.py.

Poison: before every phase A both exchange buffers of every shard are filled with NaN, and after the simulated
reduce-scatter the ranges a rank does not own are (the header calls them unspecified): whatever a kernel reads without
anybody having written it first reaches the factors as NaN and fails the step check.

Not covered: RCCL itself, more than one device, hipGraph replay (tests/test_gpu_dist.py has the process-group runs).

`run_sharded` drives MUR; the other solvers' sequences would be further `_iterate_*` functions over the same nodes and the
same HostCollective."""
import os
import struct

import numpy as np

import mur_step as S

NEVER = S.NEVER
XTAIL_RANKS = 64            # slots of the objective tail of the f32 exchange buffer (nmfx_set_exchange_rank)
FORMS = ("allreduce", "chunks", "rsag")


# ---- the objective partial as four 16-bit digits (include/nmfx.h, nmfx_set_exchange_rank) -----------------------------------
def encode_digits(x):
    """The f64 `x` as four f32 values, digit i = bits [16 i, 16 i + 16) of its representation: small exact integers, so a SUM
    over slots of which one is non-zero returns them unchanged."""
    bits = struct.unpack("<Q", struct.pack("<d", float(x)))[0]
    return np.array([(bits >> (16 * i)) & 0xFFFF for i in range(4)], dtype=np.float32)


def decode_digits(d):
    """Inverse of encode_digits; ValueError where a value is no whole number in [0, 65535] (a slot two ranks wrote into)."""
    bits = 0
    for i, val in enumerate(np.asarray(d, dtype=np.float64).tolist()):
        if not (0 <= val <= 0xFFFF and val == int(val)):
            raise ValueError(f"digit {i} is {val!r}: no 16-bit digit")
        bits |= int(val) << (16 * i)
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def same_bits(a, b):
    return struct.pack("<d", float(a)) == struct.pack("<d", float(b))


# ---- layouts of the f32 exchange buffer (include/nmfx.h, "Exchange buffers") ------------------------------------------------
def exchange_layout(kind, split_eu, kp, np_):
    """Where phase A leaves its partials.  split_eu: the split-bf16 Euclidean path (k padded to 64 / 128, precision bf16), the
    only one that stores the product [column][factor]; KL on that path, the exact-f32 kernels and k > 128 store it
    [factor][column].  Offsets in elements: g (W^T W, Euclidean), s (column sums of W, KL), tail (objective digits)."""
    lay = {"transposed": bool(split_eu and kind == "eu"), "kp": kp, "np": np_, "g": kp * np_, "tail": kp * np_ + kp * kp + kp}
    lay["s"] = kp * np_ + (kp * kp if kp > 128 else 0)
    return lay


def unpack_products(x32, lay, k, n, kind):
    """(B [k][n], W^T W [k][k] or None, column sums [k] or None) of one shard's f32 buffer, float64, padding cut off."""
    x = np.asarray(x32, dtype=np.float64)
    kp, np_ = lay["kp"], lay["np"]
    head = x[:kp * np_]
    b = head.reshape(np_, kp).T[:k, :n] if lay["transposed"] else head.reshape(kp, np_)[:k, :n]
    if kind == "eu":
        return b, x[lay["g"]:lay["g"] + kp * kp].reshape(kp, kp)[:k, :k], None
    return b, None, x[lay["s"]:lay["s"] + k]


# ---- nodes ------------------------------------------------------------------------------------------------------------------
class DeviceNode:
    """One Engine(rows, n, k) on device 0 with torch exchange buffers on torch's current stream (as dist.DeviceShard)."""

    def __init__(self, rank, v_local, k, w0_local, h0, precision=None):
        import torch
        from nmf_amd.engine import Engine
        self.torch = torch
        rows, n = v_local.shape
        self.eng = Engine(rows, n, k)
        try:
            if precision is not None:
                self.eng.set_precision(precision)
            requested = precision or ("f32" if os.environ.get("NMFX_PRECISION") in ("f32", "fp32") else "bf16")
            self.split = self.eng.precision() == "bf16"
            self.arith = "bf16" if self.split or (k > 128 and requested == "bf16") else "f32"      # (as mur_step.run_dense)
            n32, n64 = self.eng.exchange_sizes()
            self.x32 = torch.zeros(n32, dtype=torch.float32, device="cuda:0")
            self.x64 = torch.zeros(n64, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            self.eng.set_exchange_buffers(self.x32.data_ptr(), n32, self.x64.data_ptr(), n64)
            self.eng.set_stream(torch.cuda.current_stream().cuda_stream)
            _, self.np_, self.kp = self.eng.mur_chunk_info(0)
            self.eng.upload_v(v_local)
        except Exception:
            self.eng.close()
            raise

    def set_exchange(self, rank, world, merge):
        """True where the objective partial travels in the tail of the f32 buffer (dist.DeviceShard.negotiate)."""
        merged = bool(merge and self.split and world <= XTAIL_RANKS)
        self.eng.set_exchange_rank(*((rank, world) if merged else (0, 0)))
        return merged

    def layout(self, kind):
        return exchange_layout(kind, self.split, self.kp, self.np_)

    def slice_info(self, code, world):
        return self.eng.mur_slice_info(code, world)

    def sync(self):
        self.torch.cuda.current_stream().synchronize()

    def close(self):
        self.eng.close()


class HostNode:
    """A numpy stand-in of tests/host_shard.py (it is its own engine); both buffers float64, nothing padded."""
    arith = "f64"

    def __init__(self, shard, transposed=False):
        self.eng = shard
        self.x32, self.x64 = shard.buffers()
        self.kp, self.np_ = shard.k, shard.v.shape[1]
        self.transposed = transposed

    def set_exchange(self, rank, world, merge):
        return False

    def layout(self, kind):
        lay = exchange_layout(kind, self.transposed, self.kp, self.np_)
        lay["s"] = lay["g"]                      # (the stand-in keeps the KL column sums where the k <= 128 kernels do)
        return lay

    def slice_info(self, code, world):
        fn = getattr(self.eng, "slice_info", None)
        return fn(code, world) if fn else (0, 0)

    def sync(self):
        pass

    def close(self):
        pass


# ---- the collective, on the host ---------------------------------------------------------------------------------------------
class HostCollective:
    """Sums over the shards' buffers in rank order, in the buffers' own type (f32 for the device's products, f64 for the
    objective partials).  bufs: the shards' tensors in rank order; `what` names the buffer ("x32" / "x64") for the fault
    wrappers of tests/test_shard_step_bars.py.  Ranks that are absent from a sparse world contribute exact zeros."""

    @staticmethod
    def _parts(bufs, a, b):
        return [t[a:b].cpu().numpy().copy() for t in bufs]

    @staticmethod
    def _put(t, a, values):
        import torch
        t[a:a + values.size].copy_(torch.from_numpy(np.ascontiguousarray(values)))

    def total(self, parts):
        acc = parts[0].copy()
        for p in parts[1:]:
            acc = acc + p
        return acc

    def all_reduce(self, bufs, a, b, what):
        acc = self.total(self._parts(bufs, a, b))
        for t in bufs:
            self._put(t, a, acc)

    def reduce_scatter(self, bufs, ranks, elems, world):
        """Rank r receives the sum of [r elems, (r + 1) elems); the rest of [0, world elems) is unspecified: NaN."""
        parts = self._parts(bufs, 0, world * elems)
        for t, r in zip(bufs, ranks):
            out = np.full(world * elems, np.nan, dtype=parts[0].dtype)
            out[r * elems:(r + 1) * elems] = self.total([p[r * elems:(r + 1) * elems] for p in parts])
            self._put(t, 0, out)

    def all_gather(self, bufs, ranks, elems, world):
        mine = [t[r * elems:(r + 1) * elems].cpu().numpy().copy() for t, r in zip(bufs, ranks)]
        for t in bufs:
            for r, part in zip(ranks, mine):
                self._put(t, r * elems, part)


# ---- results -----------------------------------------------------------------------------------------------------------------
class Run:
    """One sharded run of s iterations.  w: the shards' rows stacked; hs / objs / states: per shard, in the order of `ranks`;
    form: the exchange form that ran ("allreduce" where `requested` was "rsag" and mur_slice_info said (0, 0));
    partials[j][i]: xf64[0] of shard i after phase A of iteration j (the last entry: after mur_finish_a);
    tails[j][i]: the tail of its f32 buffer there (merged runs); snaps[i]: (f32, f64 buffer) of shard i after phase A of
    iteration 0, before any sum (snapshot=True)."""

    def __init__(self):
        self.w = self.hs = self.objs = self.states = None
        self.form = self.requested = None
        self.merged = False
        self.ranks, self.world, self.cuts = (), 0, ()
        self.partials, self.tails, self.snaps, self.layouts = [], [], None, None
        self.arith = None

    def step(self, rank_index=0):
        """(W, H of the shard, its objective history): what mur_step.check_steps takes."""
        return self.w, self.hs[rank_index], self.objs[rank_index]


def steps_of(runs, rank_index=0):
    return {s: r.step(rank_index) for s, r in runs.items()}


def ranks_differ(run):
    """Names of what is not bit-identical on every rank (H, objective history, state): [] when all agree."""
    out = []
    for i in range(1, len(run.hs)):
        if not np.array_equal(run.hs[i], run.hs[0], equal_nan=True):
            cols = np.flatnonzero(np.any(run.hs[i] != run.hs[0], axis=0))
            out.append(f"H of rank {run.ranks[i]} differs from rank {run.ranks[0]}'s in {cols.size} columns "
                       f"({int(cols[0])} .. {int(cols[-1])}: 64-column blocks {int(cols[0]) // 64} .. {int(cols[-1]) // 64})")
        if not np.array_equal(run.objs[i], run.objs[0], equal_nan=True):
            out.append(f"objective history of rank {run.ranks[i]} differs from rank {run.ranks[0]}'s")
        if tuple(run.states[i]) != tuple(run.states[0]):
            out.append(f"state of rank {run.ranks[i]} {tuple(run.states[i])} != {tuple(run.states[0])}")
    return out


# ---- the driver --------------------------------------------------------------------------------------------------------------
def _poison(nodes):
    for nd_ in nodes:
        nd_.x32.fill_(float("nan"))
        nd_.x64.fill_(float("nan"))


def _sync(nodes):
    for nd_ in nodes:
        nd_.sync()


def _note_partials(run, nodes, tail):
    run.partials.append([float(nd_.x64[0]) for nd_ in nodes])
    run.tails.append([nd_.x32[tail:tail + 4 * XTAIL_RANKS].cpu().numpy().copy() for nd_ in nodes] if run.merged else None)


def _iterate_mur(run, nodes, coll, code, lw, lh, stop, j, ranges, plan, snapshot):
    """One outer iteration in the form run.form, from the protocol in include/nmfx.h."""
    x32 = [nd_.x32 for nd_ in nodes]
    x64 = [nd_.x64 for nd_ in nodes]
    n32 = int(x32[0].numel())
    kp, tail = nodes[0].kp, nodes[0].layout("eu")["tail"]
    snap = [np.full(n32, np.nan, dtype=np.float64) for _ in nodes] if snapshot else None

    def keep(a, b):
        if snap is not None:
            for s_, t in zip(snap, x32):
                s_[a:b] = t[a:b].cpu().numpy()

    _poison(nodes)
    if run.form == "chunks":
        for nd_ in nodes:
            nd_.eng.mur_phase_a_head(code, lw, j)
        for i, (c0, c1) in enumerate(ranges):
            for nd_ in nodes:
                nd_.eng.mur_phase_a_cols(code, c0, c1)
            _sync(nodes)
            a, b = c0 * kp, (n32 if i == len(ranges) - 1 else c1 * kp)
            keep(a, b)
            if i == len(ranges) - 1:
                _note_partials(run, nodes, tail)
            coll.all_reduce(x32, a, b, "x32")
    else:
        for nd_ in nodes:
            nd_.eng.mur_phase_a(code, lw, j)
        _sync(nodes)
        keep(0, n32)
        _note_partials(run, nodes, tail)
    if snap is not None:
        run.snaps = [(s_, nd_.x64.cpu().numpy().copy()) for s_, nd_ in zip(snap, nodes)]
    if run.form == "rsag":
        cols, elems = plan
        coll.reduce_scatter(x32, run.ranks, elems, run.world)
        coll.all_reduce(x32, run.world * elems, n32, "x32")
    elif run.form == "allreduce":
        coll.all_reduce(x32, 0, n32, "x32")
    if not run.merged:
        coll.all_reduce(x64, 0, 8, "x64")
    if run.form == "rsag":
        for nd_, r in zip(nodes, run.ranks):
            nd_.eng.mur_phase_b_slice(code, lh, *stop, j, r * cols, (r + 1) * cols)
        _sync(nodes)
        coll.all_gather(x32, run.ranks, elems, run.world)
        for nd_, r in zip(nodes, run.ranks):
            nd_.eng.mur_phase_b_rest(code, r * cols, (r + 1) * cols)
    else:
        for nd_ in nodes:
            nd_.eng.mur_phase_b(code, lh, *stop, j)


def _close_mur(run, nodes, coll, code, stop, done):
    _poison(nodes)
    for nd_ in nodes:
        nd_.eng.mur_finish_a(code, done)
    _sync(nodes)
    run.partials.append([float(nd_.x64[0]) for nd_ in nodes])
    run.tails.append(None)
    coll.all_reduce([nd_.x64 for nd_ in nodes], 0, 8, "x64")
    for nd_ in nodes:
        nd_.eng.mur_finish_b(*stop, done)


def run_sharded(v, w0, h0, kind, lw, lh, cuts, form, precision=None, merge=True, ranks=None, world=None, steps=(1, 2),
                make_engine=None, ranges=None, stop=None, snapshot=False, collective=None):
    """{s: Run} of s = 1, 2, ... iterations of MUR ('eu' | 'kl') over the row shards [cuts[i], cuts[i + 1]) of V, each from the
    start (w0, h0).  form: "allreduce", "chunks" (ranges = [(c0, c1), ...] in padded columns, ascending, the last one ending
    at the padded n) or "rsag".  ranks / world: the rank ids the shards claim (default 0 .. len - 1 of a world of that size;
    fewer shards than ranks make a sparse world).  stop = (min_iter, tol1, tol2), default off.  make_engine(rank, v_local, k,
    w0_local, h0) returns a node (default: DeviceNode with `precision`).  An error of any engine call ends the run."""
    if form not in FORMS:
        raise ValueError(f"form {form!r}: one of {FORMS}")
    cuts = [int(c) for c in cuts]
    nshard = len(cuts) - 1
    if nshard < 1 or cuts[0] != 0 or cuts[-1] != v.shape[0] or any(a >= b for a, b in zip(cuts[:-1], cuts[1:])):
        raise ValueError(f"cuts {cuts}: ascending row boundaries from 0 to {v.shape[0]}")
    ranks = list(range(nshard)) if ranks is None else [int(r) for r in ranks]
    world = (max(ranks) + 1 if world is None else int(world))
    if len(ranks) != nshard or sorted(set(ranks)) != ranks or ranks[0] < 0 or ranks[-1] >= world:
        raise ValueError(f"ranks {ranks}: one ascending rank id below the world's {world} per shard")
    if form == "rsag" and ranks != list(range(world)):
        raise ValueError("the reduce-scatter / all-gather form needs every rank of the world (each owns columns of H)")
    if form == "chunks" and not ranges:
        raise ValueError("the chunked form needs its column ranges")
    k = w0.shape[1]
    code = 0 if kind == "eu" else 1
    stop = (NEVER, 0.0, 0.0) if stop is None else tuple(stop)
    coll = collective or HostCollective()
    if make_engine is None:
        def make_engine(rank, v_local, k_, w_local, h_):
            return DeviceNode(rank, v_local, k_, w_local, h_, precision=precision)
    nodes = []
    out = {}
    try:
        for i, r in enumerate(ranks):
            nodes.append(make_engine(r, v[cuts[i]:cuts[i + 1]], k, w0[cuts[i]:cuts[i + 1]], h0))
        merged = [nd_.set_exchange(r, world, merge) for nd_, r in zip(nodes, ranks)]
        if len(set(merged)) != 1:
            raise RuntimeError("the shards disagree about carrying the objective in the f32 buffer")
        plan, actual = None, form
        if form == "rsag":
            plans = {tuple(nd_.slice_info(code, world)) for nd_ in nodes}
            if len(plans) != 1:
                raise RuntimeError(f"the shards disagree about the column slices: {plans}")
            plan = plans.pop()
            if not plan[0]:
                plan, actual = None, "allreduce"
        for s in steps:
            run = Run()
            run.form, run.requested, run.merged = actual, form, merged[0] and code == 0
            run.ranks, run.world, run.cuts, run.arith = tuple(ranks), world, tuple(cuts), nodes[0].arith
            run.layouts = [nd_.layout(kind) for nd_ in nodes]
            for i, nd_ in enumerate(nodes):
                nd_.eng.set_factors(w0[cuts[i]:cuts[i + 1]], h0)
            for j in range(s):
                _iterate_mur(run, nodes, coll, code, lw, lh, stop, j, ranges, plan, snapshot and j == 0)
            _close_mur(run, nodes, coll, code, stop, s)
            _sync(nodes)
            got = [nd_.eng.get_factors() for nd_ in nodes]
            run.w = np.concatenate([w for w, _ in got], axis=0)
            run.hs = [h for _, h in got]
            run.states = [tuple(nd_.eng.state()) for nd_ in nodes]
            run.objs = [np.asarray(nd_.eng.objectives(0, st[2])) for nd_, st in zip(nodes, run.states)]
            out[s] = run
    finally:
        for nd_ in nodes:
            nd_.close()
    return out


# ---- checks shared by the GPU test and the CPU proof -------------------------------------------------------------------------
def check(kind, v, w0, h0, runs, lw, lh, bar, rank_index=0, obj_rtol=S.OBJ_RTOL):
    """mur_step.check_steps with W the shards' rows stacked and the H / objective history of one rank; a failure names it."""
    tag = "" if rank_index == 0 else f"rank {runs[min(runs)].ranks[rank_index]}: "
    return S.check_steps(kind, v, w0, h0, steps_of(runs, rank_index), lw, lh, bar, obj_rtol=obj_rtol, tag=tag)


def check_partials(kind, v, run, w_new, h_prev, bar):
    """Assertion (c): each shard's f32 buffer after phase A of iteration 0 against float64 W1_local^T V_local and
    W1_local^T W1_local (KL: the quotient product and the column sums of W1_local), via mur_step.compare.  w_new: the
    device's W after that iteration, stacked; h_prev: the H it started from."""
    from oracle import nmf_ref as R
    fails = []
    k, n = w_new.shape[1], v.shape[1]
    for i, (x32, _) in enumerate(run.snaps):
        a, b = run.cuts[i], run.cuts[i + 1]
        vl = np.asarray(v[a:b], dtype=np.float64)
        wl = w_new[a:b]
        got_b, got_g, got_s = unpack_products(x32, run.layouts[i], k, n, kind)
        who = f"rank {run.ranks[i]} (rows {a} .. {b - 1}) "
        lay = run.layouts[i]
        full = np.asarray(x32[:lay["kp"] * lay["np"]], dtype=np.float64)
        full = full.reshape(lay["np"], lay["kp"]).T if lay["transposed"] else full.reshape(lay["kp"], lay["np"])
        pad = int(np.count_nonzero(full[k:])) + int(np.count_nonzero(full[:k, n:]))
        if pad:
            fails.append(f"{who}product: {pad} elements of the padded factors / columns are not zero")
        if kind == "eu":
            pairs = [("W^T V", got_b, wl.T @ vl), ("W^T W", got_g, wl.T @ wl)]
        else:
            pairs = [("W^T (V / W H)", got_b, wl.T @ (vl / (wl @ h_prev + R.EPS))), ("column sums of W", got_s[None, :], wl.sum(axis=0)[None, :])]
        for name, got, want in pairs:
            _, msg = S.compare(who + name, got, want, bar)
            if msg:
                fails.append(msg)
    if fails:
        raise AssertionError("\n".join(fails))


def check_objective_sums(run, merged_slots=True):
    """Assertion (d): every recorded objective is the float64 sum of the shards' partials in rank order, bit for bit; in a
    merged run slot r of the tail holds the digits of rank r's partial and every other slot up to the world's size +0.0."""
    fails = []
    hist = run.objs[0]
    for j, parts in enumerate(run.partials):
        if j >= len(hist):
            break
        total = 0.0
        for p in parts:
            total += p
        if not same_bits(total, hist[j]):
            fails.append(f"obj[{j}]: recorded {float(hist[j])!r}, the partials {parts} sum to {total!r} in rank order")
        if not merged_slots or run.tails[j] is None:
            continue
        for i, tail in enumerate(run.tails[j]):
            for r in range(run.world):
                slot = tail[4 * r:4 * r + 4]
                if r == run.ranks[i]:
                    try:
                        ok = same_bits(decode_digits(slot), parts[i])
                    except ValueError:
                        ok = False
                    if not ok:
                        fails.append(f"iteration {j}, rank {r}: its tail slot {slot.tolist()} does not hold the digits of its partial {parts[i]!r}")
                elif not (np.all(slot == 0) and not np.any(np.signbit(slot))):
                    fails.append(f"iteration {j}, rank {run.ranks[i]}: slot {r} of its tail is {slot.tolist()}, not +0.0")
    if fails:
        raise AssertionError("\n".join(fails))
