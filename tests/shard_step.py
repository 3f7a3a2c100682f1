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

`run_sharded` drives MUR.  `run_family` (ADMM, AO-ADMM in its round-by-round, speculative and KL forms) and `run_anls` drive the
other solvers' sequences over the same nodes and the same HostCollective, one `_iterate_*` function per sequence of
include/nmfx.h / nmf_amd/dist.py, and feed the step checks of tests/admm_step.py and tests/anls_step.py
(tests/test_gpu_shard_family_step.py, tests/test_shard_family_bars.py).  Their poison follows the table "who writes, who reads"
of include/nmfx.h: before every phase that precedes a collective, everything of both buffers that the table does not keep
alive from an earlier phase is NaN (_keep_poison)."""
import os
import struct

import numpy as np

import admm_step as A
import anls_step as N
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

    def counters(self):
        """(diagnostics, NNLS fall-backs) of the engine, as anls_step.Run keeps them."""
        return self.eng.diagnostics(), self.eng.nnls_fallbacks()

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

    def counters(self):
        return (0, 0), (0, 0)

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


# =============================================================================================================================
# ADMM, AO-ADMM and ANLS: the sequences of include/nmfx.h and nmf_amd/dist.py (admm_sharded, aoadmm_sharded, anls_sharded)
# =============================================================================================================================
T_OFF = (NEVER, 0, 0)       # (min_iter, tol1, tol2): the stop rule off
AO_FORMS = ("rounds", "fused")


def _keep_poison(nodes, keep32=(), keep64=()):
    """NaN into both exchange buffers of every shard except the ranges [(a, b)] that must survive from an earlier phase (on the
    buffers' own stream: ordered behind the phase that wrote them and before the one that follows)."""
    for nd_ in nodes:
        saved = [(t, a, t[a:b].clone()) for t, ranges in ((nd_.x32, keep32), (nd_.x64, keep64)) for a, b in ranges]
        nd_.x32.fill_(float("nan"))
        nd_.x64.fill_(float("nan"))
        for t, a, val in saved:
            t[a:a + val.numel()].copy_(val)


def family_layout(kp, np_):
    """The f32 buffer behind the products phase of ADMM, AO-ADMM (both losses) and ANLS, k <= 128 and composed, either arithmetic
    mode (mur_pack_kernel, pack_t_kernel, the generic products): [factor][column] at 0, the Gram matrix [kp][kp] at kp n_pad."""
    return {"kp": kp, "np": np_, "g": kp * np_}


class FamilyRun:
    """Two steps of ADMM / AO-ADMM over row shards.  states: [State after step 1, after step 2] (admm_step.State) with w, w_aux,
    dual_w stacked over the shards in row order and h, h_aux, dual_h and the inner words of shard `rank_index`;
    rank_states[step][i]: what shard i held; objs / flags: per shard the objective history 0 .. 2 and state();
    partials[t][i]: xf64[0] of shard i before the t-th objective collective (t = iteration, the last one the closing);
    norms: [(j, round or "table", [array per shard])] before every collective of the W sub-problem (norm_decision_failures
    re-derives the stop from their rank-order sums);
    snaps[i]: shard i's f32 buffer (as float64) after the first products phase of the run, before any sum."""

    def __init__(self):
        self.states, self.rank_states, self.objs, self.flags = [], [], None, None
        self.partials, self.norms, self.snaps, self.layouts = [], [], None, None
        self.ranks, self.cuts, self.arith, self.form, self.case = (), (), None, None, None

    def of_rank(self, i):
        """[State, State] with the replicated parts of shard i (the stacked W parts are everybody's)."""
        return [st._replace(h=rs[i].h, h_aux=rs[i].h_aux, dual_h=rs[i].dual_h, words=rs[i].words) for st, rs in zip(self.states, self.rank_states)]


def _note_objective(run, nodes, snap):
    run.partials.append([float(nd_.x64[0]) for nd_ in nodes])
    if snap:
        run.snaps = [nd_.x32.cpu().numpy().astype(np.float64) for nd_ in nodes]
        run.layouts = [family_layout(nd_.kp, nd_.np_) for nd_ in nodes]


def _reduce_products(nodes, coll, objective=True):
    """The all-reduce of (x32, x64[:8]) of dist.py: the whole f32 buffer and the head of the f64 one."""
    coll.all_reduce([nd_.x32 for nd_ in nodes], 0, int(nodes[0].x32.numel()), "x32")
    if objective:
        coll.all_reduce([nd_.x64 for nd_ in nodes], 0, 8, "x64")


def _carried_objective(nodes, j):
    """Beyond 128 components AO-ADMM and ADMM close every iteration with the objective partial of the new pair in xf64[0] and the
    next products phase (and nmfx_objective_partial) leave it there: the one range that survives from an earlier phase."""
    return [(0, 1)] if nodes[0].kp > 128 and j > 0 else ()


def _w_rounds(run, nodes, coll, call, close, admm_iter, j):
    """{ round r . all-reduce of f64 [1, 5) } x admm_iter . close: round r > 0 reads the reduced sums of round r - 1 there."""
    for r in range(admm_iter):
        _keep_poison(nodes, keep64=[(1, 5)] if r > 0 else ())
        for nd_ in nodes:
            call(nd_.eng, r)
        _sync(nodes)
        run.norms.append((j, r, [nd_.x64[1:5].cpu().numpy().copy() for nd_ in nodes]))
        coll.all_reduce([nd_.x64 for nd_ in nodes], 1, 5, "norms")
    for nd_ in nodes:
        close(nd_.eng)


def _iterate_admm(run, nodes, coll, c, codes, j, snap, stop=T_OFF):
    """phase_products . all-reduce . phase_update (both losses)."""
    dist, pw, ph = codes
    _keep_poison(nodes, keep64=_carried_objective(nodes, j))
    for nd_ in nodes:
        nd_.eng.admm_phase_products(dist, c.rho, pw, ph, j)
    _sync(nodes)
    _note_objective(run, nodes, snap)
    _reduce_products(nodes, coll)
    for nd_ in nodes:
        nd_.eng.admm_phase_update(dist, c.rho, pw, c.lam_w, ph, c.lam_h, *stop, j)


def _iterate_aoadmm(run, nodes, coll, c, codes, j, snap, fused, stop=T_OFF):
    """phase_h_products . all-reduce . phase_h_solve . phase_w_products . then the W sub-problem round by round, or (fused)
    phase_w_fused . all-reduce of the table f64 [8, 8 + 4 admm_iter) . phase_w_repair."""
    _, pw, ph = codes
    it = c.admm_iter
    _keep_poison(nodes, keep64=_carried_objective(nodes, j))
    for nd_ in nodes:
        nd_.eng.aoadmm_phase_h_products(j)
    _sync(nodes)
    _note_objective(run, nodes, snap)
    _reduce_products(nodes, coll)
    for nd_ in nodes:
        nd_.eng.aoadmm_phase_h_solve(ph, c.lam_h, it, *stop, j)
        nd_.eng.aoadmm_phase_w_products(*stop, j)
    if not fused:
        _w_rounds(run, nodes, coll, lambda e, r: e.aoadmm_phase_w_round(pw, c.lam_w, r), lambda e: e.aoadmm_phase_w_close(it, j), it, j)
        return
    _keep_poison(nodes)
    for nd_ in nodes:
        nd_.eng.aoadmm_phase_w_fused(pw, c.lam_w, it)
    _sync(nodes)
    run.norms.append((j, "table", [nd_.x64[8:8 + 4 * it].cpu().numpy().copy().reshape(it, 4) for nd_ in nodes]))
    coll.all_reduce([nd_.x64 for nd_ in nodes], 8, 8 + 4 * it, "table")
    for nd_ in nodes:
        nd_.eng.aoadmm_phase_w_repair(pw, c.lam_w, it, j)


def _iterate_aoadmm_kl(run, nodes, coll, c, codes, j, snap, stop=T_OFF):
    """An exchange in every inner round of both sub-problems; v_aux and dual_v stay on their ranks."""
    _, pw, ph = codes
    it = c.admm_iter
    for r in range(it):
        _keep_poison(nodes, keep64=_carried_objective(nodes, j) if r == 0 else ())
        for nd_ in nodes:
            nd_.eng.aoadmm_kl_phase_h_products(j, r)
        _sync(nodes)
        if r == 0:
            _note_objective(run, nodes, snap)
        _reduce_products(nodes, coll, objective=r == 0)
        for nd_ in nodes:
            nd_.eng.aoadmm_kl_phase_h_round(ph, c.lam_h, r, *stop, j)
    for nd_ in nodes:
        nd_.eng.aoadmm_kl_phase_h_close(it, *stop, j)
    _w_rounds(run, nodes, coll, lambda e, r: e.aoadmm_kl_phase_w_round(pw, c.lam_w, r), lambda e: e.aoadmm_kl_phase_w_close(it, j), it, j)


def _iterate_anls(run, nodes, coll, lw, lh, j, snap=False, stop_after_w=False, stop=T_OFF):
    """phase_objective . all-reduce f64 . phase_w . all-reduce f32 . phase_h."""
    _keep_poison(nodes)
    for nd_ in nodes:
        nd_.eng.anls_phase_objective(j)
    _sync(nodes)
    run.partials.append([float(nd_.x64[0]) for nd_ in nodes])
    coll.all_reduce([nd_.x64 for nd_ in nodes], 0, 8, "x64")
    _keep_poison(nodes, keep64=[(0, 1)])                # (phase_w records the reduced objective)
    for nd_ in nodes:
        nd_.eng.anls_phase_w(lw, *stop, j)
    _sync(nodes)
    if snap:
        run.snaps = [nd_.x32.cpu().numpy().astype(np.float64) for nd_ in nodes]
        run.layouts = [family_layout(nd_.kp, nd_.np_) for nd_ in nodes]
    if stop_after_w:
        return
    _reduce_products(nodes, coll, objective=False)
    for nd_ in nodes:
        nd_.eng.anls_phase_h(lh, j)


def _close_family(run, nodes, coll, done, carried, stop=T_OFF):
    """nmfx_objective_partial . all-reduce . nmfx_mur_finish_b (dist._finish_run).  carried: the composed AO-ADMM / ADMM phases have
    left the partial in xf64[0] and nmfx_objective_partial only leaves it there."""
    _keep_poison(nodes, keep64=[(0, 1)] if carried else ())
    for nd_ in nodes:
        nd_.eng.objective_partial()
    _sync(nodes)
    run.partials.append([float(nd_.x64[0]) for nd_ in nodes])
    coll.all_reduce([nd_.x64 for nd_ in nodes], 0, 8, "x64")
    for nd_ in nodes:
        nd_.eng.mur_finish_b(*stop, done)


def _check_cuts(cuts, m):
    cuts = [int(x) for x in cuts]
    if len(cuts) < 2 or cuts[0] != 0 or cuts[-1] != m or any(a >= b for a, b in zip(cuts[:-1], cuts[1:])):
        raise ValueError(f"cuts {cuts}: ascending row boundaries from 0 to {m}")
    return cuts


def _same_mode(nodes, want=None):
    modes = {nd_.arith for nd_ in nodes}
    if len(modes) != 1:
        raise AssertionError(f"the shards run different arithmetic modes: {[nd_.arith for nd_ in nodes]}")
    mode = modes.pop()
    if want is not None and mode not in ("f64", want):
        raise AssertionError(f"the shards run in {mode} arithmetic, the case asks for {want}")
    return mode


def _read_state(eng, c):
    w, h = eng.get_factors()
    if c.family == "admm":
        return A.State(w, h, eng.get_matrix("w_aux"), eng.get_matrix("h_aux"), eng.get_matrix("dual_w"), eng.get_matrix("dual_h"), (0, 0))
    return A.State(w, h, None, None, eng.get_matrix("dual_w"), eng.get_matrix("dual_h"), (0, 0))


def _stack(states, rank_index):
    cat = lambda name: None if getattr(states[0], name) is None else np.concatenate([getattr(st, name) for st in states], axis=0)
    mine = states[rank_index]
    return A.State(cat("w"), mine.h, cat("w_aux"), mine.h_aux, cat("dual_w"), mine.dual_h, mine.words)


def run_family(c, cuts, form="rounds", make_engine=None, collective=None, lead="phases", rank_index=0, stop=T_OFF):
    """Case c (admm_step.Case) over the row shards `cuts`: step 1 and step 2 from the case's start, the state read in between
    (get_factors, get_matrix) and the inner words and objectives after the closing, as admm_step.run_device.  form: the W
    sub-problem of Euclidean AO-ADMM, "rounds" or "fused".  stop = (min_iter, tol1, tol2), default off.  lead = "run": step 1 through the solver's run entry point, as
    admm_step.run_device(phases=...) does (a world of one only).  Returns a FamilyRun."""
    if form not in AO_FORMS:
        raise ValueError(f"form {form!r}: one of {AO_FORMS}")
    v, w0, h0 = A.make_case(c)
    cuts = _check_cuts(cuts, c.m)
    if lead == "run" and len(cuts) != 2:
        raise ValueError("the run entry points know one shard only")
    if c.family == "admm" and c.prox_w in ("l1inf", "l1inf_transpose"):
        raise ValueError("the l1inf operators on W couple all rows: not available row-sharded")
    from nmf_amd import _lib as L
    codes = (L.EU if c.loss == "eu" else L.KL), L.PROX[c.prox_w], L.PROX[c.prox_h]
    coll = collective or HostCollective()
    if make_engine is None:
        def make_engine(rank, v_local, k_, w_local, h_):
            return DeviceNode(rank, v_local, k_, w_local, h_, precision=c.arith)
    fused = form == "fused" and c.family == "ao" and c.loss == "eu"
    run = FamilyRun()
    run.case, run.cuts, run.ranks, run.form = c, tuple(cuts), tuple(range(len(cuts) - 1)), form
    nodes = []
    try:
        for i in run.ranks:
            nodes.append(make_engine(i, v[cuts[i]:cuts[i + 1]], c.k, w0[cuts[i]:cuts[i + 1]], h0))
        run.arith = _same_mode(nodes, c.arith if c.k > 32 else None)
        if c.family == "admm":
            for which, op in enumerate(A.operators(c)):
                if op is not None:
                    for nd_ in nodes:
                        nd_.eng.set_l2n_operator(which, op)
        for i, nd_ in enumerate(nodes):
            nd_.eng.set_factors(w0[cuts[i]:cuts[i + 1]], h0)

        def iterate(j, snap):
            if c.family == "admm":
                _iterate_admm(run, nodes, coll, c, codes, j, snap, stop)
            elif c.loss == "eu":
                _iterate_aoadmm(run, nodes, coll, c, codes, j, snap, fused, stop)
            else:
                _iterate_aoadmm_kl(run, nodes, coll, c, codes, j, snap, stop)

        if lead == "run":
            A._run(nodes[0].eng, c, 0, 1)
            run.partials.append(None)                   # (obj[0] has no collective of the driver's behind it)
        else:
            iterate(0, True)
        _sync(nodes)
        run.rank_states.append([_read_state(nd_.eng, c) for nd_ in nodes])
        iterate(1, False)
        _close_family(run, nodes, coll, 2, carried=nodes[0].kp > 128, stop=stop)
        _sync(nodes)
        run.rank_states.append([_read_state(nd_.eng, c) for nd_ in nodes])
        run.flags = [tuple(nd_.eng.state()) for nd_ in nodes]
        run.objs = [np.asarray(nd_.eng.objectives(0, fl[2])) for nd_, fl in zip(nodes, run.flags)]
        if c.family == "ao":
            for i, nd_ in enumerate(nodes):
                wd = tuple(int(x) for x in np.asarray(nd_.eng.inner_counts(0, 2)).reshape(-1))
                for s in (0, 1):
                    run.rank_states[s][i] = run.rank_states[s][i]._replace(words=wd[2 * s:2 * s + 2])
        run.states = [_stack(rs, rank_index) for rs in run.rank_states]
    finally:
        for nd_ in nodes:
            nd_.close()
    return run


class AnlsRuns:
    """runs: {s: anls_step.Run} of s = 1, 2 iterations, each from the start -- W the shards' rows stacked, H, the objectives and
    the counters of shard `rank_index`; w_mid: the stacked W after anls_phase_w of iteration 0 alone; per s: hs / objs / flags per
    shard, partials[s][t][i] as FamilyRun.partials; snaps: the f32 buffers behind that first anls_phase_w."""

    def __init__(self):
        self.runs, self.w_mid, self.hs, self.objs, self.flags, self.partials = {}, None, {}, {}, {}, {}
        self.snaps = self.layouts = None
        self.ranks, self.cuts, self.arith = (), (), None


def run_anls(c, cuts, kind="eu", make_engine=None, collective=None, rank_index=0, steps=(1, 2), stop=T_OFF):
    """Case c (anls_step.Case) over the row shards `cuts` with the recorded objective `kind`, as anls_step.run_phases."""
    v, w0, h0 = N.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = N.lam_of(c)
    cuts = _check_cuts(cuts, c.m)
    coll = collective or HostCollective()
    from nmf_amd import _lib as L
    code = L.EU if kind == "eu" else L.KL
    if make_engine is None:
        def make_engine(rank, v_local, k_, w_local, h_):
            return DeviceNode(rank, v_local, k_, w_local, h_, precision=c.arith if c.k <= 128 else None)
    out = AnlsRuns()
    out.cuts, out.ranks = tuple(cuts), tuple(range(len(cuts) - 1))
    nodes = []
    try:
        for i in out.ranks:
            nodes.append(make_engine(i, v[cuts[i]:cuts[i + 1]], c.k, w0[cuts[i]:cuts[i + 1]], h0))
        out.arith = _same_mode(nodes, c.arith if 32 < c.k <= 128 else None)

        def start():
            for i, nd_ in enumerate(nodes):
                nd_.eng.set_factors(w0[cuts[i]:cuts[i + 1]], h0)
                nd_.eng.anls_set_distance(code)

        class Notes:                                    # (what _iterate_anls and _close_family note down, per run)
            def __init__(self):
                self.partials, self.snaps, self.layouts = [], None, None

        start()
        first = Notes()
        _iterate_anls(first, nodes, coll, lw, lh, 0, snap=True, stop_after_w=True, stop=stop)
        out.snaps, out.layouts = first.snaps, first.layouts
        got = [nd_.eng.get_factors() for nd_ in nodes]
        out.w_mid = np.concatenate([w for w, _ in got], axis=0)
        for i, (_, h) in enumerate(got):
            if not np.array_equal(h, A.f32(h0)):
                raise AssertionError(f"anls_phase_w moved H on rank {i}")
        for s in steps:
            notes = Notes()
            start()
            for j in range(s):
                _iterate_anls(notes, nodes, coll, lw, lh, j, stop=stop)
            _close_family(notes, nodes, coll, s, carried=False, stop=stop)
            _sync(nodes)
            out.partials[s] = notes.partials
            got = [nd_.eng.get_factors() for nd_ in nodes]
            out.hs[s] = [h for _, h in got]
            out.flags[s] = [tuple(nd_.eng.state()) for nd_ in nodes]
            out.objs[s] = [np.asarray(nd_.eng.objectives(0, s + 1)) for nd_ in nodes]
            mine = nodes[rank_index]
            out.runs[s] = N.Run(np.concatenate([w for w, _ in got], axis=0), out.hs[s][rank_index], out.objs[s][rank_index],
                                mine.counters()[0], mine.counters()[1])
    finally:
        for nd_ in nodes:
            nd_.close()
    return out


# ---- the assertions every family case makes beside its step checks -----------------------------------------------------------
def _differs(name, a, b, ra, rb):
    if a is None and b is None:
        return None
    if np.array_equal(a, b, equal_nan=True):
        return None
    cols = np.flatnonzero(np.any(np.asarray(a) != np.asarray(b), axis=0))
    return (f"{name} of rank {ra} differs from rank {rb}'s in {cols.size} columns ({int(cols[0])} .. {int(cols[-1])}: 64-column "
            f"blocks {int(cols[0]) // 64} .. {int(cols[-1]) // 64})")


def family_ranks_differ(run):
    """(a) Names of what is not bit-identical on every rank of a FamilyRun: h, h_aux, dual_h and the inner words behind each
    step, the objective history, state().  [] when all agree."""
    out = []
    for s, states in enumerate(run.rank_states, start=1):
        for i in range(1, len(states)):
            for name in ("h", "h_aux", "dual_h"):
                msg = _differs(f"step {s}: {name}", getattr(states[i], name), getattr(states[0], name), run.ranks[i], run.ranks[0])
                if msg:
                    out.append(msg)
            if tuple(states[i].words) != tuple(states[0].words):
                out.append(f"step {s}: inner words of rank {run.ranks[i]} {tuple(states[i].words)} != rank {run.ranks[0]}'s {tuple(states[0].words)}")
    for i in range(1, len(run.objs)):
        if not np.array_equal(run.objs[i], run.objs[0], equal_nan=True):
            out.append(f"objective history of rank {run.ranks[i]} {run.objs[i]} differs from rank {run.ranks[0]}'s {run.objs[0]}")
        if tuple(run.flags[i]) != tuple(run.flags[0]):
            out.append(f"state of rank {run.ranks[i]} {tuple(run.flags[i])} != {tuple(run.flags[0])}")
    return out


def anls_ranks_differ(out):
    msgs = []
    for s in sorted(out.runs):
        for i in range(1, len(out.hs[s])):
            msg = _differs(f"{s}-step run: H", out.hs[s][i], out.hs[s][0], out.ranks[i], out.ranks[0])
            if msg:
                msgs.append(msg)
            if not np.array_equal(out.objs[s][i], out.objs[s][0], equal_nan=True):
                msgs.append(f"{s}-step run: objective history of rank {out.ranks[i]} differs from rank {out.ranks[0]}'s")
            if tuple(out.flags[s][i]) != tuple(out.flags[s][0]):
                msgs.append(f"{s}-step run: state of rank {out.ranks[i]} {tuple(out.flags[s][i])} != {tuple(out.flags[s][0])}")
    return msgs


def objective_sum_failures(partials, hist, tag=""):
    """(b) hist[t] against the float64 sum of partials[t] in rank order, bit for bit."""
    fails = []
    if len(hist) != len(partials):
        fails.append(f"{tag}{len(hist)} recorded objectives, {len(partials)} objective collectives")
    for t, parts in enumerate(partials[:len(hist)]):
        if parts is None:
            continue
        total = 0.0
        for p in parts:
            total += p
        if not same_bits(total, hist[t]):
            fails.append(f"{tag}obj[{t}]: recorded {float(hist[t])!r}, the partials {parts} sum to {total!r} in rank order")
    return fails


def norm_decision_failures(run):
    """The W sub-problem's inner word of every rank against the decision re-derived from the noted norm sums: the shards' f64
    [1, 5) of every round (or their tables) summed in rank order, `terminate` (ao_admm.py:33-43) on the sums, the first round at
    which it holds.  What a rank noted behind the stop is stale and not looked at."""
    c = run.case
    fails = []
    for j in sorted({j for j, _, _ in run.norms}):
        rows = []
        for jj, r, parts in run.norms:
            if jj != j:
                continue
            total = np.zeros_like(np.asarray(parts[0], dtype=np.float64))
            for p in parts:
                total = total + p
            rows += [total] if r != "table" else list(total)
        ran, fired = len(rows), 0
        for r, (n0, n1, n2, n3) in enumerate(rows):
            with np.errstate(all="ignore"):
                stop = bool(np.sqrt(n0) / np.sqrt(n1) < A.STOP_TOL and np.sqrt(n2) / np.sqrt(n3) < A.STOP_TOL)
            if stop:
                ran, fired = r + 1, 1
                break
        want = ran | fired << 16
        for i, st in enumerate(run.rank_states[j]):
            if int(st.words[1]) != want:
                fails.append(f"step {j + 1}: rank {run.ranks[i]} records the W word {int(st.words[1]) & 0xFFFF} rounds (break bit {int(st.words[1]) >> 16}), the "
                             f"rank-order sums of the noted norm sums stop after {ran} (break {fired})")
    return fails


def partial_failures(snaps, layouts, cuts, k, n, pairs, bar, tag=""):
    """(c) Each shard's f32 buffer behind the first products phase: pairs(a, b) returns the float64 (F_local^T D_local,
    F_local^T F_local) of the rows [a, b); compared with mur_step.compare at `bar`; rows and columns of the padding exactly zero."""
    fails = []
    for i, (x, lay) in enumerate(zip(snaps, layouts)):
        a, b = cuts[i], cuts[i + 1]
        kp, np_ = lay["kp"], lay["np"]
        who = f"{tag}rank {i} (rows {a} .. {b - 1}) "
        prod = x[:kp * np_].reshape(kp, np_)
        gram = x[lay["g"]:lay["g"] + kp * kp].reshape(kp, kp)
        pad = int(np.count_nonzero(prod[k:])) + int(np.count_nonzero(prod[:k, n:])) + int(np.count_nonzero(gram[k:])) + int(np.count_nonzero(gram[:k, k:]))
        if pad:
            fails.append(f"{who}partial: {pad} elements of the padded factors / columns are not zero")
        want_b, want_g = pairs(a, b)
        for name, got, want in (("F^T D", prod[:k, :n], want_b), ("F^T F", gram[:k, :k], want_g)):
            _, msg = S.compare(who + name, got, want, bar)
            if msg:
                fails.append(msg)
    return fails


def nan_failures(named):
    """(d) named: [(label, array or None)]."""
    return [f"{label}: {int(np.sum(~np.isfinite(a)))} values are not finite" for label, a in named if a is not None and not np.all(np.isfinite(a))]


def family_common_failures(run, bar_partials):
    """(a) - (d) of a FamilyRun; returns the list of failures."""
    c = run.case
    v, w0, h0 = A.make_case(c)
    fails = list(family_ranks_differ(run))
    fails += objective_sum_failures(run.partials, run.objs[0])
    if c.family == "ao":
        fails += norm_decision_failures(run)
    vv = np.asarray(v, dtype=np.float64)

    def pairs(a, b):
        f = w0[a:b]                                     # (ADMM: w_aux = w at the start, admm.py:27)
        d = vv[a:b] if c.loss == "eu" else np.zeros_like(vv[a:b])         # (KL: S = v_aux + dual_v = 0 at the start)
        return f.T @ d, f.T @ f

    if run.snaps is not None:
        fails += partial_failures(run.snaps, run.layouts, run.cuts, c.k, c.n, pairs, bar_partials)
    named = []
    for s, states in enumerate(run.rank_states, start=1):
        for i, st in enumerate(states):
            named += [(f"step {s}, rank {i}: {name}", getattr(st, name)) for name in ("w", "h", "w_aux", "h_aux", "dual_w", "dual_h")]
    named += [(f"objective history of rank {i}", o) for i, o in enumerate(run.objs)]
    return fails + nan_failures(named)


def anls_common_failures(out, c, bar_partials):
    v, w0, h0 = N.make_case(c.regime, c.m, c.n, c.k)
    fails = list(anls_ranks_differ(out))
    for s in sorted(out.runs):
        fails += objective_sum_failures(out.partials[s], out.objs[s][0], tag=f"{s}-step run: ")
    vv = np.asarray(v, dtype=np.float64)

    def pairs(a, b):
        f = out.w_mid[a:b]
        return f.T @ vv[a:b], f.T @ f

    if out.snaps is not None and np.all(np.isfinite(out.w_mid)):
        fails += partial_failures(out.snaps, out.layouts, out.cuts, c.k, c.n, pairs, bar_partials)
    named = [("W after anls_phase_w", out.w_mid)]
    for s, r in sorted(out.runs.items()):
        named += [(f"{s}-step run: W", r.w)] + [(f"{s}-step run: H of rank {i}", h) for i, h in enumerate(out.hs[s])]
        named += [(f"{s}-step run: objectives of rank {i}", o) for i, o in enumerate(out.objs[s])]
    return fails + nan_failures(named)


# ---- where a shard's own norm sums would stop the W sub-problem (the precondition of the local-stop case) -------------------------
# found by a search over lambda and the number of warm steps on the CPU (tests/test_shard_family_bars.py proves what it is for): the
# sums over all 70 rows stop the first W sub-problem at round 7, those of rows [0, 7) or [41, 70) alone at round 6
LOCAL_STOP_CASE = A._ao("eu", 70, 60, 16, "f32", 10, ("l1n", 0.7, "l1n", 0.7), warm=3)
LOCAL_STOP_CUTS = [0, 7, 41, 70]
# ADMM with the row-coupled l1inf operators on the H side alone (replicated work; on W they are not available row-sharded, and
# admm_step.CASES pairs them): tests/test_shard_family_bars.py proves their bars like tests/test_admm_step_bars.py the table's
ADMM_L1INF_CASES = (A._admm("eu", 257, 200, 12, "f32", 1.0, ("l1n", 0.05, "l1inf", 0.05), edges=True),
                    A._admm("eu", 257, 200, 40, "bf16", 1.0, ("l1n", 0.05, "l1inf_transpose", 0.05), edges=True))


def w_stop_rounds(c, cuts):
    """Step 1 of a Euclidean AO-ADMM case in float64: (the round at which the W sub-problem stops on the sums over ALL rows, [the
    round at which each shard's own sums alone would stop it], the smallest |ratio / tolerance - 1| any of these decisions met);
    admm_iter + 1 = no stop within admm_iter.  The rounds themselves
    are row-local given H and rho, so the local question is the global trajectory's sums restricted to the shard's rows."""
    import scipy.linalg as sla
    from oracle import nmf_ref as R
    v, w0, h0 = A.make_case(c)
    vv = np.asarray(v, dtype=np.float64)
    h1 = A.ref_block(w0, vv, h0, np.zeros_like(h0), c.k, c.prox_h, c.lam_h, c.admm_iter).x
    f, d = np.ascontiguousarray(h1.T), np.ascontiguousarray(vv.T)
    g = f.T @ f
    rho = np.trace(g) / c.k
    chol = sla.cholesky(g + rho * np.eye(c.k), lower=True)
    b = f.T @ d
    x, dual = w0.T.copy(), np.zeros_like(w0.T)
    groups = [slice(0, c.m)] + [slice(a, e) for a, e in zip(cuts[:-1], cuts[1:])]
    first = [c.admm_iter + 1] * len(groups)
    clear = np.inf
    for j in range(c.admm_iter):
        aux = sla.cho_solve((chol, True), b + rho * (x + dual))
        prev = x
        x = R.prox(c.prox_w, aux, dual, rho=rho, lam=c.lam_w, ragged_raises=False)
        dual = dual + x - aux
        for t, rows in enumerate(groups):
            if first[t] > c.admm_iter:
                ratios = R.inner_residuals(x[:, rows], prev[:, rows], aux[:, rows], dual[:, rows])
                clear = min([clear] + [abs(r / A.STOP_TOL - 1.0) for r in ratios if np.isfinite(r)])
                if all(r < A.STOP_TOL for r in ratios):
                    first[t] = j + 1
    return first[0], first[1:], clear
