"""Time an iteration of stacked HALS beside the same problems run one after another with `hals`.

    python tools/hals_stack_perf.py                        # 16384 x 8192, writes profiles/hals_stack_perf.txt
    python tools/hals_stack_perf.py --m 2048 --n 1024

The method of tools/hals_perf.py: one seeded planted matrix, seeded uniform starts, the default arithmetic; every handle gets a
warm-up batch, then --reps rounds of one batch of --iters iterations each, the handles alternated, a host clock around a device
synchronise; the median of the rounds with the smallest and the largest.  Per stack:
  1. ms per iteration of the stack (nmfx_hals_stack_run on a handle of k = the sum of the ranks, sweeps = 1, stop rule off);
  2. ms per iteration of nmfx_hals_run at every rank of the stack on a handle of that rank, and their sum over the problems:
     what the problems cost one after another;
  3. the shares of `hals_sweep` and of `stack_objective` (the five launches that form the objectives; nmfx_profile_get, device
     events, a run of its own) in a stack iteration."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("NMF_AMD_QUIET", "1")

import numpy as np

NEVER = 10 ** 12
STACKS = [("8 x k = 8", (8,) * 8), ("k = 2 .. 15", tuple(range(2, 16))), ("16 x k = 8", (8,) * 16)]


def clocked(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return time.perf_counter() - t0


def measure(v, name, ks, singles, iters, reps, say):
    from nmf_amd.engine import Engine
    m, n = v.shape
    total = sum(ks)
    rs = np.random.RandomState(0)
    legs, run, done, ms = {}, {}, {}, {}
    st = Engine(m, n, total)
    st.upload_v(v)
    st.set_factors(rs.rand(m, total), rs.rand(total, n))
    st.hals_stack_set(ks)
    zeros = [0.0] * len(ks)
    legs["stack"] = st
    run["stack"] = lambda f, c: st.hals_stack_run(zeros, zeros, 1, NEVER, 1e-30, 1e-30, f, c)
    for k in sorted(set(ks)):
        if k not in singles:
            e = Engine(m, n, k)
            e.upload_v(v)
            singles[k] = e
        singles[k].set_factors(rs.rand(m, k), rs.rand(k, n))
        legs[k] = singles[k]
        run[k] = (lambda e: lambda f, c: e.hals_run(0.0, 0.0, 1, NEVER, 1e-30, 1e-30, f, c))(singles[k])
    for key in legs:                                             # warm-up batch
        clocked(legs[key], lambda: run[key](0, iters))
        done[key], ms[key] = iters, []
    for _ in range(reps):
        for key in legs:
            ms[key].append(1e3 * clocked(legs[key], lambda: run[key](done[key], iters)) / iters)
            done[key] += iters
    med = {key: statistics.median(t) for key, t in ms.items()}
    say(f"{m} x {n}, stack {name} (sum k = {total}, {len(ks)} problems), {st.precision()} arithmetic, {reps} rounds of {iters} iterations after a warm-up batch")
    t = ms["stack"]
    say(f"  stack ms per iteration: median {med['stack']:.3f}  (min {min(t):.3f}, max {max(t):.3f})")
    for k in sorted(set(ks)):
        t = ms[k]
        say(f"  hals k = {k:3d} ({legs[k].precision()}) ms per iteration: median {med[k]:.3f}  (min {min(t):.3f}, max {max(t):.3f})")
    one_by_one = sum(med[k] for k in ks)
    say(f"  the problems one after another: {one_by_one:.3f} ms per iteration of all; stack / one after another = {med['stack'] / one_by_one:.3f} "
        f"({'the stack costs less' if med['stack'] < one_by_one else 'THE STACK DOES NOT COST LESS'})")
    st.profile_enable(True)
    st.profile_reset()
    wall = 1e3 * clocked(st, lambda: run["stack"](done["stack"], iters)) / iters
    sweep_ms, _ = st.profile_get("hals_sweep")
    obj_ms, _ = st.profile_get("stack_objective")
    st.profile_enable(False)
    say(f"  hals_sweep {sweep_ms / iters:.4f} ms per iteration (both half-steps) = {100 * sweep_ms / iters / med['stack']:.1f} %, stack_objective "
        f"{obj_ms / iters:.4f} ms = {100 * obj_ms / iters / med['stack']:.1f} % of the unprofiled iteration ({wall:.3f} ms per iteration with the events on)")
    st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hals_stack_perf.txt"))
    a = ap.parse_args()
    from nmf_amd.synth import planted_matrix
    v = planted_matrix(a.m, a.n, 16, seed=0, dtype=np.float32)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    singles = {}
    for name, ks in STACKS:
        measure(v, name, ks, singles, a.iters, a.reps, say)
    for e in singles.values():
        e.close()
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
