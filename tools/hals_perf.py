"""Time a HALS iteration beside an ANLS iteration, the share of the sweep kernel, and HALS against MUR to a common objective.

    python tools/hals_perf.py                              # 16384 x 8192, k = 64 and 128, writes profiles/hals_perf.txt
    python tools/hals_perf.py --m 2048 --n 1024 --ks 40

Per rank, on one seeded planted matrix and one seeded uniform start, in the default arithmetic:
  1. ms per `hals` iteration (sweeps = 1) and per `anls` iteration: two handles in one process, a warm-up batch each, then
     --reps rounds of one batch of --iters iterations each, alternated, a host clock around a device synchronise; median with
     the smallest and the largest round.  `anls` is code HALS does not touch beyond the shared plumbing: it is the yardstick.
  2. the share of `hals_sweep` (nmfx_profile_get, device events, a run of its own) in a HALS iteration.
  3. the objective `mur` ('eu') reaches after --mur-iters iterations, and the iterations and wall time at which `hals`
     (from the rescaled start, the rescale timed with it) and `mur` each first record an objective at or below it."""
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


def clocked(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return time.perf_counter() - t0


def measure(m, n, k, iters, reps, mur_iters, say):
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    from nmf_amd.hals import start_scale
    from nmf_amd.synth import planted_matrix
    v = planted_matrix(m, n, k, seed=0, dtype=np.float32)
    rs = np.random.RandomState(0)
    w0, h0 = rs.rand(m, k), rs.rand(k, n)
    legs = {}
    for name in ("hals", "anls"):
        e = Engine(m, n, k)
        e.upload_v(v)
        e.set_factors(w0, h0)
        legs[name] = e
    arith = legs["hals"].precision()
    run = {"hals": lambda f, c: legs["hals"].hals_run(0.0, 0.0, 1, NEVER, 1e-30, 1e-30, f, c),
           "anls": lambda f, c: legs["anls"].anls_run(0.0, 0.0, NEVER, 1e-30, 1e-30, f, c)}
    done, ms = {}, {"hals": [], "anls": []}
    for name in legs:                                            # warm-up batch
        clocked(legs[name], lambda: run[name](0, iters))
        done[name] = iters
    for _ in range(reps):
        for name in legs:
            ms[name].append(1e3 * clocked(legs[name], lambda: run[name](done[name], iters)) / iters)
            done[name] += iters
    say(f"{m} x {n}, k = {k}, {arith} arithmetic, {reps} rounds of {iters} iterations after a warm-up batch")
    for name in ("hals", "anls"):
        t = ms[name]
        say(f"  {name:5s} ms per iteration: median {statistics.median(t):.3f}  (min {min(t):.3f}, max {max(t):.3f})")
    med = {name: statistics.median(t) for name, t in ms.items()}
    spread = max(ms["anls"]) - min(ms["anls"])
    say(f"  hals - anls = {med['hals'] - med['anls']:+.3f} ms; spread of the anls rounds {spread:.3f} ms")
    legs["anls"].close()

    e = legs["hals"]                                             # the share of the sweep kernel: a run of its own
    e.profile_enable(True)
    e.profile_reset()
    wall = 1e3 * clocked(e, lambda: run["hals"](done["hals"], iters)) / iters
    sweep_ms, launches = e.profile_get("hals_sweep")
    e.profile_enable(False)
    per_iter = sweep_ms / iters
    say(f"  hals_sweep: {launches} launches in {iters} iterations, {per_iter:.4f} ms per iteration (both half-steps) = "
        f"{100 * per_iter / med['hals']:.1f} % of the unprofiled iteration ({wall:.3f} ms per iteration with the events on)")
    say(f"  bytes the sweeps touch, 3 (m + n) k 4: {3 * (m + n) * k * 4 / 1e6:.1f} MB; two passes over V: {2 * m * n * 4 / 1e6:.0f} MB")

    mur = Engine(m, n, k)                                        # to a common objective
    mur.upload_v(v)
    mur.set_factors(w0, h0)
    clocked(mur, lambda: mur.mur_run(L.EU, 0.0, 0.0, NEVER, 1e-30, 1e-30, 0, 2))
    mur.set_factors(w0, h0)
    t_mur = clocked(mur, lambda: mur.mur_run(L.EU, 0.0, 0.0, NEVER, 1e-30, 1e-30, 0, mur_iters))
    mur.mur_finish(L.EU, NEVER, 1e-30, 1e-30, mur_iters)
    obj_mur = mur.objectives(0, mur_iters + 1)
    target = float(obj_mur[mur_iters])
    first_mur = int(np.argmax(obj_mur <= target))
    mur.close()
    box = []
    t_scale = clocked(e, lambda: box.append(start_scale(e, w0, h0)))
    alpha = box[0]
    e.set_factors(w0 * np.sqrt(alpha), h0 * np.sqrt(alpha))
    e.anls_set_distance(L.EU)
    t_hals, n_done, first_hals = 0.0, 0, None
    while first_hals is None and n_done < mur_iters:
        t_hals += clocked(e, lambda: run["hals"](n_done, 10))
        n_done += 10
        obj = e.objectives(0, n_done)                            # (obj[t] is recorded when iteration t starts)
        if (obj <= target).any():
            first_hals = int(np.argmax(obj <= target))
    say(f"  mur 'eu' after {mur_iters} iterations: objective {target:.6g} ({1e3 * t_mur / mur_iters:.3f} ms per iteration); first at or below it: "
        f"iteration {first_mur}, {t_mur * first_mur / mur_iters:.3f} s")
    if first_hals is None:
        say(f"  hals: not reached in {n_done} iterations (objective {obj[-1]:.6g})")
    else:
        say(f"  hals (start scale alpha = {alpha:.4g}, {1e3 * t_scale:.1f} ms): first at or below it after {first_hals} iterations, "
            f"{t_scale + t_hals * first_hals / n_done:.3f} s ({1e3 * t_hals / n_done:.3f} ms per iteration)")
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mur-iters", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hals_perf.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for k in [int(s) for s in a.ks.split(",")]:
        measure(a.m, a.n, k, a.iters, a.reps, a.mur_iters, say)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
