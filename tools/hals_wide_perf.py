"""Time a HALS iteration beyond 128 components beside an ANLS iteration, the two sweep launches, and hals_wide against MUR to a
common objective.

    python tools/hals_wide_perf.py                            # 16384 x 8192, k = 256, 512, 1024, writes profiles/hals_wide_perf.txt
    python tools/hals_wide_perf.py --m 2048 --n 1024 --ks 200

Per rank, on one seeded planted matrix and one seeded uniform start:
  1. in both arithmetic modes (split bf16, exact f32), ms per `hals_wide` iteration (sweeps = 1) and per `anls` iteration: a
     warm-up batch each, then --reps rounds of one batch of --iters iterations each, alternated, a host clock around a device
     synchronise; median with the smallest and the largest round.  `anls` beyond 128 components is code this solver shares only the
     products with: it is the yardstick.  Its exact solve is a float64 Cholesky per right-hand side and active-set round, whose
     cost grows with k^3: a full-size run is made only where a probe on 1/8 of the rows and columns (the solves scale with m + n)
     predicts at most --anls-budget seconds per iteration, and the probe's figure times 8 is printed, marked, otherwise.
  2. the `hals_sweep_w` / `hals_sweep_h` scopes (nmfx_profile_get, device events, a run of its own) of a hals_wide iteration, and
     the bytes of G each streams through LDS.
  3. in the default mode, the objective `mur` ('eu') reaches after --mur-iters iterations, and the iterations and wall time at
     which `hals_wide` (from the rescaled start, the rescale timed with it) first records an objective at or below it."""
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
WAVES, BLOCKS_PER_CU = 8, 2          # NMFX_HALS_WAVES, NMFX_HALS_BLOCKS_PER_CU (csrc/kernels_hals.hip)


def clocked(eng, fn):
    eng.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.synchronize()
    return time.perf_counter() - t0


def handle(v, w0, h0, mode):
    from nmf_amd.engine import Engine
    e = Engine(v.shape[0], v.shape[1], w0.shape[1])
    if mode == "f32":
        e.set_precision("f32")
    e.upload_v(v)
    e.set_factors(w0, h0)
    return e


def anls_probe(v, w0, h0, mode, div):
    """Seconds of one anls iteration (the second of two) on the leading 1/div of the rows and columns."""
    m, n = v.shape[0] // div, v.shape[1] // div
    e = handle(np.ascontiguousarray(v[:m, :n]), w0[:m], h0[:, :n], mode)
    clocked(e, lambda: e.anls_run(0.0, 0.0, NEVER, 1e-30, 1e-30, 0, 1))
    t = clocked(e, lambda: e.anls_run(0.0, 0.0, NEVER, 1e-30, 1e-30, 1, 1))
    e.close()
    return t


def stream_bytes(nprob, kp, ncu, sweeps=1):
    """Bytes of G one sweep launch stages into LDS: every block restages all kp x kp floats once for the mat-vec and once per
    sweep, on each of its trips."""
    blocks = min(-(-nprob // WAVES), ncu * BLOCKS_PER_CU)
    trips = -(-nprob // (blocks * WAVES))
    return blocks * trips * (1 + sweeps) * kp * kp * 4


def measure(m, n, k, iters, reps, mur_iters, anls_budget, say):
    from nmf_amd import _lib as L
    from nmf_amd.hals import start_scale
    from nmf_amd.synth import planted_matrix
    v = planted_matrix(m, n, k, seed=0, dtype=np.float32)
    rs = np.random.RandomState(0)
    w0, h0 = rs.rand(m, k), rs.rand(k, n)
    kp = -(-k // 128) * 128
    for mode in ("bf16", "f32"):
        e = handle(v, w0, h0, mode)
        run = lambda f, c: e.hals_wide_run(0.0, 0.0, 1, NEVER, 1e-30, 1e-30, f, c)
        say(f"{m} x {n}, k = {k}, {'split-bf16' if mode == 'bf16' else 'exact-f32'} products, {reps} rounds of {iters} iterations after a warm-up batch")
        # anls: probes first, the full size only within the budget
        est, full = None, None
        for div in (64, 8):
            t = anls_probe(v, w0, h0, mode, div)
            est = (t * div, div)
            if t * (8 if div == 64 else div) > anls_budget:
                break
        else:
            full = handle(v, w0, h0, mode)
        ms = {"hals_wide": [], "anls": []}
        clocked(e, lambda: run(0, iters))
        done = {"hals_wide": iters, "anls": 0}
        if full is not None:
            clocked(full, lambda: full.anls_run(0.0, 0.0, NEVER, 1e-30, 1e-30, 0, 2))
            done["anls"] = 2
        a_iters = max(1, min(iters, int(anls_budget / max(est[0], 1e-3))))
        for _ in range(reps):
            ms["hals_wide"].append(1e3 * clocked(e, lambda: run(done["hals_wide"], iters)) / iters)
            done["hals_wide"] += iters
            if full is not None:
                ms["anls"].append(1e3 * clocked(full, lambda: full.anls_run(0.0, 0.0, NEVER, 1e-30, 1e-30, done["anls"], a_iters)) / a_iters)
                done["anls"] += a_iters
        t = ms["hals_wide"]
        med = statistics.median(t)
        say(f"  hals_wide ms per iteration: median {med:.3f}  (min {min(t):.3f}, max {max(t):.3f})")
        if full is not None:
            t = ms["anls"]
            say(f"  anls      ms per iteration: median {statistics.median(t):.3f}  (min {min(t):.3f}, max {max(t):.3f}; batches of {a_iters}); "
                f"hals_wide / anls = {med / statistics.median(t):.3f}")
            full.close()
        else:
            say(f"  anls      ms per iteration: about {1e3 * est[0]:.0f}, NOT run at full size: {est[1]} x the second iteration on the leading "
                f"1/{est[1]} of the rows and columns ({1e3 * est[0] / est[1]:.1f} ms), above the budget of {anls_budget:.0f} s per iteration; "
                f"hals_wide / anls about {med / (1e3 * est[0]):.4f}")
        e.profile_enable(True)
        e.profile_reset()
        wall = 1e3 * clocked(e, lambda: run(done["hals_wide"], iters)) / iters
        done["hals_wide"] += iters
        sw, lw_ = e.profile_get("hals_sweep_w")
        sh, lh_ = e.profile_get("hals_sweep_h")
        e.profile_enable(False)
        ncu = 256
        for name, t_ms, launches, nprob in (("hals_sweep_w", sw, lw_, m), ("hals_sweep_h", sh, lh_, n)):
            gb = stream_bytes(nprob, kp, ncu) / 1e9
            say(f"  {name}: {launches} launches in {iters} iterations, {t_ms / iters:.4f} ms per iteration = {100 * t_ms / iters / med:.1f} % of "
                f"the unprofiled iteration; G through LDS {gb:.2f} GB per launch ({gb / (t_ms / iters / 1e3) / 1e3:.2f} TB/s)")
        say(f"  ({wall:.3f} ms per iteration with the events on)")
        if mode != "bf16":
            e.close()
            continue
        mur = handle(v, w0, h0, mode)                                # to a common objective, default mode
        clocked(mur, lambda: mur.mur_run(L.EU, 0.0, 0.0, NEVER, 1e-30, 1e-30, 0, 2))
        mur.set_factors(w0, h0)
        t_mur = clocked(mur, lambda: mur.mur_run(L.EU, 0.0, 0.0, NEVER, 1e-30, 1e-30, 0, mur_iters))
        mur.mur_finish(L.EU, NEVER, 1e-30, 1e-30, mur_iters)
        target = float(mur.objectives(0, mur_iters + 1)[mur_iters])
        mur.close()
        box = []
        t_scale = clocked(e, lambda: box.append(start_scale(e, w0, h0)))
        alpha = box[0]
        e.set_factors(w0 * np.sqrt(alpha), h0 * np.sqrt(alpha))
        e.anls_set_distance(L.EU)
        t_h, n_done, first = 0.0, 0, None
        while first is None and n_done < mur_iters:
            t_h += clocked(e, lambda: run(n_done, 8))
            n_done += 8
            obj = e.objectives(0, n_done)                            # (obj[t] is recorded when iteration t starts)
            if (obj <= target).any():
                first = int(np.argmax(obj <= target))
        say(f"  mur 'eu' after {mur_iters} iterations: objective {target:.6g} ({1e3 * t_mur / mur_iters:.3f} ms per iteration, {t_mur:.3f} s)")
        if first is None:
            say(f"  hals_wide: not reached in {n_done} iterations (objective {obj[-1]:.6g})")
        else:
            say(f"  hals_wide (start scale alpha = {alpha:.4g}, {1e3 * t_scale:.1f} ms): first at or below it after {first} iterations, "
                f"{t_scale + t_h * first / n_done:.3f} s ({1e3 * t_h / n_done:.3f} ms per iteration)")
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--ks", default="256,512,1024")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mur-iters", type=int, default=500)
    ap.add_argument("--anls-budget", type=float, default=2.0, help="seconds per anls iteration a full-size run may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hals_wide_perf.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(a.out, "w") as fh:                                 # (kept current: a long run leaves what it has measured)
            fh.write("\n".join(lines) + "\n")
    for k in [int(s) for s in a.ks.split(",")]:
        measure(a.m, a.n, k, a.iters, a.reps, a.mur_iters, a.anls_budget, say)


if __name__ == "__main__":
    main()
