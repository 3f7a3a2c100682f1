"""Time one MUR iteration with the beta-divergence (kernels_phase.hip, BetaEntry) beside the two kernels it generalises.

    python tools/beta_perf.py                       # 16384 x 8192, k = 64
    python tools/beta_perf.py --m 2048 --n 1024
    python tools/beta_perf.py --ard                 # beta = 0.5 with and without automatic relevance determination

On one seeded strictly positive matrix, ms per iteration of
    (a) 'beta' at beta = 0.5 and 1.5     the BetaEntry policy of kernels_phase.hip
    (b) 'is'                             its IsEntry policy: the same kernel without the power
    (c) 'kl' under NMFX_PRECISION=f32    the exact-f32 KL path
All four run in one process on one stream, alternated: a warm-up batch each, then --reps rounds of one batch of --iters
iterations each between device events; the best round counts.  One JSON line.

--ard times two legs only, 'beta' at beta = 0.5 plain and with nmfx_set_ard (phi = 0.1, a = 5, the default b), the same way:
what the per-component penalty and the relevance reduction (two small launches per iteration, (m + n) kp 4 bytes read
against V's m n 4) add to an iteration."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NMF_AMD_QUIET", "1")
os.environ["NMFX_PRECISION"] = "f32"

import numpy as np

NEVER = 10 ** 12


def timed(eng, dist, first, count, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    eng.mur_run(dist, 0.0, 0.0, NEVER, 1e-30, 1e-30, first, count)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--betas", type=float, nargs="+", default=[0.5, 1.5])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ard", action="store_true", help="time beta = 0.5 with and without ARD instead of the four legs")
    a = ap.parse_args()

    import torch
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    rng = np.random.default_rng(a.seed)
    v = (rng.random((a.m, 16), dtype=np.float32) @ rng.random((16, a.n), dtype=np.float32)) / 16 + np.float32(0.01)
    w0 = np.ascontiguousarray(rng.uniform(0.1, 1.0, (a.m, a.k)))
    h0 = np.ascontiguousarray(rng.uniform(0.1, 1.0, (a.k, a.n)))
    stream = torch.cuda.current_stream().cuda_stream

    def engine(beta=None, ard=False):
        e = Engine(a.m, a.n, a.k)
        e.set_stream(stream)
        e.upload_v(v)
        if beta is not None:
            e.set_beta(beta)
        if ard:
            e.set_ard(0.1, 5.0, float(np.sqrt(12.0 * float(v.mean(dtype=np.float64)) / a.k)))
        return e

    if a.ard:
        legs = {"beta_0.5": (engine(0.5), L.BETA), "ard_0.5": (engine(0.5, ard=True), L.BETA)}
    else:
        legs = {f"beta_{b:g}": (engine(b), L.BETA) for b in a.betas}
        legs["is"] = (engine(), L.IS)
        legs["kl_f32"] = (engine(), L.KL)
        assert legs["kl_f32"][0].precision() == "f32"
    ms = {name: [] for name in legs}
    done = {}
    for name, (eng, dist) in legs.items():                      # fresh start, warm-up batch
        eng.set_factors(w0, h0)
        timed(eng, dist, 0, a.iters, torch)
        done[name] = a.iters
    for _ in range(a.reps):
        for name, (eng, dist) in legs.items():
            ms[name].append(timed(eng, dist, done[name], a.iters, torch))
            done[name] += a.iters
    for name, (eng, _) in legs.items():
        assert eng.state()[0] == 0, f"{name}: the stop rule fired during timing"
    best = {name: min(t) for name, t in ms.items()}
    out = {"m": a.m, "n": a.n, "k": a.k, "iters_per_batch": a.iters}
    out.update({f"{name}_ms_per_iter": round(t, 4) for name, t in best.items()})
    if a.ard:
        out["ard_over_beta"] = round(best["ard_0.5"] / best["beta_0.5"], 4)
        out["ard_extra_ms_per_iter"] = round(best["ard_0.5"] - best["beta_0.5"], 4)
    else:
        out.update({f"{name}_over_is": round(best[name] / best["is"], 3) for name in best if name.startswith("beta_")})
    out["all_ms"] = {name: [round(t, 4) for t in ts] for name, ts in ms.items()}
    print(json.dumps(out), flush=True)
    for eng, _ in legs.values():
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
