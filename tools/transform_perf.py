"""Time one fold-in step (nmfx_foldin_run: one pass over V) beside one MUR iteration of the same loss (two passes).

    python tools/transform_perf.py                       # 16384 x 8192, k = 64
    python tools/transform_perf.py --m 2048 --n 1024

On one seeded strictly positive matrix, ms per step / per iteration of
    'kl' under NMFX_PRECISION=f32      fold-in: the PlainEntry<KL> policy;   mur: the exact-f32 KL path
    'is'                               fold-in and mur: the IsEntry policy
    'beta' at beta = 0.5               fold-in and mur: the BetaEntry policy
`mur` is code that fold-in does not touch: it is the comparator.  All six legs run in one process on one stream, alternated:
a warm-up batch each, then --reps rounds of one batch of --iters steps each between device events; the best round counts.
One JSON line; foldin_over_mur is the ratio per loss."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NMF_AMD_QUIET", "1")
os.environ["NMFX_PRECISION"] = "f32"

import numpy as np

NEVER = 10 ** 12


def timed(eng, foldin, dist, first, count, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if foldin:
        eng.foldin_run(dist, 0.0, NEVER, 1e-30, 1e-30, first, count)
    else:
        eng.mur_run(dist, 0.0, 0.0, NEVER, 1e-30, 1e-30, first, count)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import torch
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    rng = np.random.default_rng(a.seed)
    v = (rng.random((a.m, 16), dtype=np.float32) @ rng.random((16, a.n), dtype=np.float32)) / 16 + np.float32(0.01)
    w0 = np.ascontiguousarray(rng.uniform(0.1, 1.0, (a.m, a.k)))
    h0 = np.ascontiguousarray(rng.uniform(0.1, 1.0, (a.k, a.n)))
    stream = torch.cuda.current_stream().cuda_stream

    def engine(beta=None):
        e = Engine(a.m, a.n, a.k)
        e.set_stream(stream)
        e.upload_v(v)
        if beta is not None:
            e.set_beta(beta)
        return e

    losses = {"kl_f32": (L.KL, None), "is": (L.IS, None), f"beta_{a.beta:g}": (L.BETA, a.beta)}
    legs = {}                                                    # name -> (engine, fold-in?, distance)
    for loss, (dist, beta) in losses.items():
        legs[f"foldin_{loss}"] = (engine(beta), True, dist)
        legs[f"mur_{loss}"] = (engine(beta), False, dist)
    assert legs["mur_kl_f32"][0].precision() == "f32"
    ms = {name: [] for name in legs}
    done = {}
    for name, (eng, foldin, dist) in legs.items():               # fresh start, warm-up batch
        eng.set_factors(w0, h0)
        timed(eng, foldin, dist, 0, a.iters, torch)
        done[name] = a.iters
    for _ in range(a.reps):
        for name, (eng, foldin, dist) in legs.items():
            ms[name].append(timed(eng, foldin, dist, done[name], a.iters, torch))
            done[name] += a.iters
    for name, (eng, _, _) in legs.items():
        assert eng.state()[0] == 0, f"{name}: the stop rule fired during timing"
    best = {name: min(t) for name, t in ms.items()}
    out = {"m": a.m, "n": a.n, "k": a.k, "iters_per_batch": a.iters}
    out.update({f"{name}_ms": round(t, 4) for name, t in best.items()})
    out["foldin_over_mur"] = {loss: round(best[f"foldin_{loss}"] / best[f"mur_{loss}"], 3) for loss in losses}
    out["all_ms"] = {name: [round(t, 4) for t in ts] for name, ts in ms.items()}
    print(json.dumps(out), flush=True)
    for eng, _, _ in legs.values():
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
