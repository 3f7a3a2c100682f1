"""Time one MUR iteration with per-entry weights (kernels_phase.hip, WtEntry) beside the two paths it sits between.

    python tools/weighted_perf.py                       # 16384 x 8192, k = 64, 10 % / 50 % / 90 % observed, eu and kl
    python tools/weighted_perf.py --m 2048 --n 1024 --fractions 0.5

On one seeded matrix and a seeded 0 / 1 pattern per observed fraction, ms per iteration of
    (a) weights=   the weighted dense path (0 / 1 weights: the pattern)
    (b) mask=      the masked sparse path on the same pattern (kernels_sparse.hip)
    (c) dense      the unweighted dense path under NMFX_PRECISION=f32 (the pattern plays no part)
All three run in one process on one stream, alternated: a warm-up batch each, then --reps rounds of one batch of --iters
iterations each between device events; the best round counts.  One JSON line per (fraction, loss)."""
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
    ap.add_argument("--fractions", type=float, nargs="+", default=[0.1, 0.5, 0.9])
    ap.add_argument("--losses", nargs="+", default=["eu", "kl"], choices=["eu", "kl", "is"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    import torch
    from nmf_amd import _lib as L
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    code = {"eu": L.EU, "kl": L.KL, "is": L.IS}
    rng = np.random.default_rng(a.seed)
    v = (rng.random((a.m, 16), dtype=np.float32) @ rng.random((16, a.n), dtype=np.float32)) / 16 + np.float32(0.01)
    w0 = np.ascontiguousarray(rng.uniform(0.1, 1.0, (a.m, a.k)))
    h0 = np.ascontiguousarray(rng.uniform(0.1, 1.0, (a.k, a.n)))
    stream = torch.cuda.current_stream().cuda_stream

    def dense_engine():
        e = Engine(a.m, a.n, a.k)
        e.set_stream(stream)
        e.upload_v(v)
        return e

    plain = dense_engine()
    assert plain.precision() == "f32"
    wt = dense_engine()
    for frac in a.fractions:
        pattern = np.random.default_rng(a.seed + 1 + int(round(frac * 1000))).random((a.m, a.n), dtype=np.float32) < frac
        wt.upload_weights(pattern.astype(np.float32))
        sparse_eng = Engine.for_sparse(masked.observed(v, pattern, a.k), a.k, masked=True)
        sparse_eng.set_stream(stream)
        legs = {"weights": wt, "mask": sparse_eng, "dense_f32": plain}
        for loss in a.losses:
            dist = code[loss]
            ms = {name: [] for name in legs}
            done = {}
            for name, eng in legs.items():                      # fresh start, warm-up batch
                eng.set_factors(w0, h0)
                timed(eng, dist, 0, a.iters, torch)
                done[name] = a.iters
            for _ in range(a.reps):
                for name, eng in legs.items():
                    ms[name].append(timed(eng, dist, done[name], a.iters, torch))
                    done[name] += a.iters
            for name, eng in legs.items():
                assert eng.state()[0] == 0, f"{name}: the stop rule fired during timing"
            best = {name: min(t) for name, t in ms.items()}
            print(json.dumps({"m": a.m, "n": a.n, "k": a.k, "observed": frac, "loss": loss, "iters_per_batch": a.iters,
                              "weights_ms_per_iter": round(best["weights"], 4), "mask_ms_per_iter": round(best["mask"], 4),
                              "dense_f32_ms_per_iter": round(best["dense_f32"], 4),
                              "weights_over_dense": round(best["weights"] / best["dense_f32"], 3),
                              "weights_over_mask": round(best["weights"] / best["mask"], 3),
                              "all_ms": {name: [round(t, 4) for t in ts] for name, ts in ms.items()}}), flush=True)
        sparse_eng.reset_stream()
        sparse_eng.close()
    for eng in (plain, wt):
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
