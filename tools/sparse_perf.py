"""Time nmfx_mur_run on sparse V (kernels_sparse.hip) with device events, beside the dense path on the same matrix.

    python tools/sparse_perf.py --m 16384 --n 8192 --density 0.01 --k 64 --dist eu
    python tools/sparse_perf.py --m 16384 --n 8192 --density 0.01 --k 64 --dist kl --powerlaw 1.1
    python tools/sparse_perf.py --m 16384 --n 8192 --density 0.10 --k 64 --dist eu --masked

Inputs are seeded random CSR (uniform column positions; --powerlaw a: row lengths proportional to rank^-a, shuffled).
One JSON line per case: ms per iteration over a warmed batch, nnz, the bytes the algorithm must move per iteration
(both index streams, the gathered factor rows, the factors and their Grams' reads), the GB/s that makes, and -- where
V fits densely (--dense-max-gib) -- the dense path's ms per iteration on the same matrix, measured alternately with the
sparse one in the same process.  --masked: a masked handle on the same stored pattern (the stored entries as the observed
set, nmfx_set_masked) timed alternately with the unmasked one ("masked_ms_per_iter"; dense leg skipped)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NMF_AMD_QUIET", "1")

import numpy as np
import scipy.sparse as sp


def make_csr(m, n, density, seed, powerlaw):
    rng = np.random.default_rng(seed)
    nnz = int(round(m * n * density))
    if powerlaw:
        p = np.arange(1, m + 1, dtype=np.float64) ** -powerlaw
        rows = rng.choice(m, size=nnz, p=rng.permutation(p / p.sum()))
    else:
        rows = rng.integers(0, m, nnz)
    cols = rng.integers(0, n, nnz)
    vals = rng.uniform(0.1, 1.0, nnz).astype(np.float32)
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, n))


def timed(eng, dist, first, count, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    eng.mur_run(dist, 0.0, 0.0, 10 ** 12, 1e-30, 1e-30, first, count)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--dist", choices=["eu", "kl"], default="eu")
    ap.add_argument("--powerlaw", type=float, default=0.0, help="row-length exponent (0: uniform rows)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3, help="alternating sparse / dense timing rounds")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dense-max-gib", type=float, default=8.0)
    ap.add_argument("--masked", action="store_true", help="time a masked handle on the same pattern instead of the dense path")
    a = ap.parse_args()

    import torch
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    dist = L.EU if a.dist == "eu" else L.KL
    x = sparse.normalise(make_csr(a.m, a.n, a.density, a.seed, a.powerlaw), a.k)
    rs = np.random.RandomState(a.seed)
    w0 = np.abs(rs.randn(a.m, a.k))
    h0 = np.abs(rs.randn(a.k, a.n))
    stream = torch.cuda.current_stream().cuda_stream

    engines = {}
    se = Engine.for_sparse(x, a.k)
    se.set_stream(stream)
    se.set_factors(w0, h0)
    engines["sparse"] = se
    dense_gib = a.m * a.n * 4 / 2 ** 30
    if a.masked:
        me = Engine.for_sparse(x, a.k, masked=True)
        me.set_stream(stream)
        me.set_factors(w0, h0)
        engines["masked"] = me
    elif dense_gib <= a.dense_max_gib:
        de = Engine(a.m, a.n, a.k)
        de.set_stream(stream)
        de.upload_v(x.toarray())
        de.set_factors(w0, h0)
        engines["dense"] = de
    done = {name: 0 for name in engines}
    ms = {name: [] for name in engines}
    for name, eng in engines.items():             # warm-up batch
        timed(eng, dist, 0, 3, torch)
        done[name] = 3
    for _ in range(a.reps):
        for name, eng in engines.items():
            ms[name].append(timed(eng, dist, done[name], a.iters, torch))
            done[name] += a.iters
    for name, eng in engines.items():
        rule, _, _ = eng.state()
        assert rule == 0, f"{name}: the stop rule fired during timing"
    kp = next(p for p in (4, 8, 16, 32, 64, 128, 256) if p >= a.k)
    nnz = x.nnz
    streams = 2 * nnz * 8                          # CSR + CSC: index and value per non-zero
    gathers = 2 * nnz * kp * 4                     # a factor row per non-zero and phase
    factors = 3 * (a.m + a.n) * kp * 4             # own rows read and written, then read by the Gram pass
    total = streams + gathers + factors
    sparse_ms = min(ms["sparse"])
    lens = np.diff(x.indptr)
    out = {"m": a.m, "n": a.n, "k": a.k, "kp": kp, "dist": a.dist, "density": a.density, "powerlaw": a.powerlaw,
           "nnz": int(nnz), "max_row_nnz": int(lens.max()), "median_row_nnz": float(np.median(lens)),
           "sparse_ms_per_iter": round(sparse_ms, 4), "bytes_per_iter": int(total), "gathered_bytes": int(gathers),
           "gb_per_s": round(total / sparse_ms / 1e6, 1),
           "dense_ms_per_iter": round(min(ms["dense"]), 4) if "dense" in ms else None,
           "dense_precision": engines["dense"].precision() if "dense" in engines else None,
           "masked_ms_per_iter": round(min(ms["masked"]), 4) if "masked" in ms else None}
    print(json.dumps(out), flush=True)
    for eng in engines.values():
        eng.reset_stream()
        eng.close()


if __name__ == "__main__":
    main()
