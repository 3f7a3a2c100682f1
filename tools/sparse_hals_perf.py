"""Time nmfx_hals_sparse_run beside nmfx_mur_run (Euclidean) on the same sparse V, and count the iterations HALS needs to
reach the objective MUR has after --mur-iters iterations.

    python tools/sparse_hals_perf.py --m 16384 --n 8192 --density 0.01 --k 64
    python tools/sparse_hals_perf.py --m 16384 --n 8192 --density 0.01 --k 64 --powerlaw 1.0
    python tools/sparse_hals_perf.py --m 1048576 --n 131072 --density 0.0001 --k 32 --mur-iters 500
    python tools/sparse_hals_perf.py --table > profiles/sparse_hals_perf.txt       # the rows of DESIGN.md 4.2's table
    python tools/sparse_hals_perf.py --wide-table > profiles/sparse_hals_wide_perf.txt      # k = 256: DESIGN.md 4.19

With 129 <= k <= 256 HALS is nmfx_hals_sparse_wide_run and the split is by its scopes: the two gathers, the two tiled sweeps
(sp_hals_wide_wsweep / _hsweep), the cross-term reduction and the two stats launches.

Inputs are the seeded random CSR of tools/sparse_perf.py.  Both solvers start from the same seeded |randn| factors, HALS
from their least-squares rescaling (hals.start_scale), each on a handle of its own in one process.  One JSON line per case:
  ms per iteration over warmed batches with device events, best of --reps rounds, the two solvers alternated;
  the per-scope split of a profiled batch of HALS (nmfx_profile_get: events around every launch site, so their sum is above
  the unprofiled figure);
  mur_obj: the recorded objective after --mur-iters MUR iterations; hals_reaches_at: the first iteration after which the
  recorded HALS objective is at or below it (None within --hals-max iterations); hals_obj_at_10 / _30 for orientation."""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NMF_AMD_QUIET", "1")

import numpy as np

from sparse_perf import make_csr

NEVER = 10 ** 12
TABLE = [["--m", "16384", "--n", "8192", "--k", "64", "--density", d] for d in ("0.001", "0.01", "0.05")]
TABLE += [["--m", "16384", "--n", "8192", "--k", "64", "--density", "0.01", "--powerlaw", "1.0"],
          ["--m", "1048576", "--n", "131072", "--k", "32", "--density", "0.0001"]]
WIDE_TABLE = [["--m", "16384", "--n", "8192", "--k", "256", "--density", d] for d in ("0.001", "0.01", "0.05")]
WIDE_TABLE += [["--m", "16384", "--n", "8192", "--k", "256", "--density", "0.01", "--powerlaw", "1.0"]]
SCOPES = ("sp_hals_wphase", "sp_stats", "sp_hals_hphase")
WIDE_SCOPES = ("sp_hals_wide_wgather", "sp_hals_wide_wsweep", "sp_hals_wide_hgather", "sp_hals_wide_hsweep", "sp_hals_wide_cross", "sp_stats")


def timed(run, first, count, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run(first, count)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--powerlaw", type=float, default=0.0, help="row-length exponent (0: uniform rows)")
    ap.add_argument("--sweeps", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3, help="alternating timing rounds")
    ap.add_argument("--mur-iters", type=int, default=500)
    ap.add_argument("--hals-max", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--table", action="store_true", help="run the rows of DESIGN.md 4.2's table, one process each")
    ap.add_argument("--wide-table", action="store_true", help="run the rows of DESIGN.md 4.19's table (k = 256), one process each")
    a = ap.parse_args()
    if a.table or a.wide_table:
        for row in (WIDE_TABLE if a.wide_table else TABLE):
            subprocess.run([sys.executable, os.path.abspath(__file__), *row], check=True)
        return

    import torch
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    from nmf_amd.hals import start_scale
    x = sparse.normalise(make_csr(a.m, a.n, a.density, a.seed, a.powerlaw), a.k)
    rs = np.random.RandomState(a.seed)
    w0 = np.abs(rs.randn(a.m, a.k))
    h0 = np.abs(rs.randn(a.k, a.n))
    stream = torch.cuda.current_stream().cuda_stream
    with Engine.for_sparse(x, a.k) as me, Engine.for_sparse(x, a.k) as he:
        me.set_stream(stream)
        he.set_stream(stream)
        alpha = start_scale(he, w0, h0)
        ws, hs = w0 * np.sqrt(alpha), h0 * np.sqrt(alpha)
        hals_run = he.hals_sparse_wide_run if a.k > 128 else he.hals_sparse_run
        run = {"mur": lambda first, count: me.mur_run(L.EU, 0.0, 0.0, NEVER, 1e-30, 1e-30, first, count),
               "hals": lambda first, count: hals_run(0.0, 0.0, a.sweeps, NEVER, 1e-30, 1e-30, first, count)}

        def restart():
            me.set_factors(w0, h0)
            he.set_factors(ws, hs)

        # -- ms per iteration, alternated ---------------------------------------------------------------------------------
        restart()
        done = {}
        ms = {name: [] for name in run}
        for name in run:
            timed(run[name], 0, 3, torch)
            done[name] = 3
        for _ in range(a.reps):
            for name in run:
                ms[name].append(timed(run[name], done[name], a.iters, torch))
                done[name] += a.iters
        # -- the per-scope split of one profiled HALS batch ---------------------------------------------------------------
        he.profile_reset()
        he.profile_enable(True)
        run["hals"](done["hals"], a.iters)
        he.synchronize()
        split = {}
        for scope in (WIDE_SCOPES if a.k > 128 else SCOPES):
            t, cnt = he.profile_get(scope)
            split[scope] = round(t / a.iters, 4)
        he.profile_enable(False)
        # -- iterations to MUR's objective --------------------------------------------------------------------------------
        restart()
        run["mur"](0, a.mur_iters)
        me.mur_finish(L.EU, NEVER, 1e-30, 1e-30, a.mur_iters)
        mur_obj = float(me.objectives(a.mur_iters, 1)[0])
        run["hals"](0, a.hals_max)
        hist = he.objectives(0, a.hals_max + 1)
        below = np.nonzero(hist[1:] <= mur_obj)[0]
        assert me.state()[0] == 0 and he.state()[0] == 0, "the stop rule fired during the measurement"
        me.reset_stream()
        he.reset_stream()
    lens = np.diff(x.indptr)
    out = {"m": a.m, "n": a.n, "k": a.k, "density": a.density, "powerlaw": a.powerlaw, "nnz": int(x.nnz), "sweeps": a.sweeps,
           "max_row_nnz": int(lens.max()), "median_row_nnz": float(np.median(lens)),
           "mur_eu_ms_per_iter": round(min(ms["mur"]), 4), "hals_ms_per_iter": round(min(ms["hals"]), 4),
           "hals_profiled_ms_per_iter": split, "alpha": alpha,
           "mur_iters": a.mur_iters, "mur_obj": mur_obj, "hals_reaches_at": int(below[0]) + 1 if len(below) else None,
           "hals_obj_at_10": float(hist[10]) if a.hals_max >= 10 else None,
           "hals_obj_at_30": float(hist[30]) if a.hals_max >= 30 else None, "hals_obj_at_max": float(hist[-1])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
