"""Time one HALS fold-in solve (nmfx_hals_foldin_run at the defaults tol = 1e-4, max_sweeps = 200) beside one H phase of the
fit it follows, on the same handle.

    python tools/hals_transform_perf.py --kind masked --m 16384 --n 8192 --density 0.10 --k 64
    python tools/hals_transform_perf.py --table > profiles/hals_transform_perf.txt

Inputs are the seeded random CSR of tools/sparse_perf.py (--kind masked: its stored entries are the observed set), the matrices
of profiles/sparse_hals_perf.txt and profiles/masked_hals_perf.txt.  W comes from --fit-iters HALS iterations from the seeded,
rescaled |randn| start on that handle; the fold-in then starts from h0 = 0 against that W.  One JSON line per case:
  foldin_ms: device time of one nmfx_hals_foldin_run (two objective records included), best of --reps, device events;
  foldin_solve_ms: the solve's own scope (sp_hals_foldin / sp_mhals_foldin) of a profiled run (nmfx_profile_get);
  sweeps_mean, sweeps_max, at_cap: over the columns of that run;
  hphase_ms: one sp_hals_hphase / sp_mhals_hphase scope of a profiled HALS iteration (sweeps = 1) on the same handle.

    python tools/hals_transform_perf.py --dense           # 16384 x 8192, k = 64 and 128, writes profiles/hals_transform_dense_perf.txt

--dense: the dense fold-in (nmfx_hals_foldin_dense_run) on one seeded planted matrix per rank, in the default
arithmetic.  W comes from --fit-iters `hals` iterations from the seeded, rescaled uniform start; the fold-in starts from h0 = 0 at
the defaults.  Per rank, in ms: one call (device events around it, as in the sparse table, best of --reps; its two float64
objective passes included), its hals_solve scope, its product scope (hphase; gram_tn and pack beside it), one hals_sweep H-side scope of the fit;
the mean and largest sweep count and the columns at the cap; and the time the multiplicative fold-in
transform(x_new, w, distance_type='eu') (nmfx_foldin_run from its default |randn| start, seeded) needs until it first records
an objective at or below the fold-in's, or its objective after --mur-max-iter iterations if it never gets there."""
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
TABLE = [["--kind", "sparse", "--m", "16384", "--n", "8192", "--k", "64", "--density", d] for d in ("0.001", "0.01", "0.05")]
TABLE += [["--kind", "sparse", "--m", "16384", "--n", "8192", "--k", "64", "--density", "0.01", "--powerlaw", "1.0"],
          ["--kind", "sparse", "--m", "1048576", "--n", "131072", "--k", "32", "--density", "0.0001"]]
TABLE += [["--kind", "masked", "--m", "16384", "--n", "8192", "--k", "64", "--density", d] for d in ("0.01", "0.10", "0.50")]
TABLE += [["--kind", "masked", "--m", "1048576", "--n", "131072", "--k", "32", "--density", "0.0001"]]


def clocked(fn):
    """Device time of fn() in ms between two events on the current torch stream (the engine runs on it: set_stream), as the
    sparse table times its calls."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def dense(a, k, say):
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    from nmf_amd.hals import start_scale
    from nmf_amd.synth import planted_matrix
    m, n = a.m, a.n
    v = planted_matrix(m, n, k, seed=a.seed, dtype=np.float32)
    rs = np.random.RandomState(a.seed)
    w0, h0 = rs.rand(m, k), rs.rand(k, n)
    zeros = np.zeros((k, n))
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    with Engine(m, n, k) as eng:
        eng.set_stream(stream)
        eng.upload_v(v)
        arith = eng.precision()
        alpha = start_scale(eng, w0, h0)
        eng.set_factors(w0 * np.sqrt(alpha), h0 * np.sqrt(alpha))
        eng.hals_run(0.0, 0.0, 1, NEVER, 1e-30, 1e-30, 0, a.fit_iters)
        eng.profile_reset()                                 # one H-side sweep of the fit, profiled
        eng.profile_enable(True)
        eng.hals_run(0.0, 0.0, 1, NEVER, 1e-30, 1e-30, a.fit_iters, 3)
        eng.synchronize()
        t, cnt = eng.profile_get("hals_sweep_h")
        sweep_h_ms = t / cnt
        t, cnt = eng.profile_get("hphase")
        fit_hphase_ms = t / cnt
        eng.profile_enable(False)
        w, _ = eng.get_factors()
        ms = []
        for _ in range(a.reps + 1):                         # (the first round warms up)
            eng.set_factors(w, zeros)
            ms.append(clocked(lambda: eng.hals_foldin_dense_run(0.0, a.tol, a.max_sweeps)))
        sweeps = eng.hals_foldin_dense_sweeps()
        obj = eng.objectives(0, 2)
        eng.set_factors(w, zeros)
        eng.profile_reset()
        eng.profile_enable(True)
        eng.hals_foldin_dense_run(0.0, a.tol, a.max_sweeps)
        eng.synchronize()
        scopes = {name: eng.profile_get(name) for name in ("hals_solve", "hphase", "gram_tn", "pack", "images", "objective_f64")}
        eng.profile_enable(False)
        eng.reset_stream()
    assert scopes["hphase"][1] == 1 and scopes["hals_solve"][1] == 1
    target = float(obj[1])
    rs = np.random.RandomState(a.seed)
    h_mur = np.abs(rs.randn(k, n))                           # transform's default start
    batch, done, t_mur, first, last = 50, 0, 0.0, None, None
    with Engine.for_phase(v, k, (w, h_mur)) as eng:
        eng.set_stream(stream)
        clocked(lambda: eng.foldin_run(L.EU, 0.0, NEVER, 0.0, 0.0, 0, 2))      # warm-up
        eng.set_factors(w, h_mur)
        while first is None and done < a.mur_max_iter:
            t_mur += clocked(lambda: eng.foldin_run(L.EU, 0.0, NEVER, 0.0, 0.0, done, batch))
            done += batch
            hist = eng.objectives(0, done)                   # (obj[t] is recorded when iteration t starts)
            last = float(hist[-1])
            if (hist <= target).any():
                first = int(np.argmax(hist <= target))
        eng.reset_stream()
    mur_ms = t_mur / done
    say(f"{m} x {n}, k = {k}, {arith} arithmetic; W from {a.fit_iters} hals iterations; fold-in from h0 = 0, tol = {a.tol:g}, max_sweeps = {a.max_sweeps}")
    say(f"  one call                       {min(ms[1:]):9.3f} ms   (best of {a.reps}; rounds {', '.join(f'{t:.3f}' for t in ms[1:])})")
    say(f"    hals_solve scope             {scopes['hals_solve'][0]:9.3f} ms")
    say(f"    product scope (hphase)       {scopes['hphase'][0]:9.3f} ms   (gram_tn {scopes['gram_tn'][0]:.3f}, pack {scopes['pack'][0]:.3f}, images {scopes['images'][0]:.3f})")
    say(f"    two objective_f64 passes     {scopes['objective_f64'][0]:9.3f} ms")
    say(f"  one hals_sweep H side of the fit {sweep_h_ms:7.3f} ms   (its hphase {fit_hphase_ms:.3f} ms); hals_solve / hals_sweep_h = {scopes['hals_solve'][0] / sweep_h_ms:.1f}")
    say(f"  sweeps per column: mean {sweeps.mean():.2f}, largest {int(sweeps.max())}; columns at the cap of {a.max_sweeps}: {int((sweeps == a.max_sweeps).sum())} of {n}")
    say(f"  objective: start {float(obj[0]):.6g}, folded {target:.6g}")
    if first is None:
        say(f"  transform 'eu' ({mur_ms:.3f} ms per iteration): not reached in {done} iterations, {t_mur:.1f} ms; its objective there {last:.6g}")
    else:
        say(f"  transform 'eu' ({mur_ms:.3f} ms per iteration): first at or below the folded objective at iteration {first}, {first * mur_ms:.1f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dense", action="store_true", help="the dense fold-in table (k from --ks), written to --out")
    ap.add_argument("--ks", default="64,128")
    ap.add_argument("--mur-max-iter", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "hals_transform_dense_perf.txt"))
    ap.add_argument("--kind", choices=("sparse", "masked"), default="sparse")
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--powerlaw", type=float, default=0.0, help="row-length exponent (0: uniform rows)")
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-sweeps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--table", action="store_true", help="every matrix of the two HALS tables, one process each")
    a = ap.parse_args()
    if a.dense:
        lines = []

        def say(text):
            print(text, flush=True)
            lines.append(text)
        for k in [int(t) for t in a.ks.split(",")]:
            dense(a, k, say)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        return
    if a.table:
        for row in TABLE:
            subprocess.run([sys.executable, os.path.abspath(__file__), *row], check=True)
        return

    import torch
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    from nmf_amd.hals import masked_start_scale, start_scale
    masked = a.kind == "masked"
    x = sparse.normalise(make_csr(a.m, a.n, a.density, a.seed, a.powerlaw), a.k)
    rs = np.random.RandomState(a.seed)
    w0 = np.abs(rs.randn(a.m, a.k))
    h0 = np.abs(rs.randn(a.k, a.n))
    zeros = np.zeros((a.k, a.n))
    stream = torch.cuda.current_stream().cuda_stream
    scope = "sp_mhals" if masked else "sp_hals"
    with Engine.for_sparse(x, a.k, masked=masked) as eng:
        eng.set_stream(stream)
        fit = eng.hals_masked_run if masked else eng.hals_sparse_run
        alpha = (masked_start_scale if masked else start_scale)(eng, w0, h0)
        eng.set_factors(w0 * np.sqrt(alpha), h0 * np.sqrt(alpha))
        fit(0.0, 0.0, 1, NEVER, 1e-30, 1e-30, 0, a.fit_iters)
        # -- one H phase of the fit, profiled ---------------------------------------------------------------------------------
        eng.profile_reset()
        eng.profile_enable(True)
        fit(0.0, 0.0, 1, NEVER, 1e-30, 1e-30, a.fit_iters, 3)
        eng.synchronize()
        t, cnt = eng.profile_get(scope + "_hphase")
        hphase_ms = t / cnt
        eng.profile_enable(False)
        w, _ = eng.get_factors()
        # -- the fold-in against that W from h0 = 0 ---------------------------------------------------------------------------
        ms = []
        for _ in range(a.reps + 1):                       # (the first round warms up)
            eng.set_factors(w, zeros)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.hals_foldin_run(0.0, a.tol, a.max_sweeps)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        sweeps = eng.hals_foldin_sweeps()
        obj = eng.objectives(0, 2)
        eng.set_factors(w, zeros)
        eng.profile_reset()
        eng.profile_enable(True)
        eng.hals_foldin_run(0.0, a.tol, a.max_sweeps)
        eng.synchronize()
        solve_ms = eng.profile_get(scope + "_foldin")[0]
        eng.profile_enable(False)
        eng.reset_stream()
    lens = np.diff(x.tocsc().indptr)
    out = {"kind": a.kind, "m": a.m, "n": a.n, "k": a.k, "density": a.density, "powerlaw": a.powerlaw, "nnz": int(x.nnz),
           "max_col_nnz": int(lens.max()), "tol": a.tol, "max_sweeps": a.max_sweeps, "fit_iters": a.fit_iters,
           "foldin_ms": round(min(ms[1:]), 4), "foldin_solve_ms": round(solve_ms, 4), "hphase_ms": round(hphase_ms, 4),
           "solve_over_hphase": round(solve_ms / hphase_ms, 3), "sweeps_mean": round(float(sweeps.mean()), 2),
           "sweeps_max": int(sweeps.max()), "at_cap": int((sweeps == a.max_sweeps).sum()),
           "obj_start": float(obj[0]), "obj_folded": float(obj[1])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
