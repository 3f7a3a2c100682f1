"""Time one sparse MUR fold-in (nmfx_sparse_foldin_run at the defaults tol = 1e-4, max_iter = 1000) beside one H phase of the
`mur` fit it follows, on the same handle.

    python tools/sparse_transform_perf.py --kind masked --m 16384 --n 8192 --density 0.10 --k 64 --loss kl
    python tools/sparse_transform_perf.py --table           # writes profiles/sparse_transform_perf.txt

Inputs are the seeded random CSR of tools/sparse_perf.py (--kind masked: its stored entries are the observed set), the matrices
of the sparse and masked MUR tables of DESIGN.md 4.2.  W comes from --fit-iters `mur` iterations of that loss from the seeded
|randn| start on that handle; the fold-in then starts from transform_sparse's default h0 = sqrt(mean / k) against that W.  One
JSON line per case:
  foldin_ms: device time of one nmfx_sparse_foldin_run (two objective records included), best of --reps, device events;
  foldin_solve_ms: the solve's own scope (sp_mur_foldin) of a profiled run (nmfx_profile_get);
  steps_mean, steps_max, at_cap: over the columns of that run;
  hphase_ms: one sp_hphase scope of a profiled `mur` iteration on the same handle -- the kernel a repeated half-step would run;
  alternative_ms = steps_mean x hphase_ms: what repeating the H half-step for the mean number of steps would cost in that
  scope alone (its 1 - 3 further launches per step and the round trip of H not counted).
--table runs every row in a process of its own under a time limit of its own (--row-limit seconds) and stops at the first row
that fails."""
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
BASE = ["--m", "16384", "--n", "8192", "--k", "64"]
BIG = ["--m", "1048576", "--n", "131072", "--k", "32", "--density", "0.0001", "--loss", "eu"]
TABLE = [["--kind", "sparse", *BASE, "--density", d, "--loss", loss] for d in ("0.001", "0.01", "0.05") for loss in ("eu", "kl")]
TABLE += [["--kind", "sparse", *BASE, "--density", "0.01", "--powerlaw", "1.0", "--loss", "eu"], ["--kind", "sparse", *BIG]]
TABLE += [["--kind", "masked", *BASE, "--density", d, "--loss", loss] for d in ("0.01", "0.10", "0.50") for loss in ("eu", "kl")]
TABLE += [["--kind", "masked", *BIG]]


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=("sparse", "masked"), default="sparse")
    ap.add_argument("--loss", choices=("eu", "kl", "is"), default="kl")
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--density", type=float, default=0.01)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--powerlaw", type=float, default=0.0, help="row-length exponent (0: uniform rows)")
    ap.add_argument("--fit-iters", type=int, default=10)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--table", action="store_true", help="every matrix of the sparse and masked MUR tables, one process each")
    ap.add_argument("--row-limit", type=int, default=240, help="--table: seconds one row may take")
    ap.add_argument("--rows", default="", help="--table: 'first:last' rows of the table only (the output file is then appended to)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "sparse_transform_perf.txt"))
    a = ap.parse_args()
    if a.table:
        lo, hi = (int(t) if t else None for t in a.rows.split(":")) if a.rows else (None, None)
        lines = [open(a.out).read()] if a.rows and lo and os.path.exists(a.out) else []
        for row in TABLE[lo:hi]:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), *row], timeout=a.row_limit, capture_output=True, text=True)
            print(p.stdout, end="", flush=True)
            if p.returncode:                              # (nothing more is started after a row that failed)
                sys.exit(f"row {' '.join(row)} ended with status {p.returncode}\n{p.stderr[-2000:]}")
            lines.append(p.stdout)
            with open(a.out, "w") as fh:
                fh.write("".join(lines))
        return

    import torch
    from nmf_amd import losses, sparse
    from nmf_amd.engine import Engine
    masked = a.kind == "masked"
    x = sparse.normalise(make_csr(a.m, a.n, a.density, a.seed, a.powerlaw), a.k)
    rs = np.random.RandomState(a.seed)
    w0 = np.abs(rs.randn(a.m, a.k))
    h0 = np.abs(rs.randn(a.k, a.n))
    cells = x.nnz if masked else a.m * a.n
    start = np.full((a.k, a.n), np.sqrt(float(np.sum(x.data, dtype=np.float64)) / cells / a.k))
    dist = losses.CODES[a.loss]
    stream = torch.cuda.current_stream().cuda_stream
    with Engine.for_sparse(x, a.k, masked=masked) as eng:
        eng.set_stream(stream)
        eng.set_factors(w0, h0)
        eng.mur_run(dist, 0.0, 0.0, NEVER, 0.0, 0.0, 0, a.fit_iters)
        # -- one H phase of the fit, profiled -------------------------------------------------------------------------------------
        eng.profile_reset()
        eng.profile_enable(True)
        eng.mur_run(dist, 0.0, 0.0, NEVER, 0.0, 0.0, a.fit_iters, 3)
        eng.synchronize()
        t, cnt = eng.profile_get("sp_hphase")
        hphase_ms = t / cnt
        eng.profile_enable(False)
        w, _ = eng.get_factors()
        # -- the fold-in against that W from the default start ----------------------------------------------------------------------
        ms = []
        for _ in range(a.reps + 1):                       # (the first round warms up)
            eng.set_factors(w, start)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.sparse_foldin_run(dist, 0.0, a.tol, a.max_iter)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        steps = eng.sparse_foldin_iters()
        obj = eng.objectives(0, 2)
        eng.set_factors(w, start)
        eng.profile_reset()
        eng.profile_enable(True)
        eng.sparse_foldin_run(dist, 0.0, a.tol, a.max_iter)
        eng.synchronize()
        solve_ms = eng.profile_get("sp_mur_foldin")[0]
        eng.profile_enable(False)
        eng.reset_stream()
    lens = np.diff(x.tocsc().indptr)
    mean = float(steps.mean())
    out = {"kind": a.kind, "loss": a.loss, "m": a.m, "n": a.n, "k": a.k, "density": a.density, "powerlaw": a.powerlaw, "nnz": int(x.nnz),
           "max_col_nnz": int(lens.max()), "long_cols": int((lens > 256).sum()), "tol": a.tol, "max_iter": a.max_iter,
           "fit_iters": a.fit_iters, "foldin_ms": round(min(ms[1:]), 4), "foldin_solve_ms": round(solve_ms, 4),
           "hphase_ms": round(hphase_ms, 4), "steps_mean": round(mean, 2), "steps_max": int(steps.max()),
           "at_cap": int((steps == a.max_iter).sum()), "alternative_ms": round(mean * hphase_ms, 3),
           "solve_over_alternative": round(solve_ms / (mean * hphase_ms), 3), "obj_start": float(obj[0]), "obj_folded": float(obj[1])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
