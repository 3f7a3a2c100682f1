"""Digest of what the dense exact-f32 phase path of MUR (kernels_phase.hip) computes: one SHA-256 per case.

    python tools/phase_digest.py > digest.txt

Every case sets seeded factors, runs 3 iterations with the stop rule off, finishes, and hashes the bytes of W, H and the
four recorded objectives.  The cases are 'is', weighted 'eu' / 'kl' / 'is', 'beta' at beta = -1, 0.5, 1, 2.5 and weighted
'beta' at beta = 0.5, 1.5, each on five shapes that between them reach every padded rank, a ragged single column and a
split contracted dimension.  The weights hold zero cells and, where the shape allows, an all-zero row and column.

Two builds that print the same lines perform the same floating-point operations in the same order: the file is what a
change of the kernels' text that is meant to change no result is checked against.  The script uses nmf_amd.engine.Engine
and nmf_amd._lib only, so it runs unmodified in a checkout of another commit; all cases run in one process."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NMF_AMD_QUIET", "1")

import numpy as np

NEVER = 10 ** 12
ITERS = 3
# m, n, k, lambda_w, lambda_h
SHAPES = [(127, 1, 3, 0.0, 0.0), (300, 200, 20, 0.0, 0.1), (257, 130, 64, 0.0, 0.0), (700, 600, 16, 0.05, 0.0),
          (640, 384, 128, 0.02, 0.3)]
# name, distance, beta, weighted
PATHS = ([("is", "IS", None, False), ("wt-eu", "EU", None, True), ("wt-kl", "KL", None, True), ("wt-is", "IS", None, True)]
         + [(f"beta{b:g}", "BETA", b, False) for b in (-1.0, 0.5, 1.0, 2.5)]
         + [(f"wt-beta{b:g}", "BETA", b, True) for b in (0.5, 1.5)])


def make_inputs(m, n, k, seed):
    """V uniform in [0.05, 1) (strictly positive: IS and beta <= 0 need that), W0 and H0 uniform in [0.1, 1) drawn as f32."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 1.0, (m, n)).astype(np.float32)
    w0 = rng.uniform(0.1, 1.0, (m, k)).astype(np.float32).astype(np.float64)
    h0 = rng.uniform(0.1, 1.0, (k, n)).astype(np.float32).astype(np.float64)
    return v, w0, h0


def make_weights(m, n, seed):
    """Log-uniform weights over four decades, a tenth of the cells at zero and -- m, n >= 8 -- row 1 and column 3 all zero."""
    rng = np.random.default_rng(seed)
    om = (10.0 ** rng.uniform(-2.0, 2.0, (m, n))).astype(np.float32)
    om[rng.random((m, n)) < 0.1] = 0
    if m >= 8 and n >= 8:
        om[1, :] = 0
        om[:, 3] = 0
    return om


def main():
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    for m, n, k, lw, lh in SHAPES:
        v, w0, h0 = make_inputs(m, n, k, seed=2000 + k)
        om = make_weights(m, n, seed=3000 + k)
        for name, dist, beta, weighted in PATHS:
            with Engine(m, n, k) as eng:
                eng.upload_v(v)
                if weighted:
                    eng.upload_weights(om)
                if beta is not None:
                    eng.set_beta(beta)
                code = getattr(L, dist)
                eng.set_factors(w0, h0)
                eng.mur_run(code, lw, lh, NEVER, 0, 0, 0, ITERS)
                eng.mur_finish(code, NEVER, 0, 0, ITERS)
                w, h = eng.get_factors()
                obj = eng.objectives(0, ITERS + 1)
            digest = hashlib.sha256(w.tobytes() + h.tobytes() + obj.tobytes()).hexdigest()
            print(f"{name:<10} {m}x{n} k={k} lw={lw:g} lh={lh:g}  {digest}  obj[{ITERS}]={obj[ITERS]!r}", flush=True)


if __name__ == "__main__":
    main()
