"""Problem-by-problem checks of single sparse HALS half-steps with 129 .. 256 components (tests/test_gpu_hals_sparse_wide_step.py,
tests/test_hals_sparse_wide_step_bars.py): nmf_amd.hals.hals_sparse_wide, nmfx_hals_sparse_wide_run (csrc/kernels_sparse.hip,
DESIGN.md 4.19).

Matrices, the float64 reference, the comparator and the two-iteration protocol are those of tests/sparse_hals_step.py.  What is
new at these ranks is the route of a half-step: sp_hals_wide_gather_kernel leaves every problem's r in a buffer (a wave holds a
256-vector as one float4 per lane, so a group is the whole wave and a step of the gather is four consecutive non-zeros), rows
longer than 256 non-zeros go through pieces and sp_hals_wide_fixup_kernel, and hals_wide_sweep_kernel streams G through LDS in
tiles of 64 rows with four variables per lane.  The cases are the smallest at which that can go wrong:
    base    k = 129 (the last tile and the last slot almost all padding), 200, 255, 256 (full); the regimes and three sweeps at 200
    rows    k = 129: rows of 1 / 255 / 256 / 257 / 513 non-zeros, both sides of the piece boundary
    1x300, 300x1, 5x4    k = 129: fewer problems than a block has waves
    tall    k = 129: 20000 rows, more than one round of the gather grid (4 x 256 blocks of 8 waves) and of the sweep grid
            (2 x 256 blocks of 8 problems)
lambda follows sparse_hals_step.lam_of (by k % 3; (0, 0) in the dead regime)."""
from hals_step import Run
from sparse_hals_step import NEVER, OBJ_RTOL, CHUNK, DEAD, Case, case_id, lam_of, matrix, start          # noqa: F401
from sparse_hals_step import host_hals, gram_rhs, half_steps, values, check_steps, objective             # noqa: F401

MIN_K, MAX_K = 129, 256
KP = 256                     # every case runs at kp = 256
TILE = 64                    # rows of G per LDS tile of hals_wide_sweep_kernel at kp = 256
LONG_ROW = 4                 # the row of the rows matrix with 513 non-zeros: pieces of 256, 256 and 1


def _cases():
    out = [Case("base", k, "scaled", 1) for k in (129, 200, 255, 256)]
    out += [Case("base", 200, rg, 1) for rg in ("cold", "settled", "dead")]
    out += [Case("base", 200, "scaled", 3)]
    out += [Case("rows", 129, "scaled", 1)]
    out += [Case(name, 129, "scaled", 1) for name in ("1x300", "300x1", "5x4")]
    out += [Case("tall", 129, "scaled", 1)]
    return out


CASES = _cases()


# ---- device runner ------------------------------------------------------------------------------------------------------------
def run_hals_sparse_wide(x, w0, h0, lw=0.0, lh=0.0, sweeps=1, steps=(1, 2)):
    """The calls nmf_amd.hals.hals_sparse_wide makes, with the stop rule off, on a fresh sparse handle: {s: Run}."""
    from nmf_amd.engine import Engine
    out = {}
    with Engine.for_sparse(x, w0.shape[1]) as eng:
        for s in steps:
            eng.set_factors(w0, h0)
            eng.hals_sparse_wide_run(lw, lh, sweeps, NEVER, 0, 0, 0, s)
            eng.hals_sparse_wide_finish(NEVER, 0, 0, s)
            w, h = eng.get_factors()
            assert eng.state()[2] == s + 1
            out[s] = Run(w, h, eng.objectives(0, s + 1))
    return out


# The bar per case: the project's rule -- 10 x the largest deviation of the host emulation of the device arithmetic from the
# float64 sweep over the emulated two-iteration trajectory (tests/test_hals_sparse_wide_step_bars.py: G rounded to f32 from
# float64 with 2 lambda added in f32, r summed in f32 on the W side and rounded from float64 on the H side, the sweep in float32
# on a kept residual).  The floor of the table is the emulated deviation with a quarter added, rounded up to two digits.
# Three floors are not small.  1x300 and 5x4 have a Gram matrix of rank 1 and 4 under 129 variables at lambda = 0 (k % 3 = 0),
# and in the cold regime at k = 200 one sweep moves x by orders of magnitude on a kept residual: float32 itself is that far from
# the float64 sweep there, in the emulation and on the device alike (the third column), and what those cases still decide is the
# exact zeros, the sign, the padding, the recorded objectives and -- through their shapes -- the launch geometry.  The
# emulation passes the comparator's exact-zero rule on every case, so no regime had to be swapped.
# case id: (emulated floor, bar = 10 x floor, largest deviation measured on an MI355X with NMFX_RECORD_BARS)
BARS = {
    "base-k129-scaled": (8.7e-06, 8.7e-05, 7.0e-06),
    "base-k200-scaled": (1.3e-05, 1.3e-04, 1.2e-05),
    "base-k255-scaled": (6.1e-05, 6.1e-04, 4.0e-05),
    "base-k256-scaled": (1.2e-05, 1.2e-04, 1.0e-05),
    "base-k200-cold": (4.7e-01, 4.7e+00, 7.9e-02),
    "base-k200-settled": (1.6e-06, 1.6e-05, 1.2e-06),
    "base-k200-dead": (4.0e-05, 4.0e-04, 3.1e-05),
    "base-k200-scaled-s3": (4.1e-05, 4.1e-04, 4.2e-05),
    "rows-k129-scaled": (6.6e-05, 6.6e-04, 1.4e-04),
    "1x300-k129-scaled": (1.1e+01, 1.1e+02, 4.1e+00),
    "300x1-k129-scaled": (3.7e-04, 3.7e-03, 2.4e-04),
    "5x4-k129-scaled": (2.5e+00, 2.5e+01, 3.2e+00),
    "tall-k129-scaled": (6.2e-05, 6.2e-04, 5.0e-05),
}


def bar_of(c):
    return BARS[case_id(c)][1]


def run_case(c):
    x = matrix(c.matrix)
    w0, h0 = start(c)
    lw, lh = lam_of(c)
    runs = run_hals_sparse_wide(x, w0, h0, lw, lh, c.sweeps)
    check_steps(x, w0, h0, runs, lw, lh, c.sweeps, bar_of(c), tag=f"{case_id(c)} ")
    return runs
