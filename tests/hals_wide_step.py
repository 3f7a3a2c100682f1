"""Problem-by-problem checks of single HALS half-steps beyond 128 components (tests/test_gpu_hals_wide_step.py,
tests/test_hals_wide_step_bars.py): nmf_amd.hals.hals_wide, nmfx_hals_wide_run, hals_wide_sweep_kernel (csrc/kernels_hals.hip).

The half-step, its float64 reference, the comparator and the two-iteration protocol are those of tests/hals_step.py; inputs,
regimes and lambdas those of tests/anls_step.py.  What is new beyond 128 components is how G reaches the sweep: the kernel streams
it through LDS in tiles of T rows (64 at kp = 256, 32 up to 512, 16 beyond) with NV = kp / 64 variables per lane, so the cases
stand at every kp the kernel is instantiated for, at ranks whose last tile and last slot are almost all padding, and at problem
counts that leave waves of a block without a problem."""
import numpy as np

import anls_step as A
import hals_step as HS
from mur_step import NEVER

WAVES = 8                    # problems per workgroup of hals_wide_sweep_kernel (NMFX_HALS_WAVES)
BLOCKS_PER_CU = 2            # NMFX_HALS_BLOCKS_PER_CU: a tile is at most 64 KiB
MIN_K, MAX_K = 129, 1024


def kp_of(k):
    return -(-k // 128) * 128


def tile_rows(k):
    """Rows of G per LDS tile of hals_wide_sweep_kernel at this rank."""
    kp = kp_of(k)
    return 64 if kp <= 256 else 32 if kp <= 512 else 16


def wrap_stride(ncu=256):
    """Problems one round of the grid covers with `ncu` CUs: beyond it the blocks of hals_wide_sweep_kernel take another trip."""
    return ncu * BLOCKS_PER_CU * WAVES


# ---- device runner ------------------------------------------------------------------------------------------------------------
def run_hals_wide(v, w0, h0, lw=0.0, lh=0.0, sweeps=1, kind="eu", precision=None, steps=(1, 2)):
    """The calls nmf_amd.hals.hals_wide makes, with the stop rule off, on a fresh dense handle: ({s: Run}, arithmetic)."""
    from nmf_amd.engine import Engine
    m, n = v.shape
    k = w0.shape[1]
    out = {}
    with Engine(m, n, k) as eng:
        if precision is not None:
            eng.set_precision(precision)
        arith = A._arith(eng, k, precision)
        eng.upload_v(v)
        for s in steps:
            eng.set_factors(w0, h0)
            eng.anls_set_distance(A._dist(kind))
            eng.hals_wide_run(lw, lh, sweeps, NEVER, 0, 0, 0, s)
            eng.aoadmm_finish(NEVER, 0, 0, s)
            w, h = eng.get_factors()
            out[s] = HS.Run(w, h, eng.objectives(0, s + 1))
    return out, arith


# ---- cases and bars -----------------------------------------------------------------------------------------------------------
Case = HS.Case               # regime m n k arith sweeps
case_id = HS.case_id
lam_of = HS.lam_of           # LAMS by k % 3; both positive where a Gram matrix is singular; 0 in the dead regime (anls_step.lam_of)

RANKS = (129, 200, 256, 257, 384, 500, 512, 640, 1000, 1024)      # kp 256, 384, 512, 640 and 1024 ...
RANKS_KP = (700, 896)                                             # ... and the two instantiations those leave out, kp 768 and 896
REGIME_RANKS = (200, 300)
SHAPES = ((1, 257), (257, 1), (130, 64))
# 257 x 1 runs the cold regime.  The mixed regime scales down every third column of V and of H0, the first among them: with a single
# column the whole problem stands at 0.02 of the planted scale under rows of W0 at the full scale.  The first W sweep then moves x
# from 0.07 to 1e-4, G_jj x_j (7e-3) carries an f32 rounding of 4e-10, and the comparator's rule for exact zeros, a float64 clamp deeper
# than STRICT max|r| = 5e-10, asks float32 for a decision inside its last bit: the host emulation of the kernel's arithmetic leaves the
# same 2^-26 on the same variable as the device, and the emulated bar is 0.13.  Cold has V and the start at one scale: 32587
# strictly clamped zeros in that half-step, all exact in the emulation (test_hals_wide_step_bars.test_emulation_passes_the_comparator),
# and a bar of 3e-3.
SHAPE_REGIME = {(257, 1): "cold"}
WRAPS = ((4400, 70), (70, 4400))
SWEEP3_RANKS = (200, 384)


def _cases():
    out = []
    for k in RANKS:                                                            # ranks: 129 a tile that is almost all padding, 257 one live column in the last slot
        out += [Case("mixed", 257, 200, k, a, 1) for a in ("f32", "bf16")]
    out += [Case("mixed", 257, 200, k, "bf16", 1) for k in RANKS_KP]
    for k in REGIME_RANKS:                                                    # regimes
        out += [Case(rg, 257, 200, k, "bf16", 1) for rg in ("settled", "cold", "dead")]
    out += [Case(SHAPE_REGIME.get((m, n), "mixed"), m, n, 129, "bf16", 1) for m, n in SHAPES]      # one problem; fewer problems than a block has waves
    out += [Case("mixed", m, n, 129, "bf16", 1) for m, n in WRAPS]             # more problems than one round of the grid
    out += [Case("mixed", 257, 200, k, "bf16", 3) for k in SWEEP3_RANKS]       # further sweeps stream G again on the kept residual
    return out


CASES = _cases()

# The bar per case: the rule of tests/hals_step.py -- 10 x the largest deviation of the host emulation of the device arithmetic
# (tests/test_hals_wide_step_bars.py: G in exact f32, r with four split-bf16 terms or in exact f32, the sweep in float32 on a
# kept residual) from the float64 sweep over the emulated two-iteration trajectory.  The floor of the table is the emulated
# deviation with a quarter added for the BLAS's summation order, rounded up to two digits.
# case id: (emulated floor, bar = 10 x floor, largest deviation measured on an MI355X with NMFX_RECORD_BARS)
BARS = {
    "mixed-257x200-k129-f32": (1.8e-04, 1.8e-03, 8.6e-05),
    "mixed-257x200-k129-bf16": (6.5e-04, 6.5e-03, 5.8e-04),
    "mixed-257x200-k200-f32": (1.5e-04, 1.5e-03, 7.1e-05),
    "mixed-257x200-k200-bf16": (1.4e-04, 1.4e-03, 1.1e-04),
    "mixed-257x200-k256-f32": (2.0e-04, 2.0e-03, 1.3e-04),
    "mixed-257x200-k256-bf16": (2.3e-04, 2.3e-03, 1.6e-04),
    "mixed-257x200-k257-f32": (1.9e-04, 1.9e-03, 1.1e-04),
    "mixed-257x200-k257-bf16": (2.2e-04, 2.2e-03, 1.6e-04),
    "mixed-257x200-k384-f32": (3.4e-04, 3.4e-03, 2.0e-04),
    "mixed-257x200-k384-bf16": (3.4e-04, 3.4e-03, 2.9e-04),
    "mixed-257x200-k500-f32": (4.3e-04, 4.3e-03, 2.9e-04),
    "mixed-257x200-k500-bf16": (4.7e-04, 4.7e-03, 3.2e-04),
    "mixed-257x200-k512-f32": (4.3e-04, 4.3e-03, 3.2e-04),
    "mixed-257x200-k512-bf16": (4.7e-04, 4.7e-03, 4.0e-04),
    "mixed-257x200-k640-f32": (6.0e-04, 6.0e-03, 3.8e-04),
    "mixed-257x200-k640-bf16": (6.1e-04, 6.1e-03, 4.9e-04),
    "mixed-257x200-k1000-f32": (1.1e-03, 1.1e-02, 7.0e-04),
    "mixed-257x200-k1000-bf16": (1.1e-03, 1.1e-02, 7.7e-04),
    "mixed-257x200-k1024-f32": (1.1e-03, 1.1e-02, 7.3e-04),
    "mixed-257x200-k1024-bf16": (1.3e-03, 1.3e-02, 8.8e-04),
    "mixed-257x200-k700-bf16": (6.9e-04, 6.9e-03, 5.3e-04),
    "mixed-257x200-k896-bf16": (9.3e-04, 9.3e-03, 6.5e-04),
    "settled-257x200-k200-bf16": (2.1e-04, 2.1e-03, 1.6e-04),
    "cold-257x200-k200-bf16": (2.9e-04, 2.9e-03, 2.2e-04),
    "dead-257x200-k200-bf16": (2.3e-03, 2.3e-02, 1.5e-03),
    "settled-257x200-k300-bf16": (3.4e-04, 3.4e-03, 3.0e-04),
    "cold-257x200-k300-bf16": (5.8e-04, 5.8e-03, 4.7e-04),
    "dead-257x200-k300-bf16": (3.1e-03, 3.1e-02, 3.3e-03),
    "mixed-1x257-k129-bf16": (1.3e-03, 1.3e-02, 1.0e-03),
    "cold-257x1-k129-bf16": (3.0e-04, 3.0e-03, 2.3e-04),
    "mixed-130x64-k129-bf16": (9.0e-05, 9.0e-04, 6.5e-05),
    "mixed-4400x70-k129-bf16": (8.8e-05, 8.8e-04, 6.2e-05),
    "mixed-70x4400-k129-bf16": (1.2e-04, 1.2e-03, 9.3e-05),
    "mixed-257x200-k200-bf16-s3": (3.5e-04, 3.5e-03, 2.6e-04),
    "mixed-257x200-k384-bf16-s3": (7.3e-04, 7.3e-03, 5.6e-04),
}


def bar_of(c):
    return BARS[case_id(c)][1]


# ---- the public call against the float64 loop (tests/test_gpu_hals_wide.py) ---------------------------------------------------------
# (m, n, k, sweeps): five iterations from the seeded uniform start scaled by the float64 alpha, lambda on both sides, on the planted
# matrix of tests/test_gpu_hals.py.  The bars are those of that file; tests/test_hals_wide_step_bars.py holds the emulated
# trajectory under half of each.
PUBLIC_CASES = [(257, 200, 160, 1), (300, 260, 300, 1), (300, 260, 160, 2)]
PUBLIC_LAMS = (0.05, 0.02)
PUBLIC_ITERS = 5
PUBLIC_SEED = 5
PUBLIC_WH_BAR = 1e-4         # ||W H - (W H)_float64|| / ||V||
PUBLIC_HIST_RTOL = 2e-4      # every entry of the objective history


def public_id(m, n, k, sweeps):
    return f"{m}x{n}-k{k}-s{sweeps}"


def public_v(m, n, k):
    v = A.planted(m, n, k, seed=1, noise=0.02, jitter=0.05)[0]
    v.setflags(write=False)
    return v


def public_start(m, n, k, seed=PUBLIC_SEED):
    """The draw hals_wide makes with nndsvd_init=(False, 'zero') after np.random.seed(seed)."""
    rng = np.random.RandomState(seed)
    return rng.rand(m, k), rng.rand(k, n)


def run_case(c, kinds=("eu", "kl")):
    """Run case c on the device for each reported objective and check every half-step.  Returns {kind: {s: Run}}."""
    v, w0, h0 = A.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = lam_of(c)
    out, fails = {}, []
    for kind in kinds:
        runs, arith = run_hals_wide(v, w0, h0, lw, lh, c.sweeps, kind, c.arith)
        assert arith == c.arith, f"{case_id(c)}: ran in {arith} arithmetic"
        try:
            HS.check_steps(v, w0, h0, runs, lw, lh, c.sweeps, bar_of(c), kind=kind, tag=f"{case_id(c)} {kind} ")
        except AssertionError as e:
            fails.append(str(e))
        out[kind] = runs
    if fails:
        raise AssertionError("\n".join(fails))
    return out
