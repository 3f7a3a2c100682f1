"""The row-sharded phases of ADMM, AO-ADMM and ANLS over several ragged shards, step by step against float64
(tests/shard_step.py: run_family, run_anls).

Several engine handles in ONE process, one per row shard, the collective done on the host in rank order between the phase calls,
both exchange buffers NaN wherever the table of include/nmfx.h ("who writes, who reads") keeps nothing alive.  The
sequences are those of nmf_amd/dist.py (tests/test_shard_family_bars.py pins them call by call); what a world of one cannot see
-- a phase that reads its own partial instead of the reduced buffer, a stop of the W sub-problem decided from a rank's own norm
sums, a table of the speculative rounds read one round off, padding rows of a ragged shard's partial, an exchange element nobody
wrote, rank-local KL auxiliaries advanced from a stale replicated h_aux -- goes through the checks the single-handle steps have,
at the single-handle bars (functions of the case alone: admm_step.bars_of, bars_ao_kl, anls_step.bar_of).  Every case asserts

  (a) h, h_aux, dual_h, the inner words, the objective history and state() are bit-identical on every rank;
  (b) each recorded objective is the float64 sum of the shards' partials, noted before the collective, in rank order, bit for bit;
  (c) each shard's f32 partial behind the first products phase is its own F_local^T D_local and F_local^T F_local (mur_step.compare
      at mur_step.BARS of the arithmetic that ran), the padding of the [factor][column] product and of the Gram matrix exactly 0;
  (d) no NaN in any readable state;
and, AO-ADMM: every rank's inner word of the W sub-problem is the decision re-derived from the rank-order float64 sums of the norm
sums (or tables) the shards left before each collective.

Not reached at a few seconds per test: the 128-row form of the fused W-side kernel (more than 32640 rows in ONE shard).  Not
covered here: RCCL, more than one device (tests/test_gpu_dist.py).

Run time on an MI355X: 84 tests in 16 s; the slowest, 2.1 s, is the first one, which loads the library (measured maxima:
DESIGN.md 5)."""
import numpy as np
import pytest

import admm_step as A
import anls_step as N
import mur_step as S
import shard_step as X

pytestmark = pytest.mark.gpu

CUTS257 = [0, 1, 66, 193, 257]                  # 1, 65, 127 and 64 rows
CUTS384 = [0, 1, 130, 321, 384]                 # 1, 129, 191 and 63 rows
CUTS130 = [0, 1, 66, 130]                       # 1, 65 and 64 rows
CUTS70 = X.LOCAL_STOP_CUTS                      # 7, 34 and 29 rows
CUTS4161 = [0, 4100, 4161]                      # 65 blocks of 64 rows inside the first shard: its norm sums wrap
AO_PROX = ("l1n", 0.05, "l1n", 0.05)


def cuts_of(c):
    return {257: CUTS257, 384: CUTS384, 130: CUTS130, 70: CUTS70, 4161: CUTS4161}[c.m]


def pick(**want):
    """The cases of admm_step.CASES with these fields (their bars are proven by tests/test_admm_step_bars.py)."""
    out = [c for c in A.CASES if all(getattr(c, key) == val for key, val in want.items())]
    assert out, want
    return out


def ids(cases):
    return [A.case_id(c) for c in cases]


# ---- running a case and applying the checks ---------------------------------------------------------------------------------------
RUNS = {}


def partial_bar(c, loss=None):
    """mur_step.BARS of the arithmetic the products phase runs in: split bf16 where k pads to 64 / 128 (Euclidean data only: the
    KL phases are the exact-f32 ones) or beyond 128 components, with the mode on."""
    loss = c.loss if loss is None else loss
    split = c.arith == "bf16" and (c.k > 128 or (c.k > 32 and loss == "eu"))
    return S.BARS[("bf16" if split else "f32", "eu")]


def family(c, cuts=None, form="rounds", fresh=False, **kw):
    """Case c over `cuts` (default: the ragged cuts of its row count): every step check at the case's bars, (a) - (d).
    Returns the FamilyRun (kept for the tests that compare two runs)."""
    cuts = cuts_of(c) if cuts is None else cuts
    key = (c, tuple(cuts), form, tuple(sorted(kw.items())))
    if key in RUNS and not fresh:
        return RUNS[key]
    kl_ao = c.family == "ao" and c.loss == "kl"
    bars = A.bars_ao_kl(c) if kl_ao else A.bars_of(c)
    run = X.run_family(c, cuts, form, **kw)
    tag = f"{A.case_id(c)} {form} over {list(cuts)} "
    v, w0, h0 = A.make_case(c)
    fails = []
    if kl_ao:
        A.check_ao_kl(c, run.states[0], run.states[1], bars["values"], fails, tag)
    else:
        fails += A.measure(c, run.states, record=True, bars=bars, tag=tag)[0]
    A.check_objectives(tag.strip(), c.loss, v, {0: (w0, h0), 1: (run.states[0].w, run.states[0].h), 2: (run.states[1].w, run.states[1].h)},
                       run.objs[0], fails)
    fails += X.family_common_failures(run, partial_bar(c))
    if any(fl != (0, -1, 3) for fl in run.flags):
        fails.append(f"states {run.flags}, expected (0, -1, 3) everywhere")
    assert not fails, tag + "\n" + "\n".join(fails)
    if not fresh:
        RUNS[key] = run
    return run


def same_bits(a, b, what):
    """Every readable array and word of two FamilyRuns' states, bit for bit."""
    fails = []
    for s, (sa, sb) in enumerate(zip(a, b), start=1):
        for name in ("w", "h", "w_aux", "h_aux", "dual_w", "dual_h"):
            x, y = getattr(sa, name), getattr(sb, name)
            if x is not None and not np.array_equal(x, y):
                fails.append(f"{what}: {name} behind step {s} differs in {int(np.sum(x != y))} elements")
        if tuple(sa.words) != tuple(sb.words):
            fails.append(f"{what}: inner words behind step {s}: {tuple(sa.words)} / {tuple(sb.words)}")
    return fails


# ---- ADMM ----------------------------------------------------------------------------------------------------------------------------
# Euclidean, 257 x 200 with the scaled row and column: one k per padding (kp 16, 32, 64, 128), both modes where k > 32, the prox
# pairs rotating as in admm_step.CASES: (l2n, l2n), (l1n, l2n), (l2n, l2n), (nn, nn)
ADMM_EU = [c for k in (12, 17, 40, 100) for c in pick(family="admm", loss="eu", m=257, k=k, edges=True)]
# the row-coupled operators on the H side (replicated work); tests/test_shard_family_bars.py proves their bars
ADMM_L1INF = list(X.ADMM_L1INF_CASES)
ADMM_COMPOSED = pick(family="admm", loss="eu", m=384, k=160, rho=1.0)
ADMM_KL = pick(family="admm", loss="kl", m=257)


@pytest.mark.parametrize("c", ADMM_EU + ADMM_L1INF + ADMM_COMPOSED, ids=ids(ADMM_EU + ADMM_L1INF + ADMM_COMPOSED))
def test_admm_eu(c):
    family(c)


@pytest.mark.parametrize("c", ADMM_KL, ids=ids(ADMM_KL))
def test_admm_kl(c):
    """The rank-local v_aux / dual_v of step 1 feed the products of step 2: its H half sums every shard's w_aux^T S."""
    family(c)


# ---- AO-ADMM, Euclidean ------------------------------------------------------------------------------------------------------------------
AO_ITERS = [c for k in (16, 40, 128) for c in pick(family="ao", loss="eu", m=257, k=k, edges=False)]       # admm_iter 1, 5 and 10 each
AO_EDGES = [c for k in (12, 17, 100) for c in pick(family="ao", loss="eu", m=257, k=k, edges=True)]       # the 2^12 row in the last shard
AO_COMPOSED = pick(family="ao", loss="eu", m=384, k=160)
AO_STOPS = list(A.PATH_CASES) + [X.LOCAL_STOP_CASE]
AO_WRAP = pick(family="ao", loss="eu", m=4161)
AO_FUSABLE = [c for c in AO_ITERS + AO_EDGES if c.admm_iter >= 2]


@pytest.mark.parametrize("c", AO_ITERS + AO_EDGES + AO_COMPOSED, ids=ids(AO_ITERS + AO_EDGES + AO_COMPOSED))
def test_aoadmm_eu_round_by_round(c):
    assert len({x.admm_iter for x in AO_ITERS}) == 3
    family(c, form="rounds")


@pytest.mark.parametrize("c", AO_FUSABLE, ids=ids(AO_FUSABLE))
def test_aoadmm_eu_fused(c):
    family(c, form="fused")


def words_of(run):
    return [tuple(st.words) for st in run.states]


@pytest.mark.parametrize("c", AO_STOPS, ids=ids(AO_STOPS))
def test_aoadmm_eu_stop_inside_the_w_rounds(c):
    """Warm starts whose W sub-problem stops inside its ten rounds, over cuts on which at least one shard's own norm sums would
    stop it at another round (the float64 reference restricted to the shard's rows says so first): every rank reports the count of
    the reference on ALL rows -- the step check compares the words with float64, (a) compares the ranks -- in both forms."""
    glob, local, clear = X.w_stop_rounds(c, CUTS70)
    assert any(r != glob for r in local) and clear >= A.STOP_CLEAR, (glob, local, clear)
    runs = {form: family(c, CUTS70, form) for form in X.AO_FORMS}
    for form, run in runs.items():
        for states in run.rank_states:
            assert all(tuple(st.words) == tuple(states[0].words) for st in states)
        assert run.states[0].words[1] == (glob | 1 << 16), (form, run.states[0].words, glob)
    assert words_of(runs["rounds"]) == words_of(runs["fused"])


def test_fused_refused_beyond_128_components():
    """The one form without a composed path: the library says so instead of running something else."""
    from nmf_amd import _lib as L
    with pytest.raises(L.NmfxError):
        X.run_family(AO_COMPOSED[0], CUTS384, "fused")


FUSED_VS_ROUNDS = [c for c in AO_FUSABLE if (c.k, c.admm_iter) in ((16, 5), (40, 10), (128, 5), (100, 10))]


@pytest.mark.parametrize("c", FUSED_VS_ROUNDS, ids=ids(FUSED_VS_ROUNDS))
def test_fused_against_round_by_round(c):
    """The same inner words, the same bars (family).  The H sub-problem of step 1 is the same launches on the same input in both
    forms: bit-identical.  The W rounds are different kernels (ao_fused_rows_kernel / the round kernel): no bit equality there."""
    a, b = family(c, form="rounds"), family(c, form="fused")
    assert words_of(a) == words_of(b)
    assert np.array_equal(a.states[0].h, b.states[0].h) and np.array_equal(a.states[0].dual_h, b.states[0].dual_h)


@pytest.mark.parametrize("form", X.AO_FORMS)
def test_norm_sums_wrap_inside_one_shard(form):
    """4161 x 72 over [0, 4100, 4161]: 65 blocks of 64 rows in the first shard (the lane-strided sums of the norm kernels wrap),
    one block in the second."""
    family(AO_WRAP[0], CUTS4161, form)


# ---- AO-ADMM, KL ------------------------------------------------------------------------------------------------------------------------
AO_KL = pick(family="ao", loss="kl", m=257) + pick(family="ao", loss="kl", m=384, k=160)


@pytest.mark.parametrize("c", AO_KL, ids=ids(AO_KL))
def test_aoadmm_kl(c):
    family(c)


# ---- ANLS ------------------------------------------------------------------------------------------------------------------------------
ANLS = [N.Case("cold", 257, 200, 16, "f32"), N.Case("zero", 257, 200, 29, "f32"), N.Case("mixed", 257, 200, 40, "f32"),
        N.Case("mixed", 257, 200, 40, "bf16"), N.Case("dead", 257, 200, 64, "bf16"), N.Case("mixed", 257, 200, 100, "bf16"),
        N.Case("settled", 257, 200, 128, "bf16"), N.Case("dead", 257, 200, 100, "bf16"), N.Case("mixed", 130, 120, 160, "bf16")]
ANLS_RUNS = {}


def anls(c, cuts=None, kinds=("eu", "kl"), fresh=False):
    """Case c over `cuts` with both recorded objectives: anls_step.check_steps at anls_step.bar_of(c) (check B in full for the
    first distance, for the second where its half-step inputs are bit-identical, as anls_step.run_case), (a) - (d)."""
    assert c in N.CASES
    cuts = cuts_of(c) if cuts is None else cuts
    key = (c, tuple(cuts), kinds)
    if key in ANLS_RUNS and not fresh:
        return ANLS_RUNS[key]
    v, w0, h0 = N.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = N.lam_of(c)
    cache, outs, fails = {}, {}, []
    for kind in kinds:
        out = outs[kind] = X.run_anls(c, cuts, kind)
        tag = f"{N.case_id(c)} {kind} over {list(cuts)} "
        try:
            N.check_steps(v, w0, h0, out.runs, lw, lh, N.bar_of(c), kind=kind, cache=cache, tag=tag,
                          skip_vars=N.DEAD_VARS if c.regime == "dead" else (), do_b=True if kind == kinds[0] else "cached")
        except AssertionError as e:
            fails.append(str(e))
        split = out.arith == "bf16" and 32 < c.k <= 128          # (beyond 128 components the phases run the exact-f32 products)
        fails += [tag + msg for msg in X.anls_common_failures(out, c, S.BARS[("bf16" if split else "f32", "eu")])]
        for s, flags in out.flags.items():
            if any(fl != (0, -1, s + 1) for fl in flags):
                fails.append(f"{tag}{s}-step run: states {flags}")
    assert not fails, "\n".join(fails)
    if not fresh:
        ANLS_RUNS[key] = outs
    return outs


@pytest.mark.parametrize("c", ANLS, ids=[N.case_id(c) for c in ANLS])
def test_anls(c):
    outs = anls(c)
    # the iterates are the least-squares ones whatever the recorded objective
    for s in (1, 2):
        assert np.array_equal(outs["eu"].runs[s].w, outs["kl"].runs[s].w) and np.array_equal(outs["eu"].runs[s].h, outs["kl"].runs[s].h)


# ---- a world of one through the driver against the plain handle, bit for bit ------------------------------------------------------------
def one(cases, **want):
    out = [c for c in cases if all(getattr(c, key) == val for key, val in want.items())]
    return out[0]


# (The KL losses at k <= 128 in f32 mode, as tests/test_gpu_admm_step.py::test_phase_protocol: the run entry points in split-bf16
#  mode keep v_aux / dual_v tile-major, the phase entry points -- exact f32 in either mode -- row-major, and a handle must not
#  change from one to the other without nmfx_set_factors in between: include/nmfx.h.)
WORLD_OF_ONE = [(one(ADMM_EU, k=40, arith="bf16"), "rounds"), (one(ADMM_KL, k=40, arith="f32"), "rounds"), (ADMM_COMPOSED[0], "rounds"),
                (one(AO_ITERS, k=40, admm_iter=5), "rounds"), (one(AO_ITERS, k=40, admm_iter=5), "fused"), (AO_COMPOSED[0], "rounds"),
                (one(AO_KL, k=40, arith="f32"), "rounds"), (one(AO_KL, k=160, arith="bf16"), "rounds")]


@pytest.mark.parametrize("c,form", WORLD_OF_ONE, ids=[f"{A.case_id(c)}-{form}" for c, form in WORLD_OF_ONE])
def test_world_of_one_equals_the_plain_handle(c, form):
    """Step 1 through the run entry point, step 2 through the phases with the poison and the host collective in between: what
    admm_step.run_device(phases=...) does on a plain handle without either."""
    run = family(c, [0, c.m], form, lead="run")
    dev = A.run_device(c, phases="fused" if form == "fused" else True, single=False)
    fails = same_bits(run.states, dev.states, "driver / plain handle")
    if not np.array_equal(run.objs[0], dev.objectives):
        fails.append(f"objective histories {run.objs[0]} / {dev.objectives}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("c", [ANLS[3], ANLS[8]], ids=lambda c: N.case_id(c))
def test_anls_world_of_one_equals_the_plain_handle(c):
    out = anls(c, [0, c.m], kinds=("eu",))["eu"]
    v, w0, h0 = N.make_case(c.regime, c.m, c.n, c.k)
    runs, _, w_mid = N.run_phases(v, w0, h0, *N.lam_of(c), "eu", c.arith if c.k <= 128 else None)
    assert np.array_equal(out.w_mid, w_mid)
    for s in (1, 2):
        assert np.array_equal(out.runs[s].w, runs[s].w) and np.array_equal(out.runs[s].h, runs[s].h)
        assert np.array_equal(out.runs[s].objectives, runs[s].objectives)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
TWICE = [(one(ADMM_KL, k=100, arith="bf16"), "rounds"), (one(AO_EDGES, k=100, arith="bf16"), "fused"), (one(AO_KL, k=40, arith="f32"), "rounds")]


@pytest.mark.parametrize("c,form", TWICE, ids=[f"{A.case_id(c)}-{form}" for c, form in TWICE])
def test_two_sharded_runs_bit_identical(c, form):
    a, b = family(c, form=form), family(c, form=form, fresh=True)
    fails = same_bits(a.states, b.states, "two identical runs")
    assert not fails and np.array_equal(a.objs[0], b.objs[0]), "\n".join(fails)


def test_two_sharded_anls_runs_bit_identical():
    a, b = anls(ANLS[5], kinds=("eu",))["eu"], anls(ANLS[5], kinds=("eu",), fresh=True)["eu"]
    for s in (1, 2):
        assert np.array_equal(a.runs[s].w, b.runs[s].w) and np.array_equal(a.runs[s].h, b.runs[s].h)
        assert np.array_equal(a.runs[s].objectives, b.runs[s].objectives)


# ---- what the split may change in W ------------------------------------------------------------------------------------------------------------
def row_deviation(wa, wb):
    """Largest |wa - wb| per row over the row's largest magnitude (the scale of the value checks: one problem per row)."""
    top = np.maximum(np.abs(wa).max(axis=1), np.abs(wb).max(axis=1))
    with np.errstate(all="ignore"):
        rel = np.abs(wa - wb).max(axis=1) / np.where(top > 0, top, 1.0)
    return np.where(np.isfinite(rel), rel, np.inf)


SPLIT = [(one(ADMM_EU, k=100, arith="bf16"), "rounds"), (one(AO_ITERS, k=128, admm_iter=10), "fused"), (one(AO_KL, k=100, arith="bf16"), "rounds")]


@pytest.mark.parametrize("c,form", SPLIT, ids=[f"{A.case_id(c)}-{form}" for c, form in SPLIT])
def test_the_split_moves_w_only_through_the_reduced_sums(c, form):
    """Rows of W are rank-local work: over [0, m] and over the ragged cuts the W of step 1 -- both from the same start, each
    within the case's value bar of the same float64 step -- differ by the f32 summation order of the reduced sums and of the
    shard's own products alone: within the value bar of each other, row by row."""
    whole, ragged = family(c, [0, c.m], form), family(c, form=form)
    bar = (A.bars_ao_kl(c) if (c.family, c.loss) == ("ao", "kl") else A.bars_of(c))["values"]
    rel = row_deviation(whole.states[0].w, ragged.states[0].w)
    S._record(f"{A.case_id(c)} {form} W_1 over [0, m] against the ragged cuts", float(rel.max()), bar)
    assert rel.max() <= bar, f"row {int(np.argmax(rel))}: {rel.max():.3e} > bar {bar:.2e}; {int(np.sum(rel > bar))} of {rel.size} rows"


def test_the_split_moves_anls_w_only_through_the_reduced_sums():
    """ANLS: W_1 depends on the start alone (no reduced sum in front of it), W_2 on the reduced W_1^T V and W_1^T W_1 through H_1."""
    c = ANLS[3]
    whole, ragged = anls(c, [0, c.m], kinds=("eu",))["eu"], anls(c, kinds=("eu",))["eu"]
    for s in (1, 2):
        rel = row_deviation(whole.runs[s].w, ragged.runs[s].w)
        S._record(f"{N.case_id(c)} W_{s} over [0, m] against the ragged cuts", float(rel.max()), N.bar_of(c))
        assert rel.max() <= N.bar_of(c), f"W_{s}, row {int(np.argmax(rel))}: {rel.max():.3e} > bar {N.bar_of(c):.2e}"
