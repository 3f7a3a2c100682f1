"""CPU proof of the lock-step drivers of ADMM, AO-ADMM and ANLS (tests/shard_step.py: run_family, run_anls) and of the checks the
GPU test feeds with them (tests/test_gpu_shard_family_step.py), on the numpy stand-ins of tests/host_shard.py:

  * float64 stand-in shards over ragged cuts pass every step check of tests/admm_step.py / tests/anls_step.py far inside the
    bars, and the assertions (a) - (d) of the GPU test;
  * for a world of one the driver issues the phase calls nmf_amd.dist.admm_sharded / aoadmm_sharded / anls_sharded issue, call by
    call and argument by argument;
  * each planted fault -- a wrapper around one stand-in or around the collective -- is rejected, and the test names the check
    that rejects it;
  * the designated local-stop case has what it is for: a shard whose own norm sums stop the W sub-problem at another round."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import admm_step as A  # noqa: E402
import anls_step as N  # noqa: E402
import shard_step as X  # noqa: E402
from host_shard import HostShard  # noqa: E402
from nmf_amd import dist as nd  # noqa: E402

TIGHT = 1e-9                                    # "far inside": every bar of the device cases is 4 f32 ulps = 4.8e-7 or more
M, NCOL = 41, 30
CUTS = [0, 1, 9, 10, 30, 41]                    # two one-row shards among five
PROX = ("l1n", 0.05, "l1n", 0.05)
# warm starts with lambda = 0.5: the W sub-problem stops inside its ten rounds (8, then 9: admm_step.PATH_CASES)
STOPPING = A.PATH_CASES[0]
STOP_CUTS = X.LOCAL_STOP_CUTS
# ... and the case in which two shards' own sums stop one round before the sums over all rows do (test_local_stop_precondition)
LOCAL_STOP = X.LOCAL_STOP_CASE


def host_nodes(per_rank=None, log=None):
    def make(rank, v_local, k, w_local, h):
        shard = (per_rank or {}).get(rank, HostShard)(v_local, k, w_local, h)
        shard.rank = rank
        if log is not None:
            log.append(shard)
        return X.HostNode(shard)
    return make


def tight(c):
    return dict(values=TIGHT, residual=TIGHT)


def family_checks(c, run, rank=0, bars=None):
    """The step checks of the GPU test on the states of shard `rank`; returns the failures."""
    states = run.of_rank(rank)
    v, w0, h0 = A.make_case(c)
    fails = []
    if c.family == "ao" and c.loss == "kl":
        A.check_ao_kl(c, states[0], states[1], (bars or tight(c))["values"], fails, "", record=False)
    else:
        fails += A.measure(c, states, record=False, bars=bars or tight(c))[0]
    A.check_objectives("", c.loss, v, {0: (w0, h0), 1: (states[0].w, states[0].h), 2: (states[1].w, states[1].h)}, run.objs[rank], fails, record=False)
    return fails


FAMILY = [
    (A._admm("eu", M, NCOL, 4, "f32", 1.0, A.PROX_ROT[1], edges=True), "rounds"),
    (A._admm("eu", M, NCOL, 4, "f32", 2.0, A.PROX_ROT[2], edges=True), "rounds"),
    (A._admm("eu", M, NCOL, 4, "f32", 1.0, ("nn", 0.0, "l1inf", 0.05)), "rounds"),
    (A._admm("eu", M, NCOL, 4, "f32", 1.0, ("l1n", 0.05, "l1inf_transpose", 0.1)), "rounds"),
    (A._admm("kl", M, NCOL, 4, "f32", 1.0, A.PROX_ROT[1]), "rounds"),
    (A._ao("eu", M, NCOL, 4, "f32", 1, PROX, edges=True), "rounds"),
    (A._ao("eu", M, NCOL, 4, "f32", 5, PROX, edges=True), "rounds"),
    (A._ao("eu", M, NCOL, 4, "f32", 5, PROX, edges=True), "fused"),
    (A._ao("eu", M, NCOL, 4, "f32", 10, PROX), "fused"),
    (A._ao("kl", M, NCOL, 4, "f32", 5, PROX), "rounds"),
]
IDS = [f"{A.case_id(c)}-{form}" for c, form in FAMILY]


@pytest.mark.parametrize("c,form", FAMILY, ids=IDS)
def test_float64_shards_pass_every_check(c, form):
    run = X.run_family(c, CUTS, form, make_engine=host_nodes())
    assert run.arith == "f64"
    fails = X.family_common_failures(run, TIGHT)
    for rank in (0, 3):
        fails += family_checks(c, run, rank)
    assert not fails, "\n".join(fails)
    assert [fl for fl in run.flags] == [(0, -1, 3)] * 5


@pytest.mark.parametrize("c,cuts", [(STOPPING, STOP_CUTS), (A.PATH_CASES[1], STOP_CUTS), (LOCAL_STOP, STOP_CUTS)], ids=["warm2", "warm3", "local-stop"])
def test_fused_and_round_by_round_agree_where_the_stop_fires(c, cuts):
    runs = {form: X.run_family(c, cuts, form, make_engine=host_nodes()) for form in X.AO_FORMS}
    for form, run in runs.items():
        fails = X.family_common_failures(run, TIGHT) + family_checks(c, run)
        assert not fails, form + "\n" + "\n".join(fails)
    a, b = runs["rounds"].states, runs["fused"].states
    assert [st.words for st in a] == [st.words for st in b]
    assert any((wd & 0xFFFF) < c.admm_iter and wd >> 16 for st in a for wd in st.words[1:])         # the W stop fired early
    for s in (0, 1):
        np.testing.assert_allclose(a[s].w, b[s].w, rtol=1e-12, atol=1e-300)


def test_local_stop_precondition():
    """The float64 reference restricted to the rows of a shard: with its own sums alone shards 0 and 2 would stop the first W
    sub-problem at round 6, the sums over all rows stop it at round 7, every ratio ten times clearer of the tolerance than the
    step checks ask (admm_step.STOP_CLEAR)."""
    glob, local, clear = X.w_stop_rounds(LOCAL_STOP, STOP_CUTS)
    assert (glob, local) == (7, [6, 7, 6]) and clear >= 10 * A.STOP_CLEAR
    bars = A.bars_of(LOCAL_STOP)
    assert bars["stop_margin"] >= 10 * A.STOP_CLEAR and bars["counts"][1]["W"] == (7, True)
    for c in A.PATH_CASES:                                   # (the designated path cases over the same cuts have such a shard too)
        glob, local, _ = X.w_stop_rounds(c, STOP_CUTS)
        assert any(r != glob for r in local), (A.case_id(c), glob, local)


ANLS_CASES = [N.Case("cold", M, NCOL, 4, "f32"), N.Case("settled", M, NCOL, 5, "f32"), N.Case("mixed", M, NCOL, 6, "f32")]


@pytest.mark.parametrize("kind", ["eu", "kl"])
@pytest.mark.parametrize("c", ANLS_CASES, ids=[N.case_id(c) for c in ANLS_CASES])
def test_float64_anls_shards_pass_every_check(c, kind):
    out = X.run_anls(c, CUTS, kind, make_engine=host_nodes())
    v, w0, h0 = N.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = N.lam_of(c)
    fails = X.anls_common_failures(out, c, TIGHT)
    assert not fails, "\n".join(fails)
    N.check_steps(v, w0, h0, out.runs, lw, lh, 1e-8, kind=kind, skip_vars=N.DEAD_VARS if c.regime == "dead" else ())
    np.testing.assert_array_equal(out.w_mid, out.runs[1].w)


# ---- the sequence of phase calls, world of one -------------------------------------------------------------------------------------
PHASES = [name for name in dir(HostShard) if "_phase_" in name and not name.startswith("mur_")] + ["objective_partial", "mur_finish_b", "anls_set_distance", "set_factors"]


def recording():
    class Recorded(HostShard):
        def __init__(self, *args):
            super().__init__(*args)
            self.calls = []

        def set_l2n_operator(self, which, p):
            self.calls.append(("set_l2n_operator", which))
            return HostShard.set_l2n_operator(self, which, p)

    def wrap(name):
        def method(self, *args):
            self.calls.append((name,) + tuple(0 if name == "set_factors" else a for a in args))
            return getattr(HostShard, name)(self, *args)
        return method

    for name in PHASES:
        setattr(Recorded, name, wrap(name))
    return Recorded


class QuietComm:
    """A communicator for a world of one: a sum over one rank is the identity."""
    rank, world, stage = 0, 1, True

    def all_reduce(self, *tensors):
        pass


STOP = (X.NEVER, 1e-3, 1e-3)                    # (the product's loop prints with the digits of its tolerances: they cannot be 0)


def after_last_start(calls):
    last = max(i for i, call in enumerate(calls) if call[0] == "set_factors")
    return [call for call in calls[:last] if call[0] == "set_l2n_operator"] + calls[last + 1:]


@pytest.mark.parametrize("c,form", FAMILY, ids=IDS)
def test_driver_issues_the_calls_of_the_sharded_solvers(c, form):
    rec = recording()
    v, w0, h0 = A.make_case(c)
    ref = rec(v, c.k, w0, h0)
    kw = dict(distance_type=c.loss, reg_w=(c.lam_w, c.prox_w), reg_h=(c.lam_h, c.prox_h), min_iter=STOP[0], max_iter=2, tol1=STOP[1], tol2=STOP[2])
    if c.family == "admm":
        nd.admm_sharded(ref, QuietComm(), rho=c.rho, **kw)
    else:
        nd.aoadmm_sharded(ref, QuietComm(), admm_iter=c.admm_iter, fused=form == "fused", **kw)
    made = []
    run = X.run_family(c, [0, c.m], form, make_engine=host_nodes({0: rec}, made), stop=STOP)
    assert after_last_start(made[0].calls) == ref.calls
    assert len(ref.calls) >= 2 * 2 + 2
    np.testing.assert_array_equal(run.states[1].w, ref.w)
    np.testing.assert_array_equal(run.states[1].h, ref.h)
    np.testing.assert_array_equal(run.objs[0], ref.objectives(0, 3))


def test_fused_is_the_default_of_the_product_where_the_driver_runs_it():
    """dist.aoadmm_sharded chooses the fused W sub-problem on its own for 2 <= admm_iter <= 64 and k <= 128: the calls of
    form="fused" are those of the default."""
    c = FAMILY[7][0]
    rec = recording()
    v, w0, h0 = A.make_case(c)
    ref = rec(v, c.k, w0, h0)
    nd.aoadmm_sharded(ref, QuietComm(), admm_iter=c.admm_iter, distance_type="eu", reg_w=(c.lam_w, c.prox_w), reg_h=(c.lam_h, c.prox_h),
                      min_iter=STOP[0], max_iter=2, tol1=STOP[1], tol2=STOP[2])
    assert any(call[0] == "aoadmm_phase_w_fused" for call in ref.calls)


@pytest.mark.parametrize("kind", ["eu", "kl"])
def test_anls_driver_issues_the_calls_of_anls_sharded(kind):
    c = ANLS_CASES[0]
    rec = recording()
    v, w0, h0 = N.make_case(c.regime, c.m, c.n, c.k)
    lw, lh = N.lam_of(c)
    ref = rec(v, c.k, w0, h0)
    nd.anls_sharded(ref, QuietComm(), distance_type=kind, lambda_w=lw, lambda_h=lh, min_iter=STOP[0], max_iter=2, tol1=STOP[1], tol2=STOP[2])
    made = []
    out = X.run_anls(c, [0, c.m], kind, make_engine=host_nodes({0: rec}, made), steps=(2,), stop=STOP)
    assert after_last_start(made[0].calls) == ref.calls
    np.testing.assert_array_equal(out.runs[2].w, ref.w)
    np.testing.assert_array_equal(out.runs[2].objectives, ref.objectives(0, 3))


# ---- planted faults ----------------------------------------------------------------------------------------------------------------
# Each is run over ragged shards, the unfaulted run passes (the tests above), and the test names the check that rejects it.
class Collective(X.HostCollective):
    """HostCollective whose result for buffer `what` is replaced on chosen shards by mangle(parts, reduced, shard index)."""

    def __init__(self, what, mangle):
        self.what, self.mangle, self.seen = what, mangle, 0

    def all_reduce(self, bufs, a, b, what):
        if what != self.what:
            return super().all_reduce(bufs, a, b, what)
        parts = self._parts(bufs, a, b)
        acc = self.total(parts)
        for i, t in enumerate(bufs):
            self._put(t, a, self.mangle(parts, acc, i, self.seen))
        self.seen += 1


ADMM_C, AO_C, KL_C = FAMILY[0][0], FAMILY[6][0], FAMILY[4][0]


def rejected_by(c, run, rank=0, bars=None):
    """(messages of the common assertions, messages of the step checks)."""
    return X.family_common_failures(run, TIGHT), family_checks(c, run, rank, bars)


def test_fault_1_one_shard_solves_h_from_its_own_partial():
    """Shard 3 skips the f32 all-reduce.  Rejected by (a): its H differs from rank 0's; and by the H half of its own step check."""
    coll = Collective("x32", lambda parts, acc, i, t: parts[3] if i == 3 else acc)
    for c, form in ((ADMM_C, "rounds"), (AO_C, "rounds"), (KL_C, "rounds")):
        run = X.run_family(c, CUTS, form, make_engine=host_nodes(), collective=coll)
        common, own = rejected_by(c, run, rank=3)
        assert any(re.match(r"step 1: h of rank 3 differs from rank 0's", msg) for msg in common), common
        assert any(re.match(r"step 1 H \[(values|residual)", msg) for msg in own), own
        assert not family_checks(c, run, rank=0)[:0]
    out = X.run_anls(ANLS_CASES[0], CUTS, make_engine=host_nodes(), collective=coll)
    assert any("1-step run: H of rank 3 differs" in msg for msg in X.anls_ranks_differ(out))


def test_fault_2_w_stop_from_local_norm_sums():
    """Shard 0 decides from its own sums.  In the local-stop case it stops at round 6, the world at 7.  Rejected by (a): the inner
    words differ between the ranks; by the inner count of shard 0 against float64; and its rows of W miss the value bar."""
    coll = Collective("norms", lambda parts, acc, i, t: parts[0] if i == 0 else acc)
    run = X.run_family(LOCAL_STOP, STOP_CUTS, "rounds", make_engine=host_nodes(), collective=coll)
    common, own = rejected_by(LOCAL_STOP, run, rank=0)
    assert any("step 1: inner words of rank 1" in msg for msg in common), common
    assert any(re.match(r"step 1: rank 0 records the W word 6 rounds \(break bit 1\), the rank-order sums .* stop after 7", msg) for msg in common), common
    assert any(re.match(r"step 1 W \[inner count\]: the device ran 6 rounds \(break bit 1\), float64 7", msg) for msg in own), own
    assert any(re.match(r"step 1 W \[values, x\]: row [0-6] ", msg) for msg in own), own
    # the same fault through the speculative form: shard 0 reads its own table
    coll = Collective("table", lambda parts, acc, i, t: parts[0] if i == 0 else acc)
    run = X.run_family(LOCAL_STOP, STOP_CUTS, "fused", make_engine=host_nodes(), collective=coll)
    common, own = rejected_by(LOCAL_STOP, run, rank=0)
    assert any("inner words of rank 1" in msg for msg in common) and any("[inner count]" in msg for msg in own)
    # what the checks do NOT see: rank 1's own step check passes except for the stacked rows of shard 0 (the W rows are everybody's)
    assert not [msg for msg in family_checks(LOCAL_STOP, run, rank=1) if "[inner count]" in msg]


def test_fault_3_fused_table_row_shifted_by_one_round():
    """Every rank reads row r + 1 of the reduced table as row r.  All ranks agree, so (a) is blind; rejected by the stop re-derived
    from the noted tables (norm_decision_failures), by the inner count against float64 (the stop one round early) and by the
    values of W."""
    def shift(parts, acc, i, t):
        out = acc.copy()
        out[:-4] = acc[4:]
        return out
    coll = Collective("table", shift)
    run = X.run_family(STOPPING, STOP_CUTS, "fused", make_engine=host_nodes(), collective=coll)
    common, own = rejected_by(STOPPING, run)
    assert not [msg for msg in common if "inner words" in msg]                       # the blind spot of (a)
    assert sum("the rank-order sums of the noted norm sums stop after 8" in msg for msg in common if msg.startswith("step 1")) == 3, common
    assert any(re.match(r"step 1 W \[inner count\]: the device ran 7 rounds \(break bit 1\), float64 8", msg) for msg in own), own
    assert any(re.match(r"step 1 W \[values, x\]", msg) for msg in own), own


def test_fault_4_objective_partial_left_out():
    """Shard 2's partial misses from every objective sum.  Rejected by (b), entry by entry, and by check_objectives."""
    coll = Collective("x64", lambda parts, acc, i, t: X.HostCollective().total([p for r, p in enumerate(parts) if r != 2]))
    for c, form in ((ADMM_C, "rounds"), (FAMILY[8][0], "fused"), (KL_C, "rounds")):
        run = X.run_family(c, CUTS, form, make_engine=host_nodes(), collective=coll)
        common, own = rejected_by(c, run)
        assert [msg[:6] for msg in common if msg.startswith("obj[")] == ["obj[0]", "obj[1]", "obj[2]"], common
        assert sum(msg.startswith(" obj[") for msg in own) == 3, own
    # a blind spot of check_objectives that (b) closes: with the row of V scaled by 2^12 (edges of an AO-ADMM case) the one row of
    # shard 2 is 1e-7 of the objective, far below OBJ_RTOL -- the comparison with the float64 objective passes, the bit-exact sum does not
    run = X.run_family(AO_C, CUTS, "fused", make_engine=host_nodes(), collective=coll)
    common, own = rejected_by(AO_C, run)
    assert not [msg for msg in own if "obj[" in msg], own
    assert [msg[:6] for msg in common if msg.startswith("obj[")] == ["obj[0]", "obj[1]", "obj[2]"], common
    out = X.run_anls(ANLS_CASES[0], CUTS, make_engine=host_nodes(), collective=coll)
    fails = X.anls_common_failures(out, ANLS_CASES[0], TIGHT)
    assert sum("obj[" in msg for msg in fails) == 2 + 3, fails


def test_fault_5_norm_sums_of_the_round_before_reused():
    """Round r + 1 decides from the reduced sums of round r - 1 (the collective hands out the result before).  All ranks agree;
    rejected by the inner count against float64: the stop comes one round late."""
    keep = {}

    def stale(parts, acc, i, t):
        prev = keep.get(t - 1, acc)
        keep[t] = acc
        return prev
    run = X.run_family(STOPPING, STOP_CUTS, "rounds", make_engine=host_nodes(), collective=Collective("norms", stale))
    common, own = rejected_by(STOPPING, run)
    assert not [msg for msg in common if "inner words" in msg]
    assert any("step 1: rank 0 records the W word 9 rounds (break bit 1), the rank-order sums of the noted norm sums stop after 8" in msg for msg in common), common
    assert any(re.match(r"step 1 W \[inner count\]: the device ran 9 rounds \(break bit 1\), float64 8", msg) for msg in own), own


def test_fault_6_one_row_shard_added_twice():
    """The partial of the one-row shard 0 enters the f32 sum twice.  All ranks agree; rejected by the H half of the step check."""
    coll = Collective("x32", lambda parts, acc, i, t: acc + parts[0])
    for c, form in ((ADMM_C, "rounds"), (AO_C, "rounds")):
        run = X.run_family(c, CUTS, form, make_engine=host_nodes(), collective=coll)
        common, own = rejected_by(c, run)
        assert not [msg for msg in common if "differs" in msg]
        assert any(re.match(r"step 1 H \[(values|residual)", msg) for msg in own), own
    out = X.run_anls(ANLS_CASES[0], CUTS, make_engine=host_nodes(), collective=coll)
    v, w0, h0 = N.make_case("cold", M, NCOL, 4)
    with pytest.raises(AssertionError, match=r"H1 \[A, KKT\]"):
        N.check_steps(v, w0, h0, out.runs, *N.lam_of(ANLS_CASES[0]), 1e-8)


class StaleVaux(HostShard):
    """ADMM-KL: v_aux / dual_v advanced from the h_aux of the iteration before."""

    def admm_phase_update(self, kind, rho, prox_w, lam_w, prox_h, lam_h, min_iter, tol1, tol2, j):
        before = self.h_aux.copy()
        v_aux, dual_v = self.v_aux, self.dual_v
        super().admm_phase_update(kind, rho, prox_w, lam_w, prox_h, lam_h, min_iter, tol1, tol2, j)
        wh = self.w_aux @ before
        v_bar = wh - dual_v
        self.v_aux = 0.5 * ((v_bar - 1) + np.sqrt((v_bar - 1) ** 2 + 4 * self.v))
        self.dual_v = dual_v + self.v_aux - wh


def test_fault_7_admm_kl_auxiliaries_from_a_stale_h_aux():
    """On shard 3 (20 rows).  The auxiliaries are rank-local and cannot be read back: the ranks agree and step 1 passes; rejected
    by step 2 -- the H half (its right-hand side sums the shard's w_aux^T S) and the W half in the rows of that shard only."""
    run = X.run_family(KL_C, CUTS, make_engine=host_nodes({3: StaleVaux}))
    common, own = rejected_by(KL_C, run)
    assert not [msg for msg in common if "differs" in msg]
    assert not [msg for msg in own if msg.startswith("step 1")], own
    assert any(re.match(r"step 2 H \[(values|residual)", msg) for msg in own), own
    rows = [int(m.group(1)) for m in (re.match(r"step 2 W \[values, \w+\]: row (\d+) ", msg) for msg in own) if m]
    assert rows and all(10 <= r < 30 for r in rows), own


def test_fault_8_padding_of_a_partial_not_zero():
    """The stand-ins pad nothing, so the fault is planted on the snapshot: shard 1's buffer re-laid with k padded to 16 and n to
    128, one element of a padded factor row and one of the padded Gram columns set.  Rejected by (c), which counts them."""
    c = ADMM_C
    run = X.run_family(c, CUTS, make_engine=host_nodes())
    kp, np_ = 16, 128

    def padded(x, poke):
        prod = np.zeros((kp, np_))
        prod[:c.k, :c.n] = x[:c.k * c.n].reshape(c.k, c.n)
        gram = np.zeros((kp, kp))
        gram[:c.k, :c.k] = x[c.k * c.n:c.k * c.n + c.k * c.k].reshape(c.k, c.k)
        if poke:
            prod[c.k, 3] = 1e-30
            gram[0, c.k] = -0.0 + 1e-30
        return np.concatenate([prod.ravel(), gram.ravel()])

    v, w0, h0 = A.make_case(c)
    vv = np.asarray(v, dtype=np.float64)
    pairs = lambda a, b: (w0[a:b].T @ vv[a:b], w0[a:b].T @ w0[a:b])
    lays = [X.family_layout(kp, np_)] * len(run.snaps)
    clean = X.partial_failures([padded(x, False) for x in run.snaps], lays, run.cuts, c.k, c.n, pairs, TIGHT)
    assert clean == []
    fails = X.partial_failures([padded(x, i == 1) for i, x in enumerate(run.snaps)], lays, run.cuts, c.k, c.n, pairs, TIGHT)
    assert fails == ["rank 1 (rows 1 .. 8) partial: 2 elements of the padded factors / columns are not zero"]


class ReadsOwnPartial(HostShard):
    """A stand-in whose update reads the partial it wrote instead of the exchange buffer (what a phase reading `E->HHt` or
    `obj_part` instead of the reduced buffer would be): the poison is what catches it, whatever the values."""

    def admm_phase_products(self, *args):
        super().admm_phase_products(*args)
        self.own = self.x32.clone()

    def admm_phase_update(self, *args):
        self.x32.copy_(self.own)
        super().admm_phase_update(*args)


def test_a_phase_that_reads_its_own_partial_turns_the_checks_red():
    run = X.run_family(ADMM_C, CUTS, make_engine=host_nodes({2: ReadsOwnPartial}))
    common, own = rejected_by(ADMM_C, run, rank=2)
    assert any("step 1: h of rank 2 differs from rank 0's" in msg for msg in common), common
    assert any(msg.startswith("step 1 H [") for msg in own), own


def test_poison_reaches_what_nobody_wrote():
    """A stand-in that reads f64 [9] (the table of the fused W rounds, which no ADMM phase writes) into its objective: NaN in
    the history, named by (d)."""
    class ReadsSpare(HostShard):
        def admm_phase_update(self, *args):
            self.x64[0] = self.x64[0] + 0 * self.x64[9]
            super().admm_phase_update(*args)
    run = X.run_family(ADMM_C, CUTS, make_engine=host_nodes({1: ReadsSpare}))
    common = X.family_common_failures(run, TIGHT)
    assert any("objective history of rank 1" in msg and "not finite" in msg for msg in common), common


# ---- the cases the GPU test adds to admm_step.CASES ----------------------------------------------------------------------------------
USEFUL = 1e-2                                   # (a bar above this checks little; tests/test_admm_step_bars.py allows its table 5e-2)


@pytest.mark.parametrize("c", list(X.ADMM_L1INF_CASES) + [X.LOCAL_STOP_CASE], ids=A.case_id)
def test_added_cases_have_proven_bars(c):
    """What tests/test_admm_step_bars.py proves of every case of the table: the emulation passes at its own bars, the bars are
    useful, and every decision the step takes (inner stop, the row sums the l1inf operators test) is clear of its threshold."""
    b = A.bars_of(c)
    assert not b["emu_fails"], "\n".join(b["emu_fails"])
    assert b["values"] <= USEFUL and b["residual"] <= USEFUL and b["emu_tie"] <= A.TIE_ULPS / 2
    assert b["stop_margin"] >= A.STOP_CLEAR and b["l1inf_margin"] >= A.L1INF_CLEAR
    fails, _, _ = A.measure(c, A.emulate(c), bars=b)
    assert not fails, "\n".join(fails)
    if c.family == "admm":
        assert c.prox_w not in ("l1inf", "l1inf_transpose") and c.prox_h in ("l1inf", "l1inf_transpose")
