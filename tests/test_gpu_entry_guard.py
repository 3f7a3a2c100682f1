"""What a handle derives from (W, H) in one call and trusts in the next (bf16 images, the KL epilogue's leftovers, the ANLS
objective pass's products, the relevances ...) is kept or voided by the entry guard of every compute entry point
(nmfx_internal.h, nmfx_enter).  Two properties per solver family, bit for bit, at k = 40 (pads to 64), k = 100 (pads to 128)
and k = 160 (the generic path):

  kept    two calls give what one call of the summed length gives;
  voided  a call sequence with a voiding event in the middle gives what a fresh handle started from the read-back state gives.

Runs only on a real MI355X (`-m gpu`); everything goes through the C ABI."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, N = 384, 320
RANKS = [40, 100, 160]
SMALL = [40, 100]          # weights, beta, ARD: k <= 128
NEVER = 10 ** 9
EU, KL, IS, BETA = 0, 1, 2, 3
T = (NEVER, 1e-3, 1e-3)


@functools.lru_cache(maxsize=None)
def inputs(k):
    rng = np.random.default_rng(7000 + k)
    v = rng.uniform(0.05, 1.0, (M, N)).astype(np.float32)
    w0 = rng.uniform(0.1, 1.0, (M, k)).astype(np.float32).astype(np.float64)
    h0 = rng.uniform(0.1, 1.0, (k, N)).astype(np.float32).astype(np.float64)
    om = (10.0 ** rng.uniform(-1.0, 1.0, (M, N))).astype(np.float32)
    for a in (v, w0, h0, om):
        a.setflags(write=False)
    return v, w0, h0, om


def handle(k, w, h, setup=None):
    from nmf_amd.engine import Engine
    eng = Engine(M, N, k)
    eng.upload_v(inputs(k)[0])
    if setup:
        setup(eng)
    eng.set_factors(w, h)
    return eng


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def mur(e, dist, first, count, lw=0.01, lh=0.02):
    e.mur_run(dist, lw, lh, NEVER, 1e-5, 1e-5, first, count)


# ---- kept: two calls equal one -----------------------------------------------------------------------------------------------
def split_equals_whole(k, run, setup=None, read=lambda e: e.get_factors()):
    _, w0, h0, _ = inputs(k)
    with handle(k, w0, h0, setup) as a:
        run(a, 0, 2)
        run(a, 2, 3)
        got = read(a)
    with handle(k, w0, h0, setup) as b:
        run(b, 0, 5)
        want = read(b)
    same(got, want)


@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("dist", [EU, KL])
def test_mur_two_calls_equal_one(k, dist):
    split_equals_whole(k, lambda e, first, count: mur(e, dist, first, count))


@pytest.mark.parametrize("k", SMALL)
def test_mur_beta_ard_two_calls_equal_one(k):
    def setup(e):
        e.set_beta(0.5)
        e.set_ard(0.1, 5.0, 1.0)
    split_equals_whole(k, lambda e, first, count: mur(e, BETA, first, count, 0.0, 0.0), setup,
                       read=lambda e: (*e.get_factors(), e.relevance()))


@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("dist", [EU, KL])
def test_aoadmm_two_calls_equal_one(k, dist):
    split_equals_whole(k, lambda e, first, count: e.aoadmm_run(dist, 1, 0.1, 1, 0.1, 5, *T, first, count))


@pytest.mark.parametrize("k", RANKS)
def test_admm_kl_two_calls_equal_one(k):
    split_equals_whole(k, lambda e, first, count: e.admm_run(KL, 1.0, 1, 0.1, 1, 0.1, *T, first, count))


@pytest.mark.parametrize("k", RANKS)
def test_anls_two_calls_equal_one(k):
    split_equals_whole(k, lambda e, first, count: e.anls_run(0.0, 0.01, *T, first, count))


# ---- voided: an event in the middle, against a fresh handle from the read-back factors ---------------------------------------
@pytest.mark.parametrize("k", RANKS)
def test_mur_kl_after_a_euclidean_iteration_equals_a_fresh_handle(k):
    """Three KL iterations, one Euclidean iteration (it voids the KL leftovers), three more KL iterations: the second leg starts
    at an even index, as the fresh handle's does, so both read W from the same buffer of the ping-pong."""
    _, w0, h0, _ = inputs(k)
    with handle(k, w0, h0) as a:
        mur(a, KL, 0, 3)
        mur(a, EU, 3, 1, 0.0, 0.0)
        w1, h1 = a.get_factors()
        mur(a, KL, 4, 3)
        got = a.get_factors()
    with handle(k, w1, h1) as b:
        mur(b, KL, 0, 3)
        want = b.get_factors()
    same(got, want)


@pytest.mark.parametrize("k", SMALL)
@pytest.mark.parametrize("ard", [False, True])
def test_mur_beta_after_set_beta_equals_a_fresh_handle(k, ard):
    _, w0, h0, _ = inputs(k)

    def setup(beta):
        def go(e):
            e.set_beta(beta)
            if ard:
                e.set_ard(0.1, 5.0, 1.0)
        return go
    lam = (0.0, 0.0) if ard else (0.01, 0.02)
    read = lambda e: (*e.get_factors(), e.relevance()) if ard else e.get_factors()
    with handle(k, w0, h0, setup(0.5)) as a:
        mur(a, BETA, 0, 2, *lam)
        a.set_beta(1.5)
        w1, h1 = a.get_factors()
        mur(a, BETA, 2, 2, *lam)
        got = read(a)
    with handle(k, w1, h1, setup(1.5)) as b:
        mur(b, BETA, 0, 2, *lam)
        want = read(b)
    same(got, want)


def precision_round_trip(e):
    e.set_precision("f32")
    e.set_precision("bf16")


def weights_round_trip(e):
    e.upload_weights(inputs(e.k)[3])
    e.clear_weights()


# (k = 40 with KL and k = 100 with either loss are left out: there the parent library is itself not bit-identical to a fresh handle --
#  neither setter voids kl_h_iter, so KL continues from the epilogue's partial sums where a fresh handle sums H afresh; why the
#  Euclidean loop at k = 100 differs was not traced (it carries by-products of its epilogues from one iteration to the next).
#  tools/entry_digest.py has those sequences: there parent = branch is what counts.  Per-entry weights need k <= 128.)
@pytest.mark.parametrize("k,dist,event", [(40, EU, "set_precision"), (40, EU, "weights"), (160, EU, "set_precision"), (160, KL, "set_precision")])
def test_mur_after_a_setter_equals_a_fresh_handle(k, dist, event):
    """Four iterations, set_precision there and back or upload_weights / clear_weights, three more (from an even index, like the
    fresh handle: the same buffer of the W ping-pong)."""
    _, w0, h0, _ = inputs(k)
    with handle(k, w0, h0) as a:
        mur(a, dist, 0, 4)
        (precision_round_trip if event == "set_precision" else weights_round_trip)(a)
        w1, h1 = a.get_factors()
        mur(a, dist, 4, 3)
        got = a.get_factors()
    with handle(k, w1, h1) as b:
        mur(b, dist, 0, 3)
        want = b.get_factors()
    same(got, want)


# (AO-ADMM and ADMM have no such test: a fresh handle given the read-back factors, duals and auxiliaries (nmfx_set_matrix) does not
#  reproduce the parent library's own continuation bit for bit at any k, with set_precision or the phase calls as the event: the
#  solvers carry state that cannot be read back -- the penalty and inverse of the last sub-problem, the m x n auxiliaries of the KL
#  forms.  Their keep sets are held by the "two calls equal one" tests above and by the digest.)


@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("event", ["anls_set_distance", "set_precision", "phase calls"])
def test_anls_after_a_voiding_event_equals_a_fresh_handle(k, event):
    _, w0, h0, _ = inputs(k)
    run = lambda e, first, count: e.anls_run(0.0, 0.01, *T, first, count)
    with handle(k, w0, h0) as a:
        run(a, 0, 2)
        j = 2
        if event == "anls_set_distance":
            a.anls_set_distance(KL)
            a.anls_set_distance(EU)
        elif event == "set_precision":
            precision_round_trip(a)
        else:
            a.anls_phase_objective(j)
            a.anls_phase_w(0.0, *T, j)
            a.anls_phase_h(0.01, j)
            j = 3
        w1, h1 = a.get_factors()
        run(a, j, 2)
        got = a.get_factors()
    with handle(k, w1, h1) as b:
        run(b, j, 2)
        want = b.get_factors()
    same(got, want)
