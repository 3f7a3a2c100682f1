"""Digest of what the C entry points compute and refuse, call by call: one line per step.

    python tools/entry_digest.py > digest.txt              # one line per step
    python tools/entry_digest.py --sections > digest.txt   # one line per section: the SHA-256 of its step lines (what is committed)
    python tools/entry_digest.py --fold digest.txt         # the second form from a file in the first

Every section opens one handle on a seeded 384 x 320 problem and makes a sequence of calls through the C ABI; after each call
that was accepted it prints the SHA-256 of W, of H and of the objectives recorded so far, after each call that was refused the
return code and the text of nmfx_last_error.  The sections are run at k = 40 (pads to 64), k = 100 (pads to 128) and k = 160
(the generic path) and walk the places where an entry point keeps or voids what the handle derived from (W, H) in an earlier
call: MUR-KL in two calls, with a Euclidean iteration in between, the phase calls behind a run, IS then KL, beta with and
without weights, ARD, fold-in, a precision switch, pair mode, a masked sparse handle; AO-ADMM (both losses) in two calls and
through the row-sharded phase calls; ADMM-KL in two calls; ANLS with a change of the reported distance and through its phase
calls.  Behind them (admm_step_sections) the ADMM family by the steps its runs and its row-sharded phase entry points share,
also at k = 12 (pads to 16): ADMM with either loss in runs and phase calls, with every prox operator (l2n through a seeded
operator, and once without it), AO-ADMM in exact f32, with prox 'l1inf', with the speculative W rounds (phase_w_fused /
phase_w_repair), and the Euclidean AO-ADMM once at k = 520 on a 640 x 576 problem (more than 512 padded components).  The
refusal sections make the refused calls: every compute entry point without V, without factors, with weights present, with ARD
set, with NMFX_BETA, behind another solver family, with two refusals applying at once, and -- one at a time -- between
the calls of a MUR-KL run and of an AO-ADMM run.  Last (hals_sections) the least-squares family behind ANLS: HALS runs at
sweeps 1 and 3 in both arithmetic modes with a change of the reported distance; stacked HALS at k = 40 and k = 100 (a stack that
fills the handle and one of ranks 3, 5, 8 that leaves components unowned) through set, terms, runs with differing lambdas, finish
and the per-problem getters; sparse HALS; and the hals entry points refused: without V, without a stack, behind another family,
with j < 0, sweeps = 0, sweeps = 17, a negative lambda.  Behind those (hals_variant_sections) hals_wide and hals_sparse_wide at
k = 160, masked HALS at k = 40 and the HALS fold-in on sparse, masked and dense handles with its sweep counts, under caps of 3 and
40 sweeps.

Two builds that print the same lines keep and void the same things and refuse in the same order: the file is what a change of
the host code between the ABI and the kernels that is meant to change nothing is checked against.  The script uses
nmf_amd.engine.Engine and nmf_amd._lib only, so it runs unmodified in a checkout of another commit; all sections run in one
process."""
import ctypes as C
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NMF_AMD_QUIET", "1")

import numpy as np

NEVER = 10 ** 12
M, N = 384, 320
RANKS = (40, 100, 160)
ONLY = os.environ.get("ENTRY_DIGEST_ONLY", "")          # substring of the section names to run (a shorter trace)
LINES = None                                            # --sections: the step lines are collected here, not printed


def emit(text):
    if LINES is None:
        print(text, flush=True)
    else:
        LINES.append(text)


def fold(lines):
    """One line per section (the lines that share "<name> k=<rank>"): how many step lines, and the SHA-256 of them."""
    sections = {}
    for ln in lines:
        sections.setdefault(re.match(r"\S+ k=\d+", ln).group(0), []).append(ln)
    for name, sec in sections.items():
        print(f"{name:<26} lines={len(sec):<4} {hashlib.sha256(''.join(x + chr(10) for x in sec).encode()).hexdigest()}")


def make_inputs(k, seed, shape=(M, N), scale=1.0):
    M, N = shape
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 1.0, (M, N)).astype(np.float32)
    w0 = (scale * rng.uniform(0.1, 1.0, (M, k))).astype(np.float32).astype(np.float64)
    h0 = (scale * rng.uniform(0.1, 1.0, (k, N))).astype(np.float32).astype(np.float64)
    om = (10.0 ** rng.uniform(-2.0, 2.0, (M, N))).astype(np.float32)
    om[rng.random((M, N)) < 0.1] = 0
    mask = rng.random((M, N)) < 0.7
    mask[0, 0] = True
    return v, w0, h0, om, mask


def sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:32]


class Section:
    """One handle; step() makes a call and prints what it left or how it was refused."""

    def __init__(self, name, eng, pair_ranks=None):
        self.name, self.eng, self.pair_ranks = name, eng, pair_ranks

    def line(self, label, text):
        emit(f"{self.name:<22} {label:<26} {text}")

    def step(self, label, call, pair=False):
        from nmf_amd._lib import NmfxError
        try:
            call()
            if pair:
                parts = []
                for p, kp in enumerate(self.pair_ranks):
                    w, h = self.eng.pair_get_factors(p, kp)
                    obj = self.eng.pair_objectives(p, 0, self.eng.pair_state(p)[2])
                    parts.append(f"W{p}={sha(w)} H{p}={sha(h)} obj{p}={sha(obj)} n={obj.size}")
                self.line(label, " ".join(parts))
                return
            w, h = self.eng.get_factors()
            n_obj = self.eng.state()[2]
            obj = self.eng.objectives(0, n_obj)
            self.line(label, f"W={sha(w)} H={sha(h)} obj={sha(obj)} n={n_obj}")
        except NmfxError as e:
            self.line(label, f"refused {e.code}: {str(e).split(': ', 1)[1]}")


def dense(name, k, v, w0, h0, body, **kw):
    from nmf_amd.engine import Engine
    if ONLY and ONLY not in name:
        return
    with Engine(v.shape[0], v.shape[1], k) as eng:
        s = Section(f"{name} k={k}", eng, **kw)
        eng.upload_v(v)
        eng.set_factors(w0, h0)
        body(s, eng)


def mur_sections(k, v, w0, h0, om, mask):
    from nmf_amd import _lib as L
    from nmf_amd import masked
    from nmf_amd.engine import Engine
    EU, KL, IS, BETA = L.EU, L.KL, L.IS, L.BETA
    run = lambda e, d, first, count, lw=0.01, lh=0.02: e.mur_run(d, lw, lh, NEVER, 1e-5, 1e-5, first, count)
    fin = lambda e, d, done: e.mur_finish(d, NEVER, 1e-5, 1e-5, done)

    def kl_two_calls(s, e):
        s.step("kl run 0..1", lambda: run(e, KL, 0, 2))
        s.step("kl run 2..4", lambda: run(e, KL, 2, 3))
        s.step("kl finish 5", lambda: fin(e, KL, 5))
    dense("mur/kl-kl", k, v, w0, h0, kl_two_calls)

    def kl_eu_kl(s, e):
        s.step("kl run 0..2", lambda: run(e, KL, 0, 3))
        s.step("eu run 3", lambda: run(e, EU, 3, 1, 0.0, 0.0))
        s.step("kl run 4..5", lambda: run(e, KL, 4, 2))
        s.step("kl finish 6", lambda: fin(e, KL, 6))
    dense("mur/kl-eu-kl", k, v, w0, h0, kl_eu_kl)

    def eu_phases(s, e):
        s.step("eu run 0..1", lambda: run(e, EU, 0, 2))
        s.step("eu phase_a 2", lambda: e.mur_phase_a(EU, 0.01, 2))
        s.step("eu phase_b 2", lambda: e.mur_phase_b(EU, 0.02, NEVER, 1e-5, 1e-5, 2))
        s.step("kl phase_a 3", lambda: e.mur_phase_a(KL, 0.01, 3))
        s.step("kl phase_b 3", lambda: e.mur_phase_b(KL, 0.02, NEVER, 1e-5, 1e-5, 3))
        s.step("eu finish_a 4", lambda: e.mur_finish_a(EU, 4))
        s.step("finish_b 4", lambda: e.mur_finish_b(NEVER, 1e-5, 1e-5, 4))
    dense("mur/eu-phases", k, v, w0, h0, eu_phases)

    def is_kl(s, e):
        s.step("is run 0..1", lambda: run(e, IS, 0, 2))
        s.step("kl run 2..3", lambda: run(e, KL, 2, 2))
        s.step("kl finish 4", lambda: fin(e, KL, 4))
    dense("mur/is-kl", k, v, w0, h0, is_kl)

    def beta(s, e):
        s.step("set_beta 0.5", lambda: e.set_beta(0.5))
        s.step("beta run 0..1", lambda: run(e, BETA, 0, 2))
        s.step("set_beta 1.5", lambda: e.set_beta(1.5))
        s.step("beta run 2..3", lambda: run(e, BETA, 2, 2))
        s.step("beta finish 4", lambda: fin(e, BETA, 4))
        s.step("upload_weights", lambda: e.upload_weights(om))
        s.step("beta run 4..5", lambda: run(e, BETA, 4, 2))
        s.step("kl run 6..7", lambda: run(e, KL, 6, 2))
        s.step("clear_weights", e.clear_weights)
        s.step("kl run 8..9", lambda: run(e, KL, 8, 2))
        s.step("kl finish 10", lambda: fin(e, KL, 10))
    dense("mur/beta-weights", k, v, w0, h0, beta)

    def ard(s, e):
        s.step("set_beta 0.5", lambda: e.set_beta(0.5))
        s.step("set_ard", lambda: e.set_ard(0.1, 5.0, 1.0))
        s.step("set_factors", lambda: e.set_factors(w0, h0))
        s.step("beta run 0..1", lambda: run(e, BETA, 0, 2, 0.0, 0.0))
        s.step("relevance", lambda: s.line("  relevance", sha(e.relevance())))
        s.step("set_beta 1.0", lambda: e.set_beta(1.0))
        s.step("beta run 2..3", lambda: run(e, BETA, 2, 2, 0.0, 0.0))
        s.step("beta finish 4", lambda: fin(e, BETA, 4))
        s.step("relevance", lambda: s.line("  relevance", sha(e.relevance())))
        s.step("clear_ard", e.clear_ard)
        s.step("beta run 4..5", lambda: run(e, BETA, 4, 2))
    dense("mur/ard", k, v, w0, h0, ard)

    def foldin(s, e):
        s.step("kl foldin 0..1", lambda: e.foldin_run(KL, 0.02, NEVER, 1e-5, 1e-5, 0, 2))
        s.step("kl foldin finish", lambda: e.foldin_finish(KL, NEVER, 1e-5, 1e-5, 2))
        s.step("kl run (no set_factors)", lambda: run(e, KL, 2, 2))
        s.step("set_factors", lambda: e.set_factors(*e.get_factors()))
        s.step("kl run 0..1", lambda: run(e, KL, 0, 2))
        s.step("kl finish 2", lambda: fin(e, KL, 2))
    dense("mur/foldin", k, v, w0, h0, foldin)

    def precision(s, e):
        s.step("kl run 0..1", lambda: run(e, KL, 0, 2))
        s.step("set_precision f32", lambda: e.set_precision("f32"))
        s.step("kl run 2..3", lambda: run(e, KL, 2, 2))
        s.step("set_precision bf16", lambda: e.set_precision("bf16"))
        s.step("kl run 4..5", lambda: run(e, KL, 4, 2))
        s.step("eu run 6..7", lambda: run(e, EU, 6, 2))
        s.step("set_precision f32", lambda: e.set_precision("f32"))
        s.step("eu run 8..9", lambda: run(e, EU, 8, 2))
        s.step("eu finish 10", lambda: fin(e, EU, 10))
    dense("mur/precision", k, v, w0, h0, precision)

    def pair(s, e):
        two = lambda a, b: (a, b)
        s.step("pair run 0..1", lambda: e.mur_pair_run(two(0.0, 0.05), two(0.1, 0.0), NEVER, 1e-5, 1e-5, 0, 2), pair=True)
        s.step("pair run 2..3", lambda: e.mur_pair_run(two(0.0, 0.05), two(0.1, 0.0), NEVER, 1e-5, 1e-5, 2, 2), pair=True)
        s.step("pair finish 4", lambda: e.mur_pair_finish(NEVER, 1e-5, 1e-5, 4), pair=True)
        s.step("eu run behind the pair", lambda: run(e, EU, 4, 2))
        s.step("set_factors", lambda: e.set_factors(w0, h0))
        s.step("eu run 0..1", lambda: run(e, EU, 0, 2))
        s.step("pair run behind it", lambda: e.mur_pair_run(two(0.0, 0.05), two(0.1, 0.0), NEVER, 1e-5, 1e-5, 2, 2), pair=True)
        s.step("eu finish 2", lambda: fin(e, EU, 2))
    dense("mur/pair", k, v, w0, h0, pair, pair_ranks=(min(k, 64), max(1, min(k - 64, 64))))

    if k <= 128 and not (ONLY and ONLY not in "mur/masked"):
        with Engine.for_sparse(masked.observed(v.astype(np.float64), mask, k), k, masked=True) as e:
            s = Section(f"mur/masked k={k}", e)
            e.set_factors(w0, h0)
            s.step("kl run 0..1", lambda: run(e, KL, 0, 2))
            s.step("eu run 2", lambda: run(e, EU, 2, 1))
            s.step("kl run 3..4", lambda: run(e, KL, 3, 2))
            s.step("is run 5..6", lambda: run(e, IS, 5, 2))
            s.step("is finish 7", lambda: fin(e, IS, 7))
            s.step("anls_run", lambda: e.anls_run(0.0, 0.0, NEVER, 1e-3, 1e-3, 0, 1))


def admm_family_sections(k, v, w0, h0, f32=False, losses=("eu", "kl")):
    """f32: the AO-ADMM two-calls and phases bodies only, behind set_precision('f32') (sections "<name>-f32"); one loss: those two
    bodies of that loss only."""
    from nmf_amd import _lib as L
    T = (NEVER, 1e-3, 1e-3)
    tag = "-f32" if f32 else ""
    for dist, dn in ((L.EU, "eu"), (L.KL, "kl")):
        if dn not in losses:
            continue

        def two_calls(s, e):
            if f32:
                s.step("set_precision f32", lambda: e.set_precision("f32"))
            s.step("run 0..1", lambda: e.aoadmm_run(dist, 1, 0.1, 1, 0.1, 5, *T, 0, 2))
            s.step("run 2..3", lambda: e.aoadmm_run(dist, 1, 0.1, 1, 0.1, 5, *T, 2, 2))
            s.step("finish 4", lambda: e.aoadmm_finish(*T, 4))
        dense(f"aoadmm-{dn}/two-calls{tag}", k, v, w0, h0, two_calls)

        def other_loss(s, e):
            s.step("run 0..1", lambda: e.aoadmm_run(dist, 1, 0.1, 1, 0.1, 5, *T, 0, 2))
            s.step("other loss 2", lambda: e.aoadmm_run(L.KL if dist == L.EU else L.EU, 1, 0.1, 1, 0.1, 5, *T, 2, 1))
            s.step("run 3..4", lambda: e.aoadmm_run(dist, 1, 0.1, 1, 0.1, 5, *T, 3, 2))
            s.step("finish 5", lambda: e.aoadmm_finish(*T, 5))
        if not f32 and len(losses) == 2:
            dense(f"aoadmm-{dn}/other-loss", k, v, w0, h0, other_loss)

        def phases(s, e):
            if f32:
                s.step("set_precision f32", lambda: e.set_precision("f32"))
            s.step("run 0..1", lambda: e.aoadmm_run(dist, 1, 0.1, 1, 0.1, 5, *T, 0, 2))
            j = 2
            if dist == L.EU:
                s.step("h_products 2", lambda: e.aoadmm_phase_h_products(j))
                s.step("h_solve 2", lambda: e.aoadmm_phase_h_solve(1, 0.1, 5, *T, j))
                s.step("w_products 2", lambda: e.aoadmm_phase_w_products(*T, j))
                for r in range(5):
                    s.step(f"w_round {r}", lambda: e.aoadmm_phase_w_round(1, 0.1, r))
                s.step("w_close 2", lambda: e.aoadmm_phase_w_close(5, j))
            else:
                for r in range(5):
                    s.step(f"kl h_products 2/{r}", lambda: e.aoadmm_kl_phase_h_products(j, r))
                    s.step(f"kl h_round 2/{r}", lambda: e.aoadmm_kl_phase_h_round(1, 0.1, r, *T, j))
                s.step("kl h_close 2", lambda: e.aoadmm_kl_phase_h_close(5, *T, j))
                for r in range(5):
                    s.step(f"kl w_round {r}", lambda: e.aoadmm_kl_phase_w_round(1, 0.1, r))
                s.step("kl w_close 2", lambda: e.aoadmm_kl_phase_w_close(5, j))
            s.step("run 3", lambda: e.aoadmm_run(dist, 1, 0.1, 1, 0.1, 5, *T, 3, 1))
            s.step("objective_partial", e.objective_partial)
            s.step("finish_b 4", lambda: e.mur_finish_b(*T, 4))
        dense(f"aoadmm-{dn}/phases{tag}", k, v, w0, h0, phases)
    if f32 or len(losses) < 2:
        return

    def admm_kl(s, e):
        s.step("kl run 0..1", lambda: e.admm_run(L.KL, 1.0, 1, 0.1, 1, 0.1, *T, 0, 2))
        s.step("kl run 2..3", lambda: e.admm_run(L.KL, 1.0, 1, 0.1, 1, 0.1, *T, 2, 2))
        s.step("eu run 4", lambda: e.admm_run(L.EU, 1.0, 1, 0.1, 1, 0.1, *T, 4, 1))
        s.step("kl products 5", lambda: e.admm_phase_products(L.KL, 1.0, 1, 1, 5))
        s.step("kl update 5", lambda: e.admm_phase_update(L.KL, 1.0, 1, 0.1, 1, 0.1, *T, 5))
        s.step("kl run 6", lambda: e.admm_run(L.KL, 1.0, 1, 0.1, 1, 0.1, *T, 6, 1))
        s.step("finish 7", lambda: e.aoadmm_finish(*T, 7))
    dense("admm/kl", k, v, w0, h0, admm_kl)

    def anls(s, e):
        s.step("run 0..1", lambda: e.anls_run(0.0, 0.01, *T, 0, 2))
        s.step("set_distance kl", lambda: e.anls_set_distance(L.KL))
        s.step("run 2..3", lambda: e.anls_run(0.0, 0.01, *T, 2, 2))
        s.step("set_distance eu", lambda: e.anls_set_distance(L.EU))
        s.step("run 4..5", lambda: e.anls_run(0.0, 0.01, *T, 4, 2))
        s.step("phase_objective 6", lambda: e.anls_phase_objective(6))
        s.step("phase_w 6", lambda: e.anls_phase_w(0.0, *T, 6))
        s.step("phase_h 6", lambda: e.anls_phase_h(0.01, 6))
        s.step("run 7", lambda: e.anls_run(0.0, 0.01, *T, 7, 1))
        s.step("objective_partial", e.objective_partial)
        s.step("finish_b 8", lambda: e.mur_finish_b(*T, 8))
    dense("anls", k, v, w0, h0, anls)


def admm_step_sections(k, v, w0, h0):
    """What the run loops and the row-sharded phase entry points of ADMM and AO-ADMM share, on the paths the sections above do not
    reach: ADMM with either loss and every prox operator, exact-f32 runs, prox 'l1inf' inside AO-ADMM, the speculative W rounds."""
    from nmf_amd import _lib as L
    T = (NEVER, 1e-3, 1e-3)
    NN, L1N, L2N, L1INF, L1INF_T = (L.PROX[p] for p in ("nn", "l1n", "l2n", "l1inf", "l1inf_transpose"))
    rng = np.random.default_rng(7000 + k)
    a = rng.standard_normal((k, k))
    op = a @ a.T / k + np.eye(k)                     # symmetric positive definite: stands in for ((lambda T^T T + rho I) / rho)^-1

    for dist, dn in ((L.EU, "eu"), (L.KL, "kl")):
        for f32 in (False, True):
            def admm(s, e):
                run = lambda first, count: e.admm_run(dist, 1.0, L1N, 0.1, L1N, 0.1, *T, first, count)
                if f32:
                    s.step("set_precision f32", lambda: e.set_precision("f32"))
                s.step("run 0..1", lambda: run(0, 2))
                s.step("run 2..3", lambda: run(2, 2))
                s.step("products 4", lambda: e.admm_phase_products(dist, 1.0, L1N, L1N, 4))
                s.step("update 4", lambda: e.admm_phase_update(dist, 1.0, L1N, 0.1, L1N, 0.1, *T, 4))
                s.step("run 5", lambda: run(5, 1))
                s.step("finish 6", lambda: e.aoadmm_finish(*T, 6))
            dense(f"admm/{dn}-steps" + ("-f32" if f32 else ""), k, v, w0, h0, admm)

        def admm_prox(s, e):
            s.step("l2n without operator", lambda: e.admm_run(dist, 1.0, L2N, 0.1, L1INF, 0.1, *T, 0, 2))
            s.step("set_l2n_operator w", lambda: e.set_l2n_operator(0, op))
            s.step("set_l2n_operator h", lambda: e.set_l2n_operator(1, op))
            for pw, ph in ((L2N, L1INF), (L1INF_T, L2N), (L1N, L2N)):
                s.step("set_factors", lambda: e.set_factors(w0, h0))
                s.step(f"run 0..1 prox {pw},{ph}", lambda: e.admm_run(dist, 1.0, pw, 0.1, ph, 0.1, *T, 0, 2))
                s.step(f"products 2 prox {pw},{ph}", lambda: e.admm_phase_products(dist, 1.0, pw, ph, 2))
                s.step(f"update 2 prox {pw},{ph}", lambda: e.admm_phase_update(dist, 1.0, pw, 0.1, ph, 0.1, *T, 2))
                s.step(f"run 3 prox {pw},{ph}", lambda: e.admm_run(dist, 1.0, pw, 0.1, ph, 0.1, *T, 3, 1))
            s.step("finish 4", lambda: e.aoadmm_finish(*T, 4))
        dense(f"admm-{dn}/prox", k, v, w0, h0, admm_prox)

        def ao_l1inf(s, e):
            for pw, ph in ((L1INF, L1N), (L1N, L1INF), (L1INF_T, L1N), (L1N, L1INF_T)):
                s.step("set_factors", lambda: e.set_factors(w0, h0))
                s.step(f"run 0..1 prox {pw},{ph}", lambda: e.aoadmm_run(dist, pw, 0.1, ph, 0.1, 4, *T, 0, 2))
                s.step(f"run 2 prox {pw},{ph}", lambda: e.aoadmm_run(dist, pw, 0.1, ph, 0.1, 4, *T, 2, 1))
                s.step("finish 3", lambda: e.aoadmm_finish(*T, 3))
        dense(f"aoadmm-{dn}/l1inf", k, v, w0, h0, ao_l1inf)

    def w_fused(s, e):
        s.step("run 0..1", lambda: e.aoadmm_run(L.EU, 1, 0.1, 1, 0.1, 5, *T, 0, 2))
        s.step("h_products 2", lambda: e.aoadmm_phase_h_products(2))
        s.step("h_solve 2", lambda: e.aoadmm_phase_h_solve(1, 0.1, 5, *T, 2))
        s.step("w_products 2", lambda: e.aoadmm_phase_w_products(*T, 2))
        s.step("w_fused", lambda: e.aoadmm_phase_w_fused(1, 0.1, 5))
        s.step("w_repair 2", lambda: e.aoadmm_phase_w_repair(1, 0.1, 5, 2))
        s.step("run 3", lambda: e.aoadmm_run(L.EU, 1, 0.1, 1, 0.1, 5, *T, 3, 1))
        s.step("finish 4", lambda: e.aoadmm_finish(*T, 4))
    if k <= 128:
        dense("aoadmm-eu/w-fused", k, v, w0, h0, w_fused)
    admm_family_sections(k, v, w0, h0, f32=True)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def entry_points(lib, h, dist, j):
    """Every compute entry point as a raw ABI call with loss `dist` and iteration index `j`, by family."""
    i64, dbl, i32 = C.c_int64(), C.c_double(), C.c_int()
    two = (C.c_double * 2)(0.0, 0.0)
    u, s, vt = np.empty((M, 4)), np.empty(4), np.empty((4, N))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    T = (NEVER, 0.0, 0.0)
    mur = {
        "mur_run": lambda: lib.nmfx_mur_run(h, dist, 0.0, 0.0, *T, j, 1),
        "mur_finish": lambda: lib.nmfx_mur_finish(h, dist, *T, j),
        "foldin_run": lambda: lib.nmfx_foldin_run(h, dist, 0.0, *T, j, 1),
        "foldin_finish": lambda: lib.nmfx_foldin_finish(h, dist, *T, j),
        "mur_phase_a": lambda: lib.nmfx_mur_phase_a(h, dist, 0.0, j),
        "mur_phase_b": lambda: lib.nmfx_mur_phase_b(h, dist, 0.0, *T, j),
        "mur_finish_a": lambda: lib.nmfx_mur_finish_a(h, dist, j),
        "mur_phase_a_head": lambda: lib.nmfx_mur_phase_a_head(h, dist, 0.0, j),
        "mur_phase_b_slice": lambda: lib.nmfx_mur_phase_b_slice(h, dist, 0.0, *T, j, 0, 64),
        "mur_phase_b_rest": lambda: lib.nmfx_mur_phase_b_rest(h, dist, 0, 64),
        "mur_run_sharded": lambda: lib.nmfx_mur_run_sharded(h, dist, 0.0, 0.0, *T, j, 1),
        "mur_finish_sharded": lambda: lib.nmfx_mur_finish_sharded(h, dist, *T, j),
        "mur_pair_run": lambda: lib.nmfx_mur_pair_run(h, two, two, *T, j, 1),
        "mur_pair_finish": lambda: lib.nmfx_mur_pair_finish(h, *T, j),
    }
    no_index = {      # (entry points without an iteration index: accepted where only the index is wrong)
        "profile_repeat": lambda: lib.nmfx_profile_repeat(h, b"wphase", dist, 1, C.byref(dbl)),
        "aoadmm_phase_w_round": lambda: lib.nmfx_aoadmm_phase_w_round(h, 1, 0.1, 0),
        "aoadmm_kl_phase_w_round": lambda: lib.nmfx_aoadmm_kl_phase_w_round(h, 1, 0.1, 0),
    }
    info = {          # (accepted without V: they launch nothing and describe the handle)
        "mur_chunk_info": lambda: lib.nmfx_mur_chunk_info(h, dist, C.byref(i64), C.byref(i64), C.byref(i64)),
        "mur_slice_info": lambda: lib.nmfx_mur_slice_info(h, dist, 1, C.byref(i64), C.byref(i64)),
    }
    unguarded = {     # (entry points that do not ask for V and factors themselves: only made where something else refuses them)
        "mur_phase_a_cols": lambda: lib.nmfx_mur_phase_a_cols(h, dist, 0, 128),
        "aoadmm_phase_w_fused": lambda: lib.nmfx_aoadmm_phase_w_fused(h, 1, 0.1, 5),
        "aoadmm_finish": lambda: lib.nmfx_aoadmm_finish(h, *T, j),
        "objective_partial": lambda: lib.nmfx_objective_partial(h),
        "objective_f64": lambda: lib.nmfx_objective_f64(h, C.byref(dbl)),
        "prox_apply": lambda: lib.nmfx_prox_apply(h, 0, 3, 1.0, 0.1, 0),
        "topk_svd": lambda: lib.nmfx_topk_svd(h, 4, 0, 0.0, 0, 0, p(u), p(s), p(vt), C.byref(i32), C.byref(dbl)),
    }
    closing = {"mur_finish_b": lambda: lib.nmfx_mur_finish_b(h, *T, j)}
    ao = {
        "aoadmm_run": lambda: lib.nmfx_aoadmm_run(h, dist, 1, 0.1, 1, 0.1, 5, *T, j, 1),
        "aoadmm_phase_h_products": lambda: lib.nmfx_aoadmm_phase_h_products(h, j),
        "aoadmm_phase_h_solve": lambda: lib.nmfx_aoadmm_phase_h_solve(h, 1, 0.1, 5, *T, j),
        "aoadmm_phase_w_products": lambda: lib.nmfx_aoadmm_phase_w_products(h, *T, j),
        "aoadmm_phase_w_close": lambda: lib.nmfx_aoadmm_phase_w_close(h, 5, j),
        "aoadmm_phase_w_repair": lambda: lib.nmfx_aoadmm_phase_w_repair(h, 1, 0.1, 5, j),
        "aoadmm_kl_phase_h_products": lambda: lib.nmfx_aoadmm_kl_phase_h_products(h, j, 0),
        "aoadmm_kl_phase_h_round": lambda: lib.nmfx_aoadmm_kl_phase_h_round(h, 1, 0.1, 0, *T, j),
        "aoadmm_kl_phase_h_close": lambda: lib.nmfx_aoadmm_kl_phase_h_close(h, 5, *T, j),
        "aoadmm_kl_phase_w_close": lambda: lib.nmfx_aoadmm_kl_phase_w_close(h, 5, j),
    }
    admm = {
        "admm_run": lambda: lib.nmfx_admm_run(h, dist, 1.0, 1, 0.1, 1, 0.1, *T, j, 1),
        "admm_phase_products": lambda: lib.nmfx_admm_phase_products(h, dist, 1.0, 1, 1, j),
    }
    anls = {
        "anls_run": lambda: lib.nmfx_anls_run(h, 0.0, 0.0, *T, j, 1),
        "anls_phase_objective": lambda: lib.nmfx_anls_phase_objective(h, j),
        "anls_phase_w": lambda: lib.nmfx_anls_phase_w(h, 0.0, *T, j),
        "anls_phase_h": lambda: lib.nmfx_anls_phase_h(h, 0.0, j),
    }
    return dict(mur=mur, no_index=no_index, info=info, unguarded=unguarded, closing=closing, ao=ao, admm=admm, anls=anls)


def refuse(s, lib, h, groups, dist, j, tag):
    """Make the calls of `groups`; every one of them must be refused (an accepted one is printed as such and ends the table:
    what it launched is not part of the digest)."""
    table = entry_points(lib, h, dist, j)
    for g in groups:
        for name, call in table[g].items():
            rc = call()
            if rc == 0 and g != "info":
                s.line(f"{tag} {name}", "ACCEPTED")
                return
            s.line(f"{tag} {name}", "ok" if rc == 0 else f"refused {rc}: {lib.nmfx_last_error(h).decode()}")
    st = s.eng.state()
    s.line(f"{tag} state", f"rule={st[0]} n_obj={st[2]}")


def refused(lib, h, rc):
    return f"refused {rc}: {lib.nmfx_last_error(h).decode()}" if rc else "ACCEPTED"


def refuse_all(s, lib, h, table, tag, skip=()):
    for name, call in table.items():
        if name not in skip:
            s.line(f"{tag} {name}", refused(lib, h, call()))


def refusal_sections(k, v, w0, h0, om):
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    lib = L.require_gpu()
    guarded = ["mur", "no_index", "info", "closing", "ao", "admm", "anls"]
    everything = guarded + ["unguarded"]
    if ONLY and ONLY not in "refusals":
        return
    with Engine(M, N, k) as e:
        s = Section(f"refusals/no-data k={k}", e)
        refuse(s, lib, e.h, guarded, L.EU, 0, "no V")
        refuse(s, lib, e.h, guarded, L.EU, -1, "no V, j<0")
        refuse(s, lib, e.h, guarded, 7, 0, "no V, loss 7")
        e.upload_v(v)
        refuse(s, lib, e.h, guarded, L.KL, 0, "no factors")
    with Engine(M, N, k) as e:
        s = Section(f"refusals/arguments k={k}", e)
        e.upload_v(v)
        e.set_factors(w0, h0)
        refuse(s, lib, e.h, ["mur", "closing", "ao", "admm", "anls"], L.EU, -1, "j<0")
        refuse(s, lib, e.h, ["mur", "admm"], 7, 0, "loss 7")
        refuse(s, lib, e.h, ["mur", "admm"], 7, -1, "loss 7, j<0")
        refuse(s, lib, e.h, ["mur", "no_index"], L.BETA, 0, "beta unset")
        if k <= 128:
            e.set_beta(0.5)
            refuse(s, lib, e.h, [g for g in ["mur", "info"]], L.BETA, -1, "beta, j<0")
            runs = ("mur_run", "mur_finish", "foldin_run", "foldin_finish", "mur_pair_run", "mur_pair_finish")
            for tag, dist in (("beta", L.BETA), ("is", L.IS)):          # (the phase-level entry points refuse both losses)
                table = entry_points(lib, e.h, dist, 0)
                refuse_all(s, lib, e.h, dict(table["mur"], profile_repeat=table["no_index"]["profile_repeat"]), tag, runs)
    if k <= 128:
        with Engine(M, N, k) as e:
            s = Section(f"refusals/weights k={k}", e)
            e.upload_v(v)
            e.upload_weights(om)
            e.set_factors(w0, h0)
            runs = ("mur_run", "mur_finish", "foldin_run", "foldin_finish")      # (they compute with weights and with ARD)
            flat = lambda table: {n: c for g in everything for n, c in table[g].items()}
            refuse_all(s, lib, e.h, flat(entry_points(lib, e.h, L.EU, 0)), "weights", runs)
            e.set_beta(0.5)
            e.set_ard(0.1, 5.0, 1.0)
            refuse_all(s, lib, e.h, flat(entry_points(lib, e.h, L.EU, -1)), "weights+ard,j<0")
            e.clear_weights()
            refuse_all(s, lib, e.h, flat(entry_points(lib, e.h, L.KL, 0)), "ard")
            for args in ((L.BETA, 0.1, 0.0), (L.BETA, 0.0, 0.1), (L.KL, 0.0, 0.0), (L.EU, 0.0, 0.0), (L.IS, 0.0, 0.0)):
                rc = lib.nmfx_mur_run(e.h, args[0], args[1], args[2], NEVER, 0.0, 0.0, 0, 1)
                s.line(f"ard mur_run {args}", refused(lib, e.h, rc))
            st = e.state()
            s.line("state", f"rule={st[0]} n_obj={st[2]}")
    with Engine(M, N, k) as e:
        s = Section(f"refusals/family k={k}", e)
        e.upload_v(v)
        e.set_factors(w0, h0)
        s.step("kl run 0..2", lambda: e.mur_run(L.KL, 0.01, 0.02, NEVER, 1e-5, 1e-5, 0, 3))
        refuse(s, lib, e.h, ["ao", "admm", "anls"], L.EU, 3, "behind mur")
        refuse(s, lib, e.h, ["ao", "admm", "anls"], L.EU, -1, "behind mur, j<0")
        s.step("kl run 3..4", lambda: e.mur_run(L.KL, 0.01, 0.02, NEVER, 1e-5, 1e-5, 3, 2))
        s.step("set_factors", lambda: e.set_factors(*e.get_factors()))
        s.step("anls run 0..1", lambda: e.anls_run(0.0, 0.0, NEVER, 1e-3, 1e-3, 0, 2))
        refuse(s, lib, e.h, ["mur", "no_index", "ao", "admm"], L.KL, 2, "behind anls")
        refuse(s, lib, e.h, ["mur", "ao", "admm"], L.KL, -1, "behind anls, j<0")
        s.step("anls run 2..3", lambda: e.anls_run(0.0, 0.0, NEVER, 1e-3, 1e-3, 2, 2))
        s.step("set_factors", lambda: e.set_factors(*e.get_factors()))
        s.step("aoadmm run 0..1", lambda: e.aoadmm_run(L.EU, 1, 0.1, 1, 0.1, 5, NEVER, 1e-3, 1e-3, 0, 2))
        refuse(s, lib, e.h, ["mur", "admm", "anls"], L.EU, 2, "behind aoadmm")
        s.step("aoadmm run 2..3", lambda: e.aoadmm_run(L.EU, 1, 0.1, 1, 0.1, 5, NEVER, 1e-3, 1e-3, 2, 2))
        s.step("set_factors", lambda: e.set_factors(*e.get_factors()))
        s.step("kl run 0..2", lambda: e.mur_run(L.KL, 0.01, 0.02, NEVER, 1e-5, 1e-5, 0, 3))


def between_sections(k, v, w0, h0):
    """Refused calls BETWEEN the calls of a run: what a refused call voids decides what the run rebuilds behind it (MUR-KL rebuilds
    its leftovers in another summation order than it continues from them; AO-ADMM rebuilds images: the same bits, more launches)."""
    from nmf_amd import _lib as L
    lib = L.require_gpu()
    flat = lambda h, dist, j: {n: c for g in entry_points(lib, h, dist, j).values() for n, c in g.items()}

    def kl_run(s, e):
        at = [0]

        def go_on():
            s.step(f"kl run {at[0]}..{at[0] + 1}", lambda: e.mur_run(L.KL, 0.01, 0.02, NEVER, 1e-5, 1e-5, at[0], 2))
            at[0] += 2
        go_on()
        for tag, dist, j, names in (("is, j<0", L.IS, -1, ("mur_run", "mur_finish", "foldin_run", "foldin_finish")),
                                    ("eu, j<0", L.EU, -1, ("mur_run", "mur_phase_a", "mur_phase_b", "mur_finish_a", "mur_finish_b", "mur_pair_run",
                                                           "anls_run", "anls_phase_objective", "aoadmm_run", "aoadmm_phase_h_products", "admm_run")),
                                    ("loss 7", 7, 0, ("admm_run", "admm_phase_products", "aoadmm_run")),
                                    ("eu, other family", L.EU, at[0], ("anls_phase_w", "aoadmm_kl_phase_w_close"))):
            for name in names:
                s.line(f"{tag} {name}", refused(lib, e.h, flat(e.h, dist, j)[name]()))
                go_on()
        s.step("kl finish", lambda: e.mur_finish(L.KL, NEVER, 1e-5, 1e-5, at[0]))
    dense("between/kl", k, v, w0, h0, kl_run)

    def ao_run(s, e):
        at = [0]

        def go_on():
            s.step(f"run {at[0]}", lambda: e.aoadmm_run(L.EU, 1, 0.1, 1, 0.1, 5, NEVER, 1e-3, 1e-3, at[0], 1))
            at[0] += 1
        go_on()
        for j in (None, -1):
            for name in ("mur_run", "mur_phase_a", "mur_finish_a", "anls_run", "admm_run", "aoadmm_phase_h_products", "mur_pair_run"):
                if not (j is None and name == "aoadmm_phase_h_products"):
                    s.line(f"j={j} {name}", refused(lib, e.h, flat(e.h, L.EU, at[0] if j is None else j)[name]()))
                    go_on()
        s.step("finish", lambda: e.aoadmm_finish(NEVER, 1e-3, 1e-3, at[0]))
    dense("between/aoadmm", k, v, w0, h0, ao_run)


# ---- the least-squares family behind ANLS: HALS, stacked HALS, sparse HALS ---------------------------------------------------------
def hals_sections(k, v, w0, h0):
    """HALS runs in both arithmetic modes with a change of the reported distance; stacks at this rank (one with ranks that leave
    components unowned) through set / terms / runs with differing lambdas / finish and the per-problem getters; sparse HALS;
    and what the hals entry points refuse."""
    import scipy.sparse as sp
    from nmf_amd import _lib as L
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    T = (NEVER, 1e-3, 1e-3)
    for f32 in (False, True):
        tag = "-f32" if f32 else ""
        for sweeps in (1, 3):
            def run(s, e):
                if f32:
                    s.step("set_precision f32", lambda: e.set_precision("f32"))
                s.step("run 0..1", lambda: e.hals_run(0.0, 0.01, sweeps, *T, 0, 2))
                s.step("set_distance kl", lambda: e.anls_set_distance(L.KL))
                s.step("run 2..3", lambda: e.hals_run(0.0, 0.01, sweeps, *T, 2, 2))
                s.step("set_distance eu", lambda: e.anls_set_distance(L.EU))
                s.step("run 4", lambda: e.hals_run(0.02, 0.0, 4 - sweeps, *T, 4, 1))
                s.step("run 5..6", lambda: e.hals_run(0.0, 0.01, sweeps, *T, 5, 2))
                s.step("finish 7", lambda: e.aoadmm_finish(*T, 7))
            dense(f"hals/s{sweeps}{tag}", k, v, w0, h0, run)

        for name, ks in (("hals_stack/part", (3, 5, 8)), ("hals_stack/full", (k // 4, k // 2, k - k // 4 - k // 2))):
            def stack(s, e):
                P = range(len(ks))
                lam = lambda a: [a * (p + 1) for p in P]

                def problems(label):
                    for p in P:
                        rule, stop_i, n_obj = e.hals_stack_state(p)
                        wp, hp = e.hals_stack_get_factors(p)
                        s.line(f"  {label} p={p}", f"W={sha(wp)} H={sha(hp)} obj={sha(e.hals_stack_objectives(p, 0, n_obj))} "
                                                    f"n={n_obj} rule={rule} stop_i={stop_i}")
                if f32:
                    s.step("set_precision f32", lambda: e.set_precision("f32"))
                s.step("set", lambda: e.hals_stack_set(ks))
                s.step("terms", lambda: s.line("  terms", sha(e.hals_stack_terms())))
                s.step("run 0..1", lambda: e.hals_stack_run(lam(0.0), lam(0.01), 1, *T, 0, 2))
                problems("run 0..1")
                s.step("run 2..3", lambda: e.hals_stack_run(lam(0.02), lam(0.0), 3, *T, 2, 2))
                problems("run 2..3")
                s.step("terms", lambda: s.line("  terms", sha(e.hals_stack_terms())))
                s.step("run 4..7 rule on", lambda: e.hals_stack_run(lam(0.02), lam(0.0), 1, 0, 1e-3, 1e-3 * 10.0 ** 6, 4, 4))
                problems("run 4..7")
                s.step("finish 8", lambda: e.hals_stack_finish(*T, 8))
                problems("finish 8")
            if k <= 128:
                dense(f"{name}{tag}", k, v, w0, h0, stack)

    if k <= 128 and not (ONLY and ONLY not in "hals_sparse"):
        x = sp.csr_matrix(np.where(np.random.default_rng(9000 + k).random(v.shape) < 0.3, v, 0).astype(np.float64))
        with Engine.for_sparse(sparse.normalise(x, k), k) as e:
            s = Section(f"hals_sparse k={k}", e)
            e.set_factors(w0, h0)
            s.step("run 0..1", lambda: e.hals_sparse_run(0.0, 0.01, 1, *T, 0, 2))
            s.step("run 2..3", lambda: e.hals_sparse_run(0.02, 0.0, 3, *T, 2, 2))
            s.step("finish 4", lambda: e.hals_sparse_finish(*T, 4))
            s.step("hals_run on it", lambda: e.hals_run(0.0, 0.0, 1, *T, 4, 1))
            hals_refusals(s, L.require_gpu(), e.h, "sparse", ("hals_sparse_run", "hals_sparse_finish"), accepted_ok=False)

    if ONLY and ONLY not in "refusals":
        return
    lib = L.require_gpu()
    stack_calls = ("hals_stack_terms", "hals_stack_run", "hals_stack_finish")
    dense_calls = ("hals_run",) + stack_calls + ("hals_sparse_run", "hals_sparse_finish")
    with Engine(M, N, k) as e:
        s = Section(f"refusals/hals k={k}", e)
        hals_refusals(s, lib, e.h, "no V", dense_calls)
        e.upload_v(v)
        e.set_factors(w0, h0)
        hals_refusals(s, lib, e.h, "no stack", dense_calls, accepted_ok=False)
        if k > 128:
            return
        s.step("set", lambda: e.hals_stack_set((3, 5, 8)))
        hals_refusals(s, lib, e.h, "stack set", stack_calls, accepted_ok=False)
        s.step("set_factors", lambda: e.set_factors(w0, h0))
        s.step("kl run 0..1", lambda: e.mur_run(L.KL, 0.01, 0.02, NEVER, 1e-5, 1e-5, 0, 2))
        s.step("set behind mur", lambda: e.hals_stack_set((3, 5, 8)))
        hals_refusals(s, lib, e.h, "behind mur", dense_calls)
        s.step("set_factors", lambda: e.set_factors(w0, h0))
        s.step("stack run 0", lambda: e.hals_stack_run([0.0] * 3, [0.0] * 3, 1, *T, 0, 1))
        hals_refusals(s, lib, e.h, "behind the stack", ("hals_run",))
        refuse(s, lib, e.h, ["mur", "ao", "admm", "anls"], L.EU, 1, "behind the stack")
        s.step("set_factors", lambda: e.set_factors(w0, h0))
        s.step("hals run 0", lambda: e.hals_run(0.0, 0.0, 1, *T, 0, 1))
        hals_refusals(s, lib, e.h, "behind hals", stack_calls)
        refuse(s, lib, e.h, ["mur", "ao", "admm", "anls"], L.EU, 1, "behind hals")
        hals_refusals(s, lib, e.h, "hals", ("hals_run",), accepted_ok=False)


def hals_refusals(s, lib, h, tag, names, accepted_ok=True):
    """The hals entry points `names` as raw ABI calls: as they should be called (accepted_ok=False: that call is left out, the
    handle would take it), then with j < 0, sweeps = 0 (terms: out = NULL), sweeps = 17, a negative lambda, no lambdas, and with two
    of these at once.  An entry point that does not take the argument in question accepts the call; the line says so."""
    T = (NEVER, 0.0, 0.0)
    out = (C.c_double * 256)()
    lam = lambda a: (C.c_double * 128)(*([a] * 128))
    table = {
        "hals_run": lambda j, sw, a: lib.nmfx_hals_run(h, a, 0.0, sw, *T, j, 1),
        "hals_sparse_run": lambda j, sw, a: lib.nmfx_hals_sparse_run(h, 0.0, a, sw, *T, j, 1),
        "hals_sparse_finish": lambda j, sw, a: lib.nmfx_hals_sparse_finish(h, *T, j),
        "hals_stack_terms": lambda j, sw, a: lib.nmfx_hals_stack_terms(h, out if sw else None),
        "hals_stack_run": lambda j, sw, a: lib.nmfx_hals_stack_run(h, lam(0.0), lam(a) if a > -1 else None, sw, *T, j, 1),
        "hals_stack_finish": lambda j, sw, a: lib.nmfx_hals_stack_finish(h, *T, j),
    }
    cases = (("", 1, 1, 0.0), ("j<0", -1, 1, 0.0), ("sweeps=0", 1, 0, 0.0), ("sweeps=17", 1, 17, 0.0), ("lambda<0", 1, 1, -0.5),
             ("lambda NULL", 1, 1, -2.0), ("sweeps=0, j<0", -1, 0, 0.0), ("sweeps=17, lambda<0", 1, 17, -0.5), ("j<0, lambda<0", -1, 1, -0.5))
    for name in names:
        for what, j, sw, a in cases:
            if what or accepted_ok:
                s.line(f"{tag} {name} {what}".rstrip(), refused(lib, h, table[name](j, sw, a)))
    st = s.eng.state()
    s.line(f"{tag} state", f"rule={st[0]} n_obj={st[2]}")


def hals_variant_sections(k, v, w0, h0, mask):
    """The HALS variants behind the stack: hals_wide and hals_sparse_wide at k = 160, masked HALS at k = 40, the fold-in on a sparse
    handle (k = 40, 100), on a masked handle (k = 40) and on a dense one (k = 40, 100).  Every fold-in runs with tol = 0 under a cap of
    3 sweeps and of 40 (the kept residual is formed anew before sweep 17 and before sweep 33), and its sweep counts are hashed.  The
    sparse data and the mask hold one full row and one full column: longer than a piece, for the fix-up and long kernels."""
    import scipy.sparse as sp
    from nmf_amd import masked
    from nmf_amd import sparse
    from nmf_amd.engine import Engine
    T = (NEVER, 1e-3, 1e-3)
    wanted = lambda name: not (ONLY and ONLY not in name)

    def runs(s, run, finish):
        s.step("run 0..1", lambda: run(0.0, 0.01, 1, *T, 0, 2))
        s.step("run 2..3", lambda: run(0.02, 0.0, 3, *T, 2, 2))
        s.step("finish 4", lambda: finish(*T, 4))

    def foldin(s, e, run, sweeps_of):
        for cap in (3, 40):
            s.step("set_factors", lambda: e.set_factors(w0, h0))
            s.step(f"foldin cap {cap}", lambda: run(0.01, 0.0, cap))
            s.line(f"  sweeps cap {cap}", f"{sha(sweeps_of())} max={int(sweeps_of().max())}")

    xd = np.where(np.random.default_rng(9100 + k).random(v.shape) < 0.3, v, 0).astype(np.float64)
    xd[:, 5], xd[7] = v[:, 5], v[7]
    full = mask.copy()
    full[:, 5], full[7] = True, True
    if k > 128:
        dense("hals_wide", k, v, w0, h0, lambda s, e: runs(s, e.hals_wide_run, e.aoadmm_finish))
        if wanted("hals_sparse_wide"):
            with Engine.for_sparse(sparse.normalise(sp.csr_matrix(xd), k), k) as e:
                s = Section(f"hals_sparse_wide k={k}", e)
                e.set_factors(w0, h0)
                runs(s, e.hals_sparse_wide_run, e.hals_sparse_wide_finish)
        return
    if wanted("hals_foldin/sparse"):
        with Engine.for_sparse(sparse.normalise(sp.csr_matrix(xd), k), k) as e:
            foldin(Section(f"hals_foldin/sparse k={k}", e), e, e.hals_foldin_run, e.hals_foldin_sweeps)
    dense("hals_foldin_dense", k, v, w0, h0, lambda s, e: foldin(s, e, e.hals_foldin_dense_run, e.hals_foldin_dense_sweeps))
    if k > 64:
        return
    if wanted("hals_masked"):
        with Engine.for_sparse(masked.observed(v.astype(np.float64), full, k), k, masked=True) as e:
            s = Section(f"hals_masked k={k}", e)
            e.set_factors(w0, h0)
            runs(s, e.hals_masked_run, e.hals_masked_finish)
    if wanted("hals_foldin/masked"):
        with Engine.for_sparse(masked.observed(v.astype(np.float64), full, k), k, masked=True) as e:
            foldin(Section(f"hals_foldin/masked k={k}", e), e, e.hals_foldin_run, e.hals_foldin_sweeps)


def main():
    global LINES
    if "--fold" in sys.argv:
        return fold(open(sys.argv[sys.argv.index("--fold") + 1]).read().splitlines())
    if "--sections" in sys.argv:
        LINES = []
    for k in RANKS:
        v, w0, h0, om, mask = make_inputs(k, seed=5000 + k)
        mur_sections(k, v, w0, h0, om, mask)
        admm_family_sections(k, v, w0, h0)
        refusal_sections(k, v, w0, h0, om)
        between_sections(k, v, w0, h0)
    # (behind the sections above, whose lines they leave where they were) the ADMM family by its steps: also at a rank that pads to 16,
    # and the Euclidean AO-ADMM once beyond 512 padded components, where its sub-problems take the rhs / solve / prox launches
    for k in (12,) + RANKS:
        v, w0, h0, om, mask = make_inputs(k, seed=5000 + k)
        if k not in RANKS:
            admm_family_sections(k, v, w0, h0)
        admm_step_sections(k, v, w0, h0)
    # (a start with W H at the data's scale: from the unscaled one the first sub-problem wipes H out and the next Gram system is singular)
    v, w0, h0, om, mask = make_inputs(520, seed=5520, shape=(640, 576), scale=0.06)
    admm_family_sections(520, v, w0, h0, losses=("eu",))
    admm_family_sections(520, v, w0, h0, f32=True, losses=("eu",))
    # (behind everything above) HALS on the products of ANLS: runs, stacks, sparse input, refusals
    for k in RANKS:
        v, w0, h0, om, mask = make_inputs(k, seed=5000 + k)
        hals_sections(k, v, w0, h0)
    # (behind them) the HALS variants that came after the stack: wide, sparse wide, masked, the three fold-ins
    for k in RANKS:
        v, w0, h0, om, mask = make_inputs(k, seed=5000 + k)
        hals_variant_sections(k, v, w0, h0, mask)
    if LINES is not None:
        fold(LINES)


if __name__ == "__main__":
    main()
