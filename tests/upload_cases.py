"""Shared by tests/test_gpu_upload.py: the base problem, the ways a matrix can be delivered to a handle (nmfx_upload_v,
nmfx_upload_v_device, nmfx_upload_weights) and one runner per solver that returns everything the solver leaves behind.

Two deliveries of the same f32 values must leave the same V on the device, and the kernels are deterministic, so two runs
from the same start agree bit for bit (`same`); one delivery per configuration is also compared with the float64 step
(mur_step.check_steps at mur_step.BARS), which is what says that the V the device holds is the caller's."""
import functools
import os

import numpy as np

from mur_step import NEVER, make_inputs

M, N = 257, 200             # ragged in both directions: straddles the 128-row tile and the 64-column group
LD = 237                    # row stride of the wide arrays
BLOCKS = [(0, 1), (1, 128), (128, 129), (129, 257)]
NEW = (100, 140)            # the rows replaced on a used handle: a partial block, aligned to neither 64 nor 128
FILL = 7.5                  # what the wide arrays hold outside the block (a reader that strays sees it)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(k, seed=0, positive=False):
    """(V f32, W0, H0) of the base problem; positive: V without its exact zeros (the Itakura-Saito loss has no value there)."""
    v, w0, h0 = make_inputs(M, N, k, seed=8100 + 7 * seed + k, edges=True, zeros=True)
    if positive:
        v = np.where(v > 0, v, np.float32(0.5)).astype(np.float32)
    for a in (v, w0, h0):
        a.setflags(write=False)
    return v, w0, h0


def merged(va, vb):
    out = va.copy()
    out[NEW[0]:NEW[1]] = vb[NEW[0]:NEW[1]]
    return out


@functools.lru_cache(maxsize=None)
def weights(seed=0):
    """Uniform in [0, 2) f32 with exact zeros (2 % of the cells, a whole row and a whole column)."""
    rng = np.random.default_rng(8800 + seed)
    om = rng.uniform(0.0, 2.0, (M, N)).astype(np.float32)
    om[rng.random((M, N)) < 0.02] = 0
    om[5, :] = 0
    om[:, 7] = 0
    om.setflags(write=False)
    return om


def hankel(dtype=np.float32, seed=0):
    """A sliding-window (Hankel) V: row i is x[i : i + N] of one signal -- rows one element apart, strides[0] == itemsize."""
    from numpy.lib.stride_tricks import sliding_window_view
    x = np.random.default_rng(8900 + seed).uniform(0.05, 1.0, M + N - 1).astype(np.float32).astype(dtype)
    return sliding_window_view(x, N)


# ---- host deliveries: put(block, row0) is eng.upload_v or eng.upload_weights ----------------------------------------------
def wide(a, ld=LD):
    """`a` as the [:, :n] view of an array with `ld` columns."""
    big = np.full((a.shape[0], ld), FILL, dtype=a.dtype)
    big[:, :a.shape[1]] = a
    return big[:, :a.shape[1]]


def every_second_row(a, ld=LD):
    big = np.full((2 * a.shape[0], ld), FILL, dtype=a.dtype)
    big[::2, :a.shape[1]] = a
    return big[::2, :a.shape[1]]


def _blocks(put, a):
    for r0, r1 in BLOCKS:
        put(a[r0:r1], r0)


def _blocks_reversed(put, a):
    for r0, r1 in reversed(BLOCKS):
        put(a[r0:r1], r0)


def _overlapping(put, a):
    """The later call wins: garbage first, then the true rows over it."""
    junk = np.random.default_rng(1).uniform(2.0, 3.0, (100, a.shape[1])).astype(a.dtype)
    put(junk, 100)
    put(a[64:], 64)
    put(a[:64], 0)


HOST_FORMS = {
    "blocks": _blocks,
    "blocks_reversed": _blocks_reversed,
    "overlapping": _overlapping,
    "ld237": lambda put, a: put(wide(a), 0),
    "every_second_row": lambda put, a: put(every_second_row(a), 0),
}
HOST_DELIVERIES = [(form, dt) for dt in ("f32", "f64") for form in HOST_FORMS]
NP_DTYPE = {"f32": np.float32, "f64": np.float64}


def deliver_host(put, a, form, dt):
    """`a` (f32 values) through one of HOST_FORMS as float32 or as float64 holding the same values."""
    b = np.asarray(a, dtype=NP_DTYPE[dt])
    HOST_FORMS[form](put, b)


# ---- device deliveries ------------------------------------------------------------------------------------------------------
DEVICE_DELIVERIES = [(dt, parts, ld) for dt in ("f32", "f64") for parts in ("whole", "blocks") for ld in (N, LD)]


def deliver_device(eng, a, dt, parts, ld):
    """nmfx_upload_v_device from a torch tensor on the GPU, which is freed before the caller runs anything (include/nmfx.h:
    the source may be freed once the call returns)."""
    import torch
    n = a.shape[1]
    host = np.full((a.shape[0], ld), FILL, dtype=NP_DTYPE[dt])
    host[:, :n] = a
    t = torch.from_numpy(host).cuda()
    item = host.itemsize
    for r0, r1 in ([(0, a.shape[0])] if parts == "whole" else BLOCKS):
        torch.cuda.synchronize()
        eng.upload_v_device(t.data_ptr() + r0 * ld * item, r1 - r0, row0=r0, dtype=NP_DTYPE[dt], ld=ld)
    del t
    torch.cuda.empty_cache()


# ---- runners: everything a solver leaves behind, as a flat tuple of arrays ---------------------------------------------------
def code(kind):
    from nmf_amd import _lib as L
    return {"eu": L.EU, "kl": L.KL, "is": L.IS, "beta": L.BETA}[kind]


def drive(eng, kind, w0, h0, lw=0.0, lh=0.0, steps=(1, 2)):
    """mur_step._drive for any loss of nmfx_mur_run: {s: (W_s, H_s, recorded objectives 0 .. s)}."""
    out = {}
    for s in steps:
        eng.set_factors(w0, h0)
        eng.mur_run(code(kind), lw, lh, NEVER, 0, 0, 0, s)
        eng.mur_finish(code(kind), NEVER, 0, 0, s)
        w, h = eng.get_factors()
        out[s] = (w, h, eng.objectives(0, s + 1))
    return out


def flat(runs):
    return tuple(a for s in sorted(runs) for a in runs[s])


def arith_of(eng, k, precision):
    """The bar a dense MUR run on this handle is held to (mur_step.run_dense)."""
    requested = precision or ("f32" if os.environ.get("NMFX_PRECISION") in ("f32", "fp32") else "bf16")
    return "bf16" if eng.precision() == "bf16" or (k > 128 and requested == "bf16") else "f32"


def run_mur(deliver, kind, k, precision, w0, h0, lw=0.0, lh=0.0, m=M, n=N, steps=(1, 2)):
    """A fresh handle, `deliver(eng)`, then the two runs of mur_step._drive: (runs, arithmetic)."""
    from nmf_amd.engine import Engine
    with Engine(m, n, k) as eng:
        if precision is not None:
            eng.set_precision(precision)
        arith = arith_of(eng, k, precision)
        deliver(eng)
        return drive(eng, kind, w0, h0, lw, lh, steps), arith


def solver_pair(eng, w0, h0):
    """Two Euclidean problems (k = 40 and 24) in a k = 128 handle; (w0, h0) has 64 components to cut them from."""
    ks = (40, 24)
    ws, hs = np.zeros((M, 128)), np.zeros((128, N))
    for p, kp in enumerate(ks):
        ws[:, 64 * p:64 * p + kp] = w0[:, 40 * p:40 * p + kp]
        hs[64 * p:64 * p + kp] = h0[40 * p:40 * p + kp]
    eng.set_factors(ws, hs)
    eng.mur_pair_run((0.0, 0.01), (0.0, 0.02), NEVER, 0, 0, 0, 2)
    eng.mur_pair_finish(NEVER, 0, 0, 2)
    out = []
    for p, kp in enumerate(ks):
        out += list(eng.pair_get_factors(p, kp)) + [eng.pair_objectives(p, 0, 3)]
    return tuple(out)


def solver_hals(eng, w0, h0):
    eng.set_factors(w0, h0)
    eng.anls_set_distance(code("eu"))
    eng.hals_run(0.0, 0.0, 1, NEVER, 0, 0, 0, 2)
    eng.aoadmm_finish(NEVER, 0, 0, 2)
    return (*eng.get_factors(), eng.objectives(0, 3))


def solver_hals_stack(eng, w0, h0):
    ks = [24, 16]
    eng.set_factors(w0, h0)
    eng.hals_stack_set(ks)
    eng.hals_stack_run([0.0, 0.01], [0.0, 0.02], 1, NEVER, 0, 0, 0, 2)
    eng.hals_stack_finish(NEVER, 0, 0, 2)
    return (*eng.get_factors(), *(eng.hals_stack_objectives(p, 0, 3) for p in range(2)))


def solver_anls(eng, w0, h0):
    eng.set_factors(w0, h0)
    eng.anls_set_distance(code("eu"))
    eng.anls_run(0.0, 0.0, NEVER, 0, 0, 0, 2)
    eng.aoadmm_finish(NEVER, 0, 0, 2)
    return (*eng.get_factors(), eng.objectives(0, 3))


def solver_aoadmm(eng, w0, h0):
    from nmf_amd import _lib as L
    eng.set_factors(w0, h0)
    eng.aoadmm_run(L.EU, L.PROX["nn"], 0.0, L.PROX["nn"], 0.0, 5, NEVER, 0, 0, 0, 2)
    eng.aoadmm_finish(NEVER, 0, 0, 2)
    return (*eng.get_factors(), eng.objectives(0, 3), eng.get_matrix("dual_w"), eng.get_matrix("dual_h"))


def solver_admm(kind):
    def run(eng, w0, h0):
        from nmf_amd import _lib as L
        eng.set_factors(w0, h0)
        eng.admm_run(code(kind), 1.0, L.PROX["nn"], 0.0, L.PROX["nn"], 0.0, NEVER, 0, 0, 0, 2)
        eng.aoadmm_finish(NEVER, 0, 0, 2)
        return (*eng.get_factors(), eng.objectives(0, 3), *(eng.get_matrix(name) for name in ("w_aux", "h_aux", "dual_w", "dual_h")))
    return run


def solver_svd(eng, w0, h0):
    u, s, vt, _, _ = eng.topk_svd(4)
    return u, s, vt


def solver_objective_f64(eng, w0, h0):
    eng.set_factors(w0, h0)
    return (np.array([eng.objective_f64()]),)


def same(got, want, what):
    """Bit for bit: every array of `got` equals its partner in `want`."""
    assert len(got) == len(want), what
    bad = [i for i, (a, b) in enumerate(zip(got, want)) if not np.array_equal(a, b)]
    if bad:
        i = bad[0]
        a, b = np.asarray(got[i], dtype=np.float64), np.asarray(want[i], dtype=np.float64)
        diff = np.argwhere(a != b) if a.shape == b.shape else []
        where = tuple(int(x) for x in diff[0]) if len(diff) else "?"
        raise AssertionError(f"{what}: results {bad} of {len(got)} differ; result {i}: {len(diff)} of {a.size} entries, the first at {where}"
                             + (f": {a[where]!r} != {b[where]!r}" if len(diff) else ""))
