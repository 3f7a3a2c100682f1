"""The device top-k SVD (nmf_amd/csrc/kernels_svd.hip, LAB_NOTES 4d') stated in numpy float64, the comparator that holds a set
of returned triplets to LAPACK's, and the case table shared by tests/test_svd_bars.py (CPU) and tests/test_gpu_svd.py (GPU).

emulate_topk follows topk_svd step by step: the padded f64 blocks, the Gram-based Rayleigh-Ritz with its floors, the two-pass
orthonormalisation, locking, the deflated Chebyshev filter with its degree cap, the completion of null triplets and the residual
taken again over all k triplets behind it.  numpy.linalg.eigh stands for the host's threshold Jacobi solver and numpy's generator
for mt19937_64: the iterates differ from the device's in rounding and in the start block.  eigh resolves a Gram matrix to
eps theta_1 absolutely, threshold Jacobi to eps per column, so the emulation is the less accurate of the two at k >= 85 and, at
k = 33 and 44, loses the weakest wanted column under the first filter pass and needs hundreds of sweeps where the device needs 4
and 8 (both recorded in DESIGN.md 2): its deviations and sweep counts bound the device's from above.  `fault=` plants the faults
of tests/test_svd_bars.py."""
import json
import os
from collections import namedtuple

import numpy as np

SIZES = (32, 48, 64, 96, 128, 160, 192)          # block widths L = 16 NT of the seven instantiations
DOC = dict(values=1e-12, orth=1e-10, vectors=1e-7, recon=1e-9, resid=1e-11)       # the documented bars (LAB_NOTES 4d')
NULL_ABS = 1e-12            # |s_j - sr_j| <= NULL_ABS sr_0 behind the numerical rank
RANK_REL = 1e-10            # numerical rank: #{sr_j > RANK_REL sr_0}
GAP = 1e-3                  # a triplet is compared vector by vector where both neighbours are further than GAP sr_0
EQUAL = 1e-6                # values within EQUAL sr_0 of their neighbour form a cluster (f32 rounding of equal values: 1e-7)


def block_width(k, block=0):
    """L as nmfx_topk_svd picks it."""
    if block <= 0:
        block = max(k + 16, k + k // 2)
    block = max(block, k)
    return next((c for c in SIZES if c >= block), 192)


def _pad(x):
    return -(-x // 128) * 128


def _eigh_desc(t):
    th, s = np.linalg.eigh(t)
    o = np.argsort(-th, kind="stable")
    return th[o], s[:, o]


def _gram(x, fault=None):
    t = x.T @ x
    if fault == "gram_tile4":                       # tile column 4 never written: the second pass of the waves (NW >= 2)
        t[:, 64:80] = 0.0
    return 0.5 * (t + t.T)                          # gram_to_host: exact symmetry for the host solver


def _orth(x):
    """orthonormalize: Ritz order of x^T x, then (I + E)^-1/2 of what the first pass leaves."""
    th, s = _eigh_desc(_gram(x))
    fl = max(th[0], 0.0) * 1e-28
    sc = np.where((th > fl) & (th > 0), 1.0 / np.sqrt(np.where(th > 0, th, 1.0)), 0.0)
    tmp = x @ (s * sc)
    th2, s2 = _eigh_desc(_gram(tmp))
    sc2 = np.where(th2 > 0.25, 1.0 / np.sqrt(np.where(th2 > 0, th2, 1.0)), 0.0)
    return tmp @ ((s2 * sc2) @ s2.T)


def _complete(x, dead, rng, rows):
    """complete_columns: each dead column becomes a random unit vector orthogonal to the other columns (two Gram-Schmidt passes)."""
    for j in dead:
        for _ in range(4):
            c = np.zeros(x.shape[0])
            c[:rows] = rng.standard_normal(rows)
            x[:, j] = 0.0
            for _ in range(2):
                c -= x @ (x.T @ c)
            nrm = np.linalg.norm(c)
            if nrm > 1e-8:
                break
        x[:, j] = c / nrm
    return x


def emulate_topk(v, k, block=0, tol=0, max_sweeps=0, seed=0, fault=None):
    """(u m x k, s k, vt k x n, sweeps, resid, L) of the algorithm of kernels_svd.hip on the f32-rounded v, in float64."""
    v = np.asarray(v, np.float32).astype(np.float64)
    m, n = v.shape
    L = block_width(k, block)
    tol = 1e-11 if tol <= 0 else tol
    max_sweeps = 4000 if max_sweeps <= 0 else max_sweeps
    mp, npad = _pad(m), _pad(n)
    vp = np.zeros((mp, npad))
    vp[:m, :n] = v
    rng = np.random.default_rng(seed)
    q = np.zeros((npad, L))
    q[:n] = rng.standard_normal((n, L))
    if fault == "pad_start":                        # the padded rows of the start block are not zero
        q[n:] = rng.standard_normal((npad - n, L))
    q = _orth(q)
    sweep, u = 0, None
    while True:
        sweep += 1
        if fault == "drop_chunk":                   # the last 32-column chunk of the contraction is missing from V Q
            y = vp[:, :npad - 32] @ q[:npad - 32]
        else:
            y = vp @ q
        theta, s = _eigh_desc(_gram(y, fault))
        fl = max(theta[0], 0.0) * 1e-28
        sigma = np.where(theta > 0, np.sqrt(np.abs(theta)), 0.0)
        live = (theta > fl) & (theta > 0)
        sc = np.where(live, 1.0 / np.where(sigma > 0, sigma, 1.0), 0.0)
        u_prev, u = u, y @ (s * sc)
        if fault == "stale_block" and u_prev is not None:      # one 64-row block of U left from the sweep before
            u[64:128] = u_prev[64:128]
        qr = q @ s
        z = vp.T @ u
        res = np.linalg.norm(z - qr * sigma, axis=0)
        worst = max([res[j] / sigma[0] for j in range(k) if sigma[j] > 0] + [0.0])
        # null triplets among the first k: completed to an orthonormal set, the residual taken again over all k
        dead = [j for j in range(k) if not live[j]]
        completed = False
        if dead and (worst <= tol or sweep >= max_sweeps):
            crng = np.random.default_rng([seed, sweep])
            sigma[dead] = 0.0
            uk = _complete(u[:, :k].copy(), dead, crng, m)
            vk = _complete(qr[:, :k].copy(), dead, crng, n)
            u[:, :k], qr[:, :k] = uk, vk
            z = vp.T @ u
            res = np.linalg.norm(z - qr * sigma, axis=0)
            worst = max(worst, max(res[j] / sigma[0] if sigma[0] > 0 else 0.0 for j in range(k)))
            completed = True
        if worst <= tol or sweep >= max_sweeps:
            break
        nl = 0
        while nl < k and sigma[nl] > 0 and res[nl] / sigma[0] <= tol:
            nl += 1
        cb, a0 = theta[L - 1], theta[min(nl, L - 1)]
        ranged = cb > 1e-12 * a0 and a0 > 1.000001 * cb
        degree = 10
        if ranged:
            e0 = 0.5 * cb

            def grow(th):
                xx = max((th - e0) / e0, 1.0)
                return xx + np.sqrt(xx * xx - 1.0)
            ratio = grow(a0) / max(grow(theta[k - 1]), 1.0)
            if ratio > 1.0:
                degree = int(min(10.0, np.floor(np.log(1e9) / np.log(ratio))))
        if completed or sweep < 3 or degree < 2 or not ranged:
            q = _orth(z)                            # (behind a completion z = V^T U carries the fresh directions)
            continue
        e = c = 0.5 * cb
        sg = e / (a0 - c)
        tau = 2.0 / sg

        def deflate(x, ax):
            if nl == 0 or fault == "no_deflation":
                return ax
            d = np.zeros((L, L))
            d[:nl] = theta[:nl, None] * (qr.T @ x)[:nl]
            return ax - qr @ d
        x0 = qr
        x1 = sg / e * deflate(x0, z * sigma) - c * sg / e * x0
        xp = x0
        for _ in range(2, degree + 1):
            sn = 1.0 / (tau - sg)
            ax = deflate(x1, vp.T @ (vp @ x1))
            xp, x1 = x1, 2.0 * sn / e * ax - 2.0 * sn * c / e * x1 - sg * sn * xp
            sg = sn
        nb = x1.copy()
        nb[:, :nl] = qr[:, :nl]
        q = _orth(nb)
    return u[:m, :k].copy(), sigma[:k].copy(), qr[:n, :k].T.copy(), sweep, float(worst), L


# ---- comparator -----------------------------------------------------------------------------------------------------------
_LAPACK = {}


def lapack(v):
    """numpy.linalg.svd of the f32-rounded v in float64 (computed once per input)."""
    v64 = np.asarray(v, np.float32).astype(np.float64)
    key = (v64.shape, hash(v64.tobytes()))
    if key not in _LAPACK:
        _LAPACK[key] = np.linalg.svd(v64, full_matrices=False)
    return (v64,) + _LAPACK[key]


def recompute_resid(v, u, s, vt):
    """max_j ||V^T u_j - s_j v_j|| / s_0 over all returned triplets, float64 on the host."""
    v64 = np.asarray(v, np.float32).astype(np.float64)
    d = v64.T @ u - vt.T * s
    return float(np.max(np.linalg.norm(d, axis=0)) / s[0]) if s[0] > 0 else float("inf")


def _where(x, ref, j, what):
    i = int(np.argmax(np.abs(x - ref)))
    return f"{what}: triplet {j}, row {i} (64-row block {i // 64}): {x[i]:.6e} against {ref[i]:.6e}"


def check_triplets(v, u, s, vt, resid, k, bars):
    """(fails, dev): `fails` lists every bar of `bars` (keys of DOC; resid None: not asserted) that the triplets miss against
    LAPACK's, `dev` the measured deviation per quantity.  With sr LAPACK's values and r the numerical rank: s_j relative for
    j < r, absolute (NULL_ABS sr_0) behind; u^T u and vt vt^T against I over all k; the rank-min(k, r) reconstruction;
    separated triplets vector by vector after sign alignment, clusters of equal values that end inside k by their projector;
    the reported residual against the one recomputed here over all k."""
    v64, ur, sr, vtr = lapack(v)
    fails, dev = [], dict(values=0.0, null=0.0, orth=0.0, vectors=0.0, recon=0.0, resid=float(resid))
    if not (np.isfinite(u).all() and np.isfinite(s).all() and np.isfinite(vt).all() and np.isfinite(resid)):
        return ["[finite]: a returned value is not finite"], dict(dev, values=np.inf, orth=np.inf, vectors=np.inf, recon=np.inf)
    r = int(np.sum(sr > RANK_REL * sr[0]))
    kr = min(k, r)
    # values
    for j in range(k):
        if j < r:
            d = abs(s[j] - sr[j]) / sr[j]
            dev["values"] = max(dev["values"], d)
            if d > bars["values"]:
                fails.append(f"[values]: triplet {j}: {s[j]:.15e} against {sr[j]:.15e} (relative {d:.2e}, bar {bars['values']:.1e})")
        else:
            d = abs(s[j] - sr[j]) / sr[0]
            dev["null"] = max(dev["null"], d)
            if d > NULL_ABS:
                fails.append(f"[values]: null triplet {j}: {s[j]:.3e} against {sr[j]:.3e} ({d:.2e} of s_0, bar {NULL_ABS:.0e})")
    # orthonormality over all k triplets
    for name, g in (("u^T u", u.T @ u), ("vt vt^T", vt @ vt.T)):
        e = np.abs(g - np.eye(k))
        d = float(e.max())
        dev["orth"] = max(dev["orth"], d)
        if d > bars["orth"]:
            a, b = np.unravel_index(int(np.argmax(e)), e.shape)
            fails.append(f"[orthonormality]: {name}[{a}, {b}] is off by {d:.2e} (bar {bars['orth']:.1e})")
    # reconstruction of numerical rank
    rec, rec_ref = (u[:, :kr] * s[:kr]) @ vt[:kr], (ur[:, :kr] * sr[:kr]) @ vtr[:kr]
    dev["recon"] = float(np.linalg.norm(rec - rec_ref) / np.linalg.norm(rec_ref))
    if dev["recon"] > bars["recon"]:
        e = np.abs(rec - rec_ref)
        a, b = np.unravel_index(int(np.argmax(e)), e.shape)
        fails.append(f"[reconstruction]: rank {kr}: {dev['recon']:.2e} (bar {bars['recon']:.1e}); worst element ({a}, {b}), 64-row block {a // 64}")
    # vectors
    gap = GAP * sr[0]
    ext = np.concatenate(([np.inf], sr, [-np.inf]))                # ext[j + 1] = sr[j]
    j = 0
    while j < kr:
        e = j + 1
        while e < len(sr) and sr[e - 1] - sr[e] <= EQUAL * sr[0]:
            e += 1                                                  # [j, e): values equal to their neighbours
        lo, hi = ext[j] - sr[j], sr[e - 1] - ext[e + 1]
        if e <= kr and lo > gap and hi > gap:
            if e == j + 1:
                sgn = 1.0 if float(u[:, j] @ ur[:, j]) >= 0 else -1.0
                for what, x, ref in (("u", sgn * u[:, j], ur[:, j]), ("vt", sgn * vt[j], vtr[j])):
                    d = float(np.max(np.abs(x - ref)))
                    dev["vectors"] = max(dev["vectors"], d)
                    if d > bars["vectors"]:
                        fails.append(f"[vectors, {what}]: {_where(x, ref, j, what)} (off by {d:.2e}, bar {bars['vectors']:.1e})")
            else:
                for what, x, ref in (("u", u[:, j:e], ur[:, j:e]), ("vt", vt[j:e].T, vtr[j:e].T)):
                    pe = np.abs(x @ x.T - ref @ ref.T)
                    d = float(pe.max())
                    dev["vectors"] = max(dev["vectors"], d)
                    if d > bars["vectors"]:
                        a = int(np.unravel_index(int(np.argmax(pe)), pe.shape)[0])
                        fails.append(f"[vectors, {what}]: projector of the cluster of triplets {j}..{e - 1}: row {a} (64-row block {a // 64}) "
                                     f"off by {d:.2e} (bar {bars['vectors']:.1e})")
        j = e
    # the reported residual
    dev["resid_host"] = recompute_resid(v, u, s, vt)
    if not resid >= 0.5 * dev["resid_host"] - 1e-13:
        jw = int(np.argmax(np.linalg.norm(v64.T @ u - vt.T * s, axis=0)))
        fails.append(f"[residual]: reported {resid:.2e}, recomputed over all {k} triplets {dev['resid_host']:.2e} (triplet {jw})")
    if bars.get("resid") is not None and not resid <= bars["resid"]:
        fails.append(f"[residual]: reported {resid:.2e} (bar {bars['resid']:.1e})")
    return fails, dev


def record(label, dev, bars):
    """NMFX_RECORD_BARS=<file> (tests/conftest.py): the worst-to-bar ratio per quantity, as mur_step._record writes them."""
    path = os.environ.get("NMFX_RECORD_BARS")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
        with open(path, "a") as fh:
            for q in ("values", "orth", "vectors", "recon", "resid"):
                if bars.get(q) is not None:
                    fh.write(json.dumps({"test": test, "step": f"{label} {q}", "worst_rel": float(dev[q]), "bar": bars[q],
                                         "ratio": float(dev[q] / bars[q])}) + "\n")
            fh.write(json.dumps({"test": test, "step": f"{label} sweeps", "sweeps": int(dev.get("sweeps", 0)), "cap": int(bars.get("sweep_cap", 0))}) + "\n")


# ---- the case table -------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id kind m n k kw")


def _c(cid, kind, m, n, k, **kw):
    return Case(cid, kind, m, n, k, tuple(sorted(kw.items())))


# both sides of every switch of L = first size >= max(k + 16, k + k / 2), k / 2 in integers (16 | 17, 32 | 33, 43 | 44, 64 | 65,
# 85 | 86, 107 | 108), and 48, 49, 106, 128
WIDTHS = (16, 17, 32, 33, 43, 44, 48, 49, 64, 65, 85, 86, 106, 107, 108, 128)
WIDTHS_L = (32, 48, 48, 64, 64, 96, 96, 96, 96, 128, 128, 160, 160, 160, 192, 192)
CASES = (
    [_c(f"L{block_width(k)}-k{k}", "planted", 257, 200, k) for k in WIDTHS]
    + [_c("wide-130x1000-k64", "planted", 130, 1000, 64),
       _c("L192-plain-640x384-k150", "planted", 640, 384, 150, max_sweeps=60),
       _c("L>n-700x40-k20", "planted", 700, 40, 20),
       _c("L>np-300x100-k100", "planted", 300, 100, 100),
       _c("k=n-300x24", "uniform", 300, 24, 24),
       _c("k=m-24x300", "uniform", 24, 300, 24),
       _c("1x300", "uniform", 1, 300, 1),
       _c("300x1", "uniform", 300, 1, 1),
       _c("5x7-k3", "uniform", 5, 7, 3),
       _c("zero-row-col", "zeroed", 257, 200, 12),
       _c("rank6-k10", "integer", 300, 200, 10),
       _c("tiled8-k12", "tiled", 300, 200, 12),
       _c("repeated-k6", "repeated", 300, 200, 6)]
    + [_c(f"k70-seed{s}", "planted", 257, 200, 70, seed=s) for s in (0, 1, 2, 3)]
    + [_c("k70-block70", "planted", 257, 200, 70, block=70)]
)
WIDE_BLOCK = _c("k40-block192", "planted", 257, 200, 40, block=192, max_sweeps=250)      # passes check_triplets or returns resid > tol
TWO_SWEEPS = _c("uniform-512x256-k40-2sweeps", "uniform", 512, 256, 40, max_sweeps=2)
BY_ID = {c.id: c for c in CASES + [WIDE_BLOCK, TWO_SWEEPS]}
_INPUTS = {}


def make_input(c):
    """The f32 matrix of case c (built once; read-only)."""
    key = (c.kind, c.m, c.n, c.k if c.kind in ("planted", "zeroed") else 0)
    if key not in _INPUTS:
        from oracle import nmf_ref as R
        m, n = c.m, c.n
        rs = np.random.RandomState(6)
        if c.kind == "planted":
            v = R.planted_matrix(m, n, c.k, seed=5, dtype=np.float32)
        elif c.kind == "uniform":
            v = rs.rand(m, n).astype(np.float32)
        elif c.kind == "zeroed":
            v = R.planted_matrix(m, n, c.k, seed=5, dtype=np.float32).copy()
            v[3] = 0
            v[:, 5] = 0
        elif c.kind == "integer":                   # rank 6, every entry an integer: exact in f32
            v = (rs.randint(0, 4, (m, 6)).astype(np.float64) @ rs.randint(0, 4, (6, n)).astype(np.float64)).astype(np.float32)
        elif c.kind == "tiled":                     # 8 distinct columns, 25 times
            v = np.tile(rs.rand(m, 8).astype(np.float32), (1, n // 8))
        elif c.kind == "repeated":
            ug, _ = np.linalg.qr(rs.randn(m, 12))
            vg, _ = np.linalg.qr(rs.randn(n, 12))
            v = ((ug * np.array([5, 3, 3, 3, 2, 2, 1, 1, 1, 1, .5, .25])) @ vg.T).astype(np.float32)
        else:
            raise ValueError(c.kind)
        v = np.ascontiguousarray(v, dtype=np.float32)
        v.setflags(write=False)
        _INPUTS[key] = v
    return _INPUTS[key]


def measure_bars(c, seeds=(0, 1, 2, 3)):
    """The bars of case c as tests/test_svd_bars.py derives them: max(documented, 10 x the worst of the emulations) per
    quantity, sweep_cap = 2 x the most sweeps + 2.  Also returns the worst deviations themselves."""
    v, kw = make_input(c), dict(c.kw)
    kw.pop("seed", None)
    worst, sweeps = dict(values=0.0, orth=0.0, vectors=0.0, recon=0.0, resid=0.0), 0
    for sd in seeds:
        u, s, vt, sw, resid, _ = emulate_topk(v, c.k, seed=sd, **kw)
        _, dev = check_triplets(v, u, s, vt, resid, c.k, DOC)
        worst = {q: max(worst[q], dev[q]) for q in worst}
        sweeps = max(sweeps, sw)
    bars = {q: max(DOC[q], 10.0 * worst[q]) for q in worst}
    # the reported residual is what the stop test compares with tol = 1e-11: its bar is tol itself, or none where the
    # emulation itself has not converged within the case's max_sweeps
    bars["resid"] = DOC["resid"] if worst["resid"] <= DOC["resid"] else None
    bars["sweep_cap"] = 2 * sweeps + 2
    return bars, worst, sweeps


# id: (bars above the documented ones {quantity: bar}, sweep_cap, the emulation's worst (values, orth, vectors, recon, resid), its
# most sweeps) over seeds 0..3 -- written by `python tests/svd_ref.py`, held to a fresh measurement by tests/test_svd_bars.py.
TABLE = {
    "L32-k16": ({'values': 2.4e-12}, 10, (2.3e-13, 4.6e-13, 6.6e-13, 2.9e-12, 2.9e-12), 4),
    "L48-k17": ({'values': 2.9e-12}, 10, (2.8e-13, 5.5e-13, 3.6e-13, 1.7e-12, 1.7e-12), 4),
    "L48-k32": ({'values': 5.3e-12}, 10, (5.0e-13, 1.0e-12, 5.0e-13, 2.1e-12, 2.1e-12), 4),
    "L64-k33": ({}, 574, (6.2e-14, 1.3e-13, 3.4e-13, 8.0e-12, 7.4e-12), 286),
    "L64-k43": ({}, 20, (3.3e-15, 2.9e-15, 4.2e-16, 6.9e-12, 5.3e-12), 9),
    "L96-k44": ({}, 1320, (2.8e-15, 4.2e-15, 5.0e-16, 1.3e-11, 9.7e-12), 659),
    "L96-k48": ({}, 52, (2.7e-15, 3.1e-12, 5.1e-16, 1.2e-11, 9.4e-12), 25),
    "L96-k49": ({}, 20, (2.4e-15, 3.8e-15, 2.9e-16, 1.2e-11, 9.5e-12), 9),
    "L96-k64": ({}, 30, (2.0e-14, 6.3e-12, 4.3e-16, 1.7e-11, 8.4e-12), 14),
    "L128-k65": ({}, 46, (3.4e-15, 1.2e-12, 2.9e-16, 1.2e-11, 9.2e-12), 22),
    "L128-k85": ({'values': 1.3e-12, 'orth': 1.4e-10}, 46, (1.2e-13, 1.3e-11, 2.9e-16, 1.3e-11, 8.0e-12), 22),
    "L160-k86": ({'orth': 1.8e-10}, 34, (4.2e-15, 1.7e-11, 4.2e-16, 7.3e-12, 5.9e-12), 16),
    "L160-k106": ({'orth': 1.8e-10}, 52, (5.0e-14, 1.7e-11, 5.1e-16, 1.6e-11, 9.6e-12), 25),
    "L160-k107": ({'values': 4.4e-12, 'orth': 2.1e-10}, 50, (4.2e-13, 2.0e-11, 4.0e-16, 1.5e-11, 8.7e-12), 24),
    "L192-k108": ({'values': 9.2e-12, 'orth': 4.6e-10}, 38, (8.8e-13, 4.3e-11, 9.4e-16, 1.4e-11, 8.8e-12), 18),
    "L192-k128": ({'values': 1.2e-11, 'orth': 1.1e-09}, 44, (1.2e-12, 1.1e-10, 4.0e-16, 6.2e-12, 4.8e-12), 21),
    "wide-130x1000-k64": ({}, 32, (4.8e-15, 3.3e-12, 7.2e-16, 1.6e-11, 9.1e-12), 15),
    "L192-plain-640x384-k150": ({'orth': 4.5e-10}, 84, (6.8e-14, 4.3e-11, 3.1e-16, 3.5e-11, 9.6e-12), 41),
    "L>n-700x40-k20": ({'values': 3.2e-12}, 4, (3.0e-13, 6.0e-13, 3.3e-13, 2.7e-14, 2.7e-14), 1),
    "L>np-300x100-k100": ({'values': 2.3e-10, 'orth': 4.7e-10}, 4, (2.2e-11, 4.4e-11, 9.2e-16, 3.2e-15, 2.5e-13), 1),
    "k=n-300x24": ({}, 4, (4.4e-15, 1.1e-14, 1.3e-13, 4.2e-15, 2.4e-15), 1),
    "k=m-24x300": ({}, 6, (2.2e-15, 3.1e-15, 4.4e-14, 2.3e-15, 1.6e-15), 2),
    "1x300": ({}, 6, (1.1e-15, 1.2e-15, 9.7e-17, 1.7e-15, 1.7e-15), 2),
    "300x1": ({}, 4, (1.1e-15, 1.7e-15, 6.7e-16, 8.5e-16, 3.4e-15), 1),
    "5x7-k3": ({}, 4, (1.2e-15, 2.0e-15, 4.8e-15, 2.8e-15, 1.9e-15), 1),
    "zero-row-col": ({'values': 1.2e-12}, 10, (1.2e-13, 2.3e-13, 7.2e-13, 3.2e-12, 3.3e-12), 4),
    "rank6-k10": ({}, 12, (1.6e-15, 2.0e-15, 2.4e-15, 1.8e-15, 1.0e-15), 5),
    "tiled8-k12": ({}, 12, (2.0e-15, 3.8e-15, 5.8e-15, 2.4e-15, 1.3e-15), 5),
    "repeated-k6": ({}, 10, (1.8e-15, 2.7e-15, 5.0e-16, 2.6e-15, 3.0e-15), 4),
    "k70-seed0": ({'orth': 1.7e-10}, 34, (3.7e-15, 1.6e-11, 3.7e-16, 1.0e-11, 6.8e-12), 16),
    "k70-seed1": ({'orth': 1.7e-10}, 34, (3.7e-15, 1.6e-11, 3.7e-16, 1.0e-11, 6.8e-12), 16),
    "k70-seed2": ({'orth': 1.7e-10}, 34, (3.7e-15, 1.6e-11, 3.7e-16, 1.0e-11, 6.8e-12), 16),
    "k70-seed3": ({'orth': 1.7e-10}, 34, (3.7e-15, 1.6e-11, 3.7e-16, 1.0e-11, 6.8e-12), 16),
    "k70-block70": ({'orth': 1.4e-10}, 38, (4.4e-15, 1.3e-11, 3.5e-16, 1.2e-11, 7.6e-12), 18),
    "k40-block192": ({}, 16, (2.3e-15, 3.3e-15, 3.7e-16, 3.9e-12, 2.4e-12), 7),
}


def bars_of(c):
    over, cap = TABLE[c.id][0], TABLE[c.id][1]
    return dict(DOC, **over, sweep_cap=cap)


if __name__ == "__main__":
    for case in CASES + [WIDE_BLOCK]:
        b, w, sw = measure_bars(case)
        over = {q: (None if b[q] is None else float(f"{b[q] * 1.05:.1e}")) for q in DOC if b[q] is None or b[q] > DOC[q]}     # (rounded up)
        print(f'    "{case.id}": ({over}, {b["sweep_cap"]}, ({w["values"]:.1e}, {w["orth"]:.1e}, {w["vectors"]:.1e}, {w["recon"]:.1e}, {w["resid"]:.1e}), {sw}),')
