"""Time one MUR iteration with the Itakura-Saito divergence (kernels_phase.hip, IsEntry) beside exact-f32 MUR-KL on the same matrix.

    python tools/is_perf.py --m 16384 --n 8192 --k 64 128
    python tools/is_perf.py --k 64 --kl-lib /path/to/another/libnmfx.so       # KL from another build (e.g. the parent commit's)

Both run under NMFX_PRECISION=f32 in one process, alternated, on the same seeded strictly positive matrix and start:
warmed batches between device events, best of --reps.  One JSON line per k: ms per iteration of both, their ratio, and per
IS product kernel (events around every launch, a run of its own) its time and the fraction of the HBM peak that one pass
over V in that time amounts to.  --kl-lib loads the second library privately (its own symbols first) and drives it
through the C ABI directly."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NMF_AMD_QUIET", "1")
os.environ["NMFX_PRECISION"] = "f32"

import numpy as np

HBM_PEAK = 8.0e12          # bytes / s (MI355X)
NEVER = 10 ** 12


class ForeignKL:
    """MUR-KL on another build of libnmfx, through its C ABI."""

    def __init__(self, path, v, w0, h0, stream):
        from nmf_amd import _lib as L
        self.lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        for name in ("nmfx_create", "nmfx_destroy", "nmfx_upload_v", "nmfx_set_factors", "nmfx_mur_run", "nmfx_set_stream",
                     "nmfx_reset_stream", "nmfx_get_state", "nmfx_get_precision", "nmfx_version"):
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = L.SIGNATURES[name]
        self.h = C.c_void_p()
        m, n = v.shape
        self.ck(self.lib.nmfx_create(C.byref(self.h), 0, m, n, w0.shape[1]))
        self.ck(self.lib.nmfx_set_stream(self.h, stream))
        self.ck(self.lib.nmfx_upload_v(self.h, v.ctypes.data_as(C.c_void_p), L.F32, n, 0, m))
        self.ck(self.lib.nmfx_set_factors(self.h, w0.ctypes.data_as(C.c_void_p), h0.ctypes.data_as(C.c_void_p)))
        self.version = self.lib.nmfx_version()

    def ck(self, rc):
        if rc:
            raise RuntimeError(f"foreign libnmfx: error {rc}")

    def mur_run(self, dist, lw, lh, min_iter, tol1, tol2, first, count):
        self.ck(self.lib.nmfx_mur_run(self.h, dist, lw, lh, min_iter, tol1, tol2, first, count))

    def precision(self):
        return "bf16" if self.lib.nmfx_get_precision(self.h) == 1 else "f32"

    def state(self):
        rule, stop_i, n_obj = C.c_int(), C.c_int64(), C.c_int64()
        self.ck(self.lib.nmfx_get_state(self.h, C.byref(rule), C.byref(stop_i), C.byref(n_obj)))
        return rule.value, stop_i.value, n_obj.value

    def close(self):
        self.lib.nmfx_reset_stream(self.h)
        self.lib.nmfx_destroy(self.h)


def timed(eng, dist, first, count, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    eng.mur_run(dist, 0.0, 0.0, NEVER, 1e-30, 1e-30, first, count)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=16384)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--k", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kl-lib", default=None, help="time MUR-KL on this build of libnmfx.so instead of the loaded one")
    a = ap.parse_args()

    import torch
    from nmf_amd import _lib as L
    from nmf_amd.engine import Engine
    rng = np.random.default_rng(a.seed)
    v = (rng.random((a.m, 16), dtype=np.float32) @ rng.random((16, a.n), dtype=np.float32)) / 16 + np.float32(0.01)
    stream = torch.cuda.current_stream().cuda_stream
    for k in a.k:
        w0 = np.ascontiguousarray(rng.uniform(0.1, 1.0, (a.m, k)))
        h0 = np.ascontiguousarray(rng.uniform(0.1, 1.0, (k, a.n)))
        ie = Engine(a.m, a.n, k)
        ie.set_stream(stream)
        ie.upload_v(v)
        ie.set_factors(w0, h0)
        if a.kl_lib:
            ke = ForeignKL(a.kl_lib, v, w0, h0, stream)
        else:
            ke = Engine(a.m, a.n, k)
            ke.set_stream(stream)
            ke.upload_v(v)
            ke.set_factors(w0, h0)
        legs = {"is": (ie, L.IS), "kl": (ke, L.KL)}
        done = {name: 0 for name in legs}
        ms = {name: [] for name in legs}
        for name, (eng, dist) in legs.items():          # warm-up batch
            timed(eng, dist, 0, 3, torch)
            done[name] = 3
        for _ in range(a.reps):
            for name, (eng, dist) in legs.items():
                ms[name].append(timed(eng, dist, done[name], a.iters, torch))
                done[name] += a.iters
        for name, (eng, _) in legs.items():
            assert eng.state()[0] == 0, f"{name}: the stop rule fired during timing"
        # per-kernel times of the IS iteration: events around every launch, so a run of its own
        ie.lib.nmfx_profile_enable(ie.h, 1)
        ie.lib.nmfx_profile_reset(ie.h)
        ie.mur_run(L.IS, 0.0, 0.0, NEVER, 1e-30, 1e-30, done["is"], a.iters)
        kernels = {}
        mp, np_ = -(-a.m // 128) * 128, -(-a.n // 128) * 128
        for name in ("is_wphase", "w_update", "is_hphase", "h_update"):
            tot, cnt = C.c_double(), C.c_int64()
            ie.lib.nmfx_profile_get(ie.h, name.encode(), C.byref(tot), C.byref(cnt))
            per = tot.value / max(1, cnt.value)
            kernels[name] = {"ms": round(per, 4)}
            if name.startswith("is_") and per > 0:
                kernels[name]["hbm_fraction"] = round(mp * np_ * 4 / (per * 1e-3) / HBM_PEAK, 3)
        ie.lib.nmfx_profile_enable(ie.h, 0)
        out = {"m": a.m, "n": a.n, "k": k, "is_ms_per_iter": round(min(ms["is"]), 4), "kl_f32_ms_per_iter": round(min(ms["kl"]), 4),
               "ratio": round(min(ms["is"]) / min(ms["kl"]), 3), "kl_precision": ke.precision(),
               "kl_library": a.kl_lib or L.LIB_PATH, "kl_library_version": ke.version if a.kl_lib else L.load().nmfx_version(),
               "is_ms_all": [round(t, 4) for t in ms["is"]], "kl_ms_all": [round(t, 4) for t in ms["kl"]], "is_kernels": kernels}
        print(json.dumps(out), flush=True)
        for eng in (ie, ke):
            if isinstance(eng, Engine):
                eng.reset_stream()
            eng.close()


if __name__ == "__main__":
    main()
