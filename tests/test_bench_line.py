"""The ONE stdout line of bench.py must stay small enough for the driver to parse: the compact
headline is built from the full record by bench.headline(); the full record goes to bench_detail.json / stderr."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _detail():
    with open(os.path.join(ROOT, "profiles", "r04_bench_n1.json")) as f:      # a real full record (27.8 KB: the one the driver could not parse)
        return json.load(f)


def test_headline_fits_and_keeps_the_contract():
    import bench
    d = _detail()
    assert len(json.dumps(d)) > 20000
    line = bench.headline(d)
    text = json.dumps(line)
    assert len(text) < bench.HEADLINE_LIMIT <= 4096
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline", "parity"):
        assert key in line, key
    assert line["value"] == d["value"] and line["ms_per_step"] == d["ms_per_step"]
    assert set(line["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    assert set(line["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"}
    assert abs(line["roofline"]["frac"] - d["roofline"]["frac"]) < 1e-4
    for cfg in ("cfg3", "cfg4", "cfg5_on_1_gpu"):
        assert line[cfg]["iter_per_s"] > 0 and 0 < line[cfg]["frac_of_hbm_peak"] < 1
    assert line["exact_f32_iter_per_s"] > 0
    assert "cfg5_n8" in line["scaling_model_predicted_speedup"]
    assert "\n" not in text


def test_headline_sheds_optional_slots_rather_than_grow():
    import bench
    d = _detail()
    d["time_to_tol"] = d["time_to_tol"] * 40                      # something upstream grew
    d["config"]["workload"] = d["config"]["workload"] + " x" * 200
    line = bench.headline(d)
    assert len(json.dumps(line)) < bench.HEADLINE_LIMIT
    assert "roofline" in line and "cpu_baseline" in line and "value" in line


def test_headline_without_optional_legs():
    import bench
    d = _detail()
    for k in ("other_configs", "scaling_model", "time_to_tol", "parity", "cpu_baseline"):
        d[k] = None
    line = bench.headline(d)
    assert line["cpu_baseline"] is None and line["parity"] is None and "cfg3" not in line


def test_this_rounds_record_and_line_agree():
    """profiles/r05_bench_n1.json is the line bench.py printed, profiles/r05_bench_n1_detail.json the record it was built from: the same
    function gives the same line, and the fused KL-ADMM legs carry their stream counts (3 per AO-ADMM round, 4 for ADMM's stored S)."""
    import bench
    with open(os.path.join(ROOT, "profiles", "r05_bench_n1.json")) as f:
        printed = json.loads(f.read().strip().splitlines()[-1])
    with open(os.path.join(ROOT, "profiles", "r05_bench_n1_detail.json")) as f:
        detail = json.load(f)
    assert len(json.dumps(printed)) < bench.HEADLINE_LIMIT
    rebuilt = bench.headline(detail)
    for key in ("value", "ms_per_step", "roofline", "cpu_baseline", "parity", "cfg3", "cfg4", "cfg5_on_1_gpu"):
        assert rebuilt[key] == printed[key], key
    legs = {leg["config"]: leg for leg in detail["other_configs"] if "config" in leg}
    ao = legs["aoadmm_kl_on_cfg3_shape"]["dominant_kernel"]
    assert ao["name"] == "kl_vaux_fused" and ao["algorithmic_bytes_per_launch"] == 3 * 16384 * 8192 * 4.0
    assert 0.3 < ao["frac"] < 1.0


def test_dump_outputs_writes_float64_whole_or_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: float64 .npy files, whole while they fit in DUMP_LIMIT; past it the large arrays keep the same seeded
    sample of their elements on every run and the files stay inside the limit."""
    import numpy as np

    import bench
    w = np.arange(3000, dtype=np.float32).reshape(300, 10)
    h = np.arange(200, dtype=np.float32).reshape(10, 20)
    obj = np.linspace(2.0, 1.0, 5)
    bench.dump_outputs(str(tmp_path / "whole"), {"w": w, "h": h, "obj_history": obj})
    for name, a in (("w", w), ("h", h), ("obj_history", obj)):
        got = np.load(tmp_path / "whole" / (name + ".npy"))
        assert got.dtype == np.float64 and got.shape == a.shape and np.array_equal(got, a)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 8 * 1200)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"w": w, "h": h, "obj_history": obj})
    files = sorted((tmp_path / "a").iterdir())
    assert sum(np.load(f).nbytes for f in files) <= bench.DUMP_LIMIT
    wa, wb = np.load(tmp_path / "a" / "w.npy"), np.load(tmp_path / "b" / "w.npy")
    assert wa.dtype == np.float64 and wa.size == 400 and np.array_equal(wa, wb)
    assert np.all(np.diff(wa) > 0) and np.isin(wa, w).all()        # elements of w, in index order
    assert np.array_equal(np.load(tmp_path / "a" / "h.npy"), h)      # within its share: whole


def test_bench_arguments_refuse_what_cannot_be_honoured(monkeypatch, capsys):
    import pytest

    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("NMFX_BENCH_FORCE_SHARDED", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.dump_outputs) == (7, 2, "out")
    for argv in (["--steps", "0"], ["--gpus", "2", "--dump-outputs", "out"]):
        monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
        with pytest.raises(SystemExit):
            bench.parse()


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("NMFX_BENCH_FORCE_SHARDED", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--full"])
    assert bench.parse().full is True


def _run_bench(cwd, *extra):
    import subprocess
    cwd.mkdir()
    env = dict(os.environ, NMFX_BENCH_SHAPE="1024x512x64", NMF_AMD_QUIET="1", NMFX_BENCH_DETAIL=str(cwd / "detail.json"))
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "NMFX_BENCH_FORCE_SHARDED"):
        env.pop(key, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", *extra],
                       env=env, cwd=str(cwd), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), json.loads((cwd / "detail.json").read_text())


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_full_adds_the_legs(tmp_path):
    """A plain run times the steps and prints the line with the other legs empty; --full runs the per-kernel pass and roofline
    (the CPU, traffic and time-to-tol legs are left out here: the shrunken shape has no other configs either)."""
    line, detail = _run_bench(tmp_path / "plain")
    assert line["value"] > 0 and line["steps"] == 4 and line["warmup"] == 2 and line["higher_is_better"] is True
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e-6
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity"] is None and "time_to_tol" not in line
    assert not detail["kernels"] and detail["other_configs"] is None and detail["scaling_model"] is None
    line, detail = _run_bench(tmp_path / "full", "--full", "--no-cpu", "--no-traffic", "--tol-max-iter", "0")
    assert line["value"] > 0 and line["roofline"]["frac"] > 0 and "wphase" in detail["kernels"]
