"""bench.py's one-line JSON contract, checked on the committed GPU-box lines (no GPU here): the driver, the judge and
tools/ab_bench.py all parse these fields."""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lines():
    out = []
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench_default.json")) +
                    glob.glob(os.path.join(ROOT, "profiles", "r*_bench_20_steps.json")) +
                    glob.glob(os.path.join(ROOT, "profiles", "r*_rehearsal_*.json"))):
        d = json.load(open(p))
        if "ranks" in d:                                  # lines written since round 3 (earlier rounds' lines predate some fields)
            out.append((os.path.basename(p), d))
    assert len(out) >= 4
    return out


def test_committed_bench_lines_carry_the_contract_fields():
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    with_cpu = 0
    for name, d in _lines():
        assert d["metric"] == base["metric"], name
        assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["scaling"] == "weak", name
        assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None, name
        assert d["value"] > 1e8 and d["n_gpus"] >= 1 and d["steps"] >= 1, name
        assert abs(d["value"] - d["config"]["envs_per_gpu"] * d["n_gpus"] / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"], name
        cfg = d["config"]
        assert "workload" in cfg and "model" not in cfg and cfg["envs_per_gpu"] == 65536 and cfg["n_options"] == 5, name
        assert "untimed_ramp_steps" in cfg and cfg["backend"] in ("none", "nccl", "gloo"), name
        r = d["roofline"]
        assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0, name
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and r["kernel_ms"] > 0, name
        # the source says whether this run measured it (two rocprofv3 counter passes run first) or read the tracked profile
        assert r["traffic"] is None or (r["traffic"] > 1e7 and ("(static" in r["traffic_source"] or r["traffic_source"].startswith("measured by this run"))), name
        if r["traffic"] is not None and r["traffic_source"].startswith("measured by this run"):
            kb = r["traffic_counters_kb"]
            assert r["traffic"] == int((2.0 * kb["FETCH_SIZE"] + kb["WRITE_SIZE"]) * 1024), name
        m = d["mfma"]
        assert m["bound"] == "mfma" and m["peak"] == 157.3 and 0.05 < m["frac"] < 1.0, name
        rk = d["ranks"]
        assert rk["world_size_seen"] == d["n_gpus"] and rk["ms_per_step_min"] <= rk["ms_per_step_max"], name
        if d["n_gpus"] == 1 and d["cpu_baseline"] is not None:      # (None: a line taken with --no-cpu-baseline)
            cb = d["cpu_baseline"]
            assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb, name
            with_cpu += 1
        else:
            assert d["cpu_baseline"] is None, name
        if "shared option-Q weights" in cfg["workload"]:
            ar = rk["allreduce"]
            assert ar["samples"] >= 1 and ar["bytes"] == (6 * 5 * 1296 + 6) * 4 and ar["mean_us"] > 0, name
        else:
            assert rk["allreduce"] is None, name
    assert with_cpu >= 2                                            # the default and the driver-form line of the final build


def test_traffic_files_are_consistent_with_the_pmc_summary():
    for name in ("r03_traffic.json", "r04_traffic.json"):
        t = json.load(open(os.path.join(ROOT, "profiles", name)))
        assert t["traffic_bytes_per_launch"] == int((2 * t["fetch_size_kb"] + t["write_size_kb"]) * 1024), name
        assert abs(t["traffic_over_algorithmic"] - t["traffic_bytes_per_launch"] / t["algorithmic_bytes_per_launch"]) < 1e-9, name
        assert t["algorithmic_bytes_per_launch"] == 65536 * 46, name


def test_bench_reads_the_newest_traffic_file():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'TRAFFIC_FILES = ("r05_traffic.json"' in src
    assert os.path.exists(os.path.join(ROOT, "profiles", "r05_traffic.json"))


def test_round_4_lines_carry_the_extra_measurements():
    """the small config and the DISCOVERED chain as extra keys beside the headline (which stays as it was)."""
    seen = 0
    for name, d in _lines():
        if not name.startswith("r04_") or "rehearsal" in name:      # (the 2-rank rehearsal lines are taken with --no-extras)
            continue
        ex = d.get("extras")
        assert ex is not None, name
        c1, dc = ex["config1_4096_envs_root_plus_1_option"], ex["discovered_chain_65536_envs"]
        assert c1["unit"] == dc["unit"] == "env-steps/s" and c1["workgroups"] == 16 and c1["value"] > 1e7, name
        assert abs(c1["value"] - 4096 / (c1["us_per_step"] * 1e-6)) < 1e-3 * c1["value"], name
        assert 1 <= dc["options_created"] <= 5 and len(dc["fit_accuracy"]) == dc["options_created"], name
        assert sum(dc["envs_per_running_option_at_end"]) == 65536, name
        assert dc["envs_in_an_option_at_end"] == sum(dc["envs_per_running_option_at_end"][1:]), name
        assert abs(dc["value"] - 65536 / (dc["us_per_step"] * 1e-6)) < 1e-3 * dc["value"], name
        seen += 1
    assert seen >= 2


def test_live_traffic_never_starts_counter_passes_from_a_profiled_process(monkeypatch):
    """bench.py measures roofline.traffic with two rocprofv3 child passes run before it touches the GPU. Under a profiler the
    process has the GPU open from its first instruction (the tool's preloaded library): no child may be started from it —
    the guard reads exactly the variables rocprofv3 7.2 sets for its child (checked in this image), and the line falls back
    to the tracked static figure."""
    import subprocess
    sys.path.insert(0, ROOT)
    import bench
    def boom(*a, **k):
        raise AssertionError("live_traffic started a child process from a profiled process")
    monkeypatch.setattr(subprocess, "run", boom)
    for var, val in (("ROCPROFILER_LIBRARY_CTOR", "1"), ("ROCP_TOOL_LIBRARIES", "/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so"),
                     ("ROCPROF_KERNEL_TRACE", "1"), ("LD_PRELOAD", "/opt/rocm/lib/rocprofiler-sdk/librocprofiler-sdk-tool.so"), ("HSA_TOOLS_LIB", "libx.so")):
        monkeypatch.setenv(var, val)
        assert bench.live_traffic(65536, 5) is None, var
        monkeypatch.delenv(var)


class _FakeAgent:
    """What dump_outputs reads from a SkillChainingAgent: the env state SoA and W (host tensors here)."""
    _STATE_FIELDS = ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "qcache", "action", "reward", "done")

    def __init__(self, n):
        import types
        import torch
        g = torch.Generator().manual_seed(1)
        f32 = lambda *s: torch.randn(*s, generator=g)
        i32 = lambda: torch.randint(-5, 3000, (n,), generator=g, dtype=torch.int32)
        u8 = lambda: torch.randint(0, 5, (n,), generator=g, dtype=torch.uint8)
        self.n_envs = n
        self.W = f32(6, 5, 1296)
        self.state = types.SimpleNamespace(x=f32(n), y=f32(n), vx=f32(n), vy=f32(n), option_id=i32(), opt_steps=i32(),
                                           ep_steps=i32(), qcache=f32(5, n), action=u8(), reward=f32(n), done=u8())


def test_dump_outputs_writes_every_array_exactly_and_samples_beyond_the_limit(tmp_path, monkeypatch):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    ag = _FakeAgent(4096)
    d = tmp_path / "full"
    info = bench.dump_outputs(ag, str(d))
    assert not info["sampled"] and info["envs"] == 4096
    assert (d / ".gitignore").read_text() == "*\n"
    for f in ag._STATE_FIELDS + ("W",):
        a = np.load(d / (f + ".npy"))
        src = (ag.W if f == "W" else getattr(ag.state, f)).numpy()
        assert a.dtype in (np.float32, np.float64) and a.shape == src.shape, f
        assert np.array_equal(a, src.astype(a.dtype)) and np.array_equal(a.astype(src.dtype), src), f
    assert not (d / "env_index.npy").exists()

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 18)                 # force the seeded sample
    runs = []
    for name in ("a", "b"):
        info = bench.dump_outputs(ag, str(tmp_path / name))
        assert info["sampled"] and 0 < info["envs"] < 4096
        total = sum(p.stat().st_size for p in (tmp_path / name).glob("*.npy"))
        assert total <= 1 << 18
        runs.append({p.stem: np.load(p) for p in (tmp_path / name).glob("*.npy")})
    idx = runs[0]["env_index"].astype(np.int64)
    assert np.array_equal(runs[0]["env_index"], runs[1]["env_index"]) and np.all(np.diff(idx) > 0)
    assert np.array_equal(runs[0]["qcache"], ag.state.qcache.numpy()[:, idx])
    assert np.array_equal(runs[0]["option_id"], ag.state.option_id.numpy()[idx].astype(np.float64))
    assert np.array_equal(runs[0]["W"], ag.W.numpy())


def test_bench_refuses_zero_timed_steps():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr
