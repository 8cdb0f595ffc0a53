"""SPEC §31.4's measuring tool end to end at toy size: tools/fit_pipeline_bench.py --solver."""
import pytest

pytestmark = pytest.mark.gpu


def test_solver_bench_runs_end_to_end_at_toy_size(tmp_path):
    from test_gpu_tools import tool
    out = tool("fit_pipeline_bench.py", "--solver", "--envs", 256, "--options", 1, "--episodes", 32, "--sweeps", 1, "--rounds", 3, "--toy",
               "--out", tmp_path / "bench.txt").splitlines()
    assert out[0].startswith("# fit_pipeline_bench --solver envs 256 options 1 episodes 32 ") and " rounds 3 (toy) " in out[0]
    assert (tmp_path / "bench.txt").read_text().splitlines() == out
    assert out[1] == "equal by bits: host arm twice True, device arm twice True, device arm under pipeline='device' True"
    arms = [ln.split() for ln in out if " median " in ln]
    assert [r[0] for r in arms] == ["host", "torch", "device"] + ["scg_ridge_solve", "torch"] * 2
    assert all(float(r[5]) <= float(r[2]) <= float(r[7]) and r[-1] == "3" for r in arms)      # min <= median <= max, three rounds each
    assert sum(" separated " in ln for ln in out) == 2
    rows = [ln.split() for ln in out if ln.split()[:1] in (["host"], ["torch"], ["device"]) and " median " not in ln and " / " not in ln]
    assert [r[0] for r in rows] == ["host", "torch", "device"] and all(len(r) == 8 for r in rows)
    assert all(abs(sum(float(v) for v in r[1:7]) - float(r[7])) < 0.5 for r in rows)           # the parts add up to the total
    alone = [ln for ln in out if ln.startswith("the call alone, ")]
    assert len(alone) == 2 and all("info all 0: True" in ln for ln in alone)
