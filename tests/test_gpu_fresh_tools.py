"""SPEC §30.4's two tools end to end at toy size: tools/fresh_fit_report.py and tools/fit_pipeline_bench.py."""
import pytest

pytestmark = pytest.mark.gpu


def test_fresh_fit_report_runs_end_to_end_at_toy_size(tmp_path):
    from test_gpu_tools import tool
    out = tool("fresh_fit_report.py", "--maps", "pinball_simple", "--seeds", 1, "--envs", 256, "--warm", 40, "--after", 8, "--steps-per-option", 16,
               "--min-examples", 64, "--episodes", 64, "--options", 2, "--lambdas", 0.5, "--sweeps", 2, "--eval-episodes", 64,
               "--out-dir", tmp_path).splitlines()
    assert out[0].startswith("# fresh_fit_report map pinball_simple envs 256 ")
    assert (tmp_path / "r36_fresh_fit_pinball_simple.txt").read_text().splitlines() == out
    arms = {("peng", "0.00"), ("peng", "0.50"), ("watkins", "0.50")}
    kept = [ln.split() for ln in out if ln.startswith("    ") and ln.split()[0] in ("peng", "watkins") and len(ln.split()) == 12]
    fresh = [ln.split() for ln in out if ln.startswith("    fresh/") and len(ln.split()) == 12 and ln.split()[1] != "lambda"]
    assert len(kept) == len(fresh) == 3 * 2 * 3                # three (arm, lambda) pairs; two sweeps; three value functions
    assert {(r[0], r[1]) for r in kept} == arms == {(r[0][len("fresh/"):], r[1]) for r in fresh}
    first = lambda rows: [r[1:11] for r in rows if r[2] == "1"]
    assert first(kept) == first(fresh)                         # sweep 1 of the fresh arm is the kept arm's
    ran = [r for r in fresh if int(r[4]) + int(r[5]) > 0]
    assert ran and all(0.0 <= float(r[6]) <= 1.0 and float(r[7]) >= 1.0 for r in ran)
    assert all(0.0 <= float(r[11]) <= 1.0 for r in fresh if r[2] == "2")                  # the sweep's own record's success rate
    assert any("the fresh arm's sweep 1 equals the kept arm's by bits" in ln for ln in out)
    pol = [ln.split() for ln in out if "+-" in ln and " table " not in ln]
    assert len(pol) == (1 + 3 * 2 + 3) * 2 and [p[0] for p in pol[:2]] == ["W", "W"] and pol[-1][0] == "fresh/watkins/0.50/2"
    assert all(float(p[5]) == 0.0 and float(p[7]) == 0.0 for p in pol[:2])       # W against itself: exact zeros
    descent = [ln.split() for ln in out if ln.startswith("  descent ")]
    assert len(descent) == 2 * 3 * 2 and all(len(d) == 5 + 2 for d in descent)
    assert [d[5] for d in descent[:6]] == [d[5] for d in descent[6:]]          # sweep 1: one table for both record arms


def test_fit_pipeline_bench_runs_end_to_end_at_toy_size(tmp_path):
    from test_gpu_tools import tool
    out = tool("fit_pipeline_bench.py", "--envs", 256, "--options", 1, "--episodes", 32, "--sweeps", 1, "--rounds", 3, "--toy",
               "--out", tmp_path / "bench.txt").splitlines()
    assert out[0].startswith("# fit_pipeline_bench envs 256 options 1 episodes 32 ") and " rounds 3 (toy) " in out[0]
    assert (tmp_path / "bench.txt").read_text().splitlines() == out
    assert out[1] == "record_episodes: same_bits True" and out[5].endswith("same_bits True")
    arms = [ln.split() for ln in out if " median " in ln]
    assert [r[0] for r in arms] == ["record_host", "record_device", "fit_host", "fit_device"]
    assert all(float(r[5]) <= float(r[2]) <= float(r[7]) and r[-1] == "3" for r in arms)      # min <= median <= max, three rounds each
    assert sum(" separated " in ln for ln in out) == 2 and out[-1].startswith("per sweep: host ")
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "fit_pipeline_bench.py"), "--rounds", "3"], capture_output=True, text=True)
    assert p.returncode != 0 and "at least 9" in p.stderr                           # a measurement takes nine rounds (refused before any import of torch)
