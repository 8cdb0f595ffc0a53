"""The two tools of SPEC §14 still run against the package: each case is one tool as a fresh child process, at its smallest
size, under tests/test_gpu_tools.py's rules (own time limit; no further child after one that ended by a signal)."""
import json
import re

import pytest

from test_gpu_tools import tool

pytestmark = pytest.mark.gpu


def test_rollout_bench_choose_runs_one_round_on_both_layouts():
    out = tool("rollout_bench.py", "--choose", "--sizes", 64, "--k", 4, "--rounds", 1).strip().splitlines()
    rows = [json.loads(ln) for ln in out]
    assert [r["layout"] for r in rows] == ["chain", "sibling"] and all(r["n_envs"] == 64 and r["k"] == 4 for r in rows)
    for r in rows:
        assert r["record_kernel_us_per_step"] > 0 and r["choose_us_per_step"] > 0
        assert abs(r["choose_over_record"] - r["choose_us_per_step"] / r["record_kernel_us_per_step"]) < 1e-2
    assert rows[0]["choose_overrides_per_env_step"] == 0          # a chain: at most one candidate
    assert rows[0]["choose_offers_per_env_step"] == rows[0]["record_offers_per_env_step"]


def test_choice_report_prints_both_trees(tmp_path):
    out = tool("choice_report.py", "--maps", "pinball_simple", "--seeds", 1, "--envs", 256, "--warm", 40, "--after", 8,
               "--steps-per-option", 16, "--episodes", 128, "--record-envs", 16, "--out-dir", tmp_path).splitlines()
    assert out[0].startswith("# choice_report map pinball_simple envs 256 ")
    heads = [ln for ln in out if ln.startswith("seed 1 ")]
    assert len(heads) == 2 and heads[0].startswith("seed 1 discovered: ") and heads[1].startswith("seed 1 hand-set sibling tree: ")
    assert [ln.split()[0] for ln in out if ln.startswith("  ")] == ["lowest", "value", "offers", "delta"] * 2
    value = [ln for ln in out if ln.startswith("  value")]
    assert all(re.search(r"overrides \[0(, \d+){5}\]$", ln) for ln in value)
    offers = re.match(r"  offers +(\d+) on 16 recorded episodes, (\d+) with two or more candidates", [ln for ln in out if ln.startswith("  offers")][1])
    assert int(offers.group(1)) >= int(offers.group(2)) > 0, "the hand-set tree offered no env two candidates"
    assert (tmp_path / "r11_choice_report_pinball_simple.txt").read_text().splitlines() == out
