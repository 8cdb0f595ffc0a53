"""The two tools of SPEC §15 still run against the package: each case is one tool as a fresh child process, at its smallest
size, under tests/test_gpu_tools.py's rules (own time limit; no further child after one that ended by a signal)."""
import json
import re

import pytest

from test_gpu_tools import tool

pytestmark = pytest.mark.gpu


def test_rollout_bench_audit_runs_one_round_for_the_four_rules():
    out = tool("rollout_bench.py", "--audit", "--sizes", 64, "--k", 4, "--rounds", 1).strip().splitlines()
    rows = [json.loads(ln) for ln in out]
    assert [r["rules"] for r in rows] == ["none", "interrupt", "best", "best+interrupt"]
    for r in rows:
        assert r["n_envs"] == 64 and r["k"] == 4 and r["select_us_per_step"] > 0 and r["audit_us_per_step"] > 0
        assert abs(r["audit_over_select"] - r["audit_us_per_step"] / r["select_us_per_step"]) < 1e-2


def test_gate_audit_report_prints_a_table_per_way_of_drawing_states(tmp_path):
    out = tool("gate_audit_report.py", "--maps", "pinball_simple", "--seeds", 1, "--envs", 256, "--warm", 40, "--after", 8,
               "--steps-per-option", 16, "--min-examples", 64, "--states", 128, "--record-envs", 16, "--out-dir", tmp_path).splitlines()
    assert out[0].startswith("# gate_audit_report map pinball_simple envs 256 ")
    head = re.match(r"seed 1: (\d+) options, enabled mask 0x[0-9a-f]+$", out[1])
    assert head and out[2].startswith("  greedy      success ")
    assert (tmp_path / "r20_gate_audit_pinball_simple.txt").read_text().splitlines() == out
    if int(head.group(1)) == 0:
        assert len(out) == 3                                  # no option: nothing to audit
        return
    ways = [i for i, ln in enumerate(out) if ln.startswith("  (a) ") or ln.startswith("  (b) ")]
    assert len(ways) == 2 and out[ways[0]].startswith("  (a) 128 free positions at rest: ")
    for i in ways:
        if "no offer state" in out[i]:
            continue
        n = int(re.search(r": (\d+) have a candidate$", out[i]).group(1))
        assert out[i + 1].split()[:3] == ["option", "n", "enter"]
        rows = []
        for ln in out[i + 2:]:
            rows.append(ln.split())
            if rows[-1][0] == "all":
                break
        assert rows[-1][0] == "all" and int(rows[-1][1]) == n == sum(int(r[1]) for r in rows[:-1])
        assert all(len(r) == 14 for r in rows)
