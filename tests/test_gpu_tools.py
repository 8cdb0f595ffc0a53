"""The measurement tools still run against the package: each case is one tool as a fresh child process under its own
time limit. A child that ends by a signal or at its time limit may have left the card in a bad state: the module then starts no
further child."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 120                      # seconds: process start and the torch import; the GPU work of every case is well under a second
_stop = []                       # why no further child is started


def tool(name, *args):
    """stdout of `python tools/<name> <args>`; the geometry is the context's own choice (the suite pins SCG_BLOCK_ENVS)."""
    if _stop:
        pytest.skip(_stop[0])
    env = {k: v for k, v in os.environ.items() if k != "SCG_BLOCK_ENVS"}
    cmd = [sys.executable, os.path.join(ROOT, "tools", name), *map(str, args)]
    try:
        p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        _stop.append(f"{name} ran into its {LIMIT} s limit: no further tool is started")
        pytest.fail(_stop[0])
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _stop.append(f"{name} ended by a signal (status {p.returncode}): no further tool is started")
        pytest.fail(_stop[0] + "\n" + p.stderr[-2000:])
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("args", [("--options", 0), ("--options", 2, "--trace")], ids=["root-only", "options-traced"])
def test_run_checksum_repeats_across_processes(args):
    """320 envs: five 64-env blocks under the automatic geometry; the two branches of rig.headline_agent's set-up."""
    a, b = (tool("run_checksum.py", "--envs", 320, "--steps", 20, *args).strip() for _ in range(2))
    assert a == b and "\n" not in a
    assert a.startswith(f"envs 320 options {args[1]} steps 20 trace {len(args) == 3} poison False: sha256 ") and a.endswith(" status 0")


def test_pass_census_prints_its_table():
    out = tool("pass_census.py").splitlines()
    assert out[0].startswith("blocks 256 chunk c ") and "update passes/block" in out[0] and "hist of eval-only per block" in out[0]
    assert out[1].startswith("option counts [") and sum(json.loads(out[1][len("option counts "):])) == 65536
    assert out[-1].startswith("items per evaluation-only pass: mean ")


def test_action_skew_prints_its_table():
    out = tool("action_skew.py").splitlines()
    assert len(out) == 4 and [ln.split(" action shares ")[0] for ln in out[:3]] == ["t 300", "t 1000", "t 3000"]
    for ln in out[:3]:
        assert abs(sum(json.loads(ln.split(" action shares ")[1])) - 1.0) < 0.01
    assert out[3].startswith("groups per action per block: mean [")


@pytest.mark.parametrize("name, args, keys", [
    ("rollout_bench.py", ("--sizes", 1, "--k", 1, "--rounds", 1), ("rollout_us_per_step", "step_loop_us_per_step", "speedup")),
    ("trial_bench.py", ("--n", 1, "--rounds", 1, "--max-option-steps", 1), ("trials_ms", "step_loop_ms", "longest_trial_steps")),
    ("step_interrupt_bench.py", ("--sizes", 1, "--k", 1, "--rounds", 1), ("plain_us_per_step", "interrupt_us_per_step", "option_running_share")),
], ids=["rollout", "trial", "step-interrupt"])
def test_bench_tools_run_one_round_at_their_smallest_size(name, args, keys):
    out = tool(name, *args).strip().splitlines()
    assert len(out) == 1
    d = json.loads(out[0])
    assert all(k in d for k in keys) and d.get("n_envs", d.get("n")) == 1
