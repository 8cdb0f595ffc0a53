"""SPEC §8 acting rollouts, host side (no GPU): the header and every build carry scg_rollout, the ctypes struct has the C
layout, and EpisodeStats.summary() aggregates hand-made counters."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scg_abi.h")


def test_header_declares_rollout():
    src = open(HEADER).read()
    assert re.search(r"int\s+scg_rollout\s*\(", src)
    assert "} scg_rollout_stats;" in src
    for macro in ("SCG_ROLLOUT_BEGIN 1u", "SCG_ROLLOUT_ONE_EPISODE 2u", "SCG_ROLLOUT_MAX_STEPS 1024"):
        assert f"#define {macro}" in src, macro
    assert "#define SCG_ABI_VERSION 5" in src


def test_every_build_exports_rollout():
    from skill_chaining_with_graphs_amd import _lib
    assert "scg_rollout" in _lib.EXPORTED_SYMBOLS
    for blk in _lib.BLOCK_ENVS_BUILDS:
        path = _lib.lib_path(blk)
        assert os.path.exists(path), f"{path} not built"
        assert hasattr(C.CDLL(path), "scg_rollout"), path


def test_stats_struct_layout_matches_c():
    from skill_chaining_with_graphs_amd._lib import RolloutStats
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler to build the layout probe")
    fields = [f for f, _ in RolloutStats._fields_]
    probe = "#include <stddef.h>\n#include <stdio.h>\n#include \"scg_abi.h\"\nint main(void) {\n"
    probe += '    printf("%zu\\n", sizeof(scg_rollout_stats));\n'
    probe += "".join(f'    printf("%zu\\n", offsetof(scg_rollout_stats, {f}));\n' for f in fields)
    probe += "    return 0;\n}\n"
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        c_path, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(c_path, "w") as fh:
            fh.write(probe)
        subprocess.run([cc, "-std=c99", "-I", os.path.dirname(HEADER), "-o", exe, c_path], check=True)
        out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(RolloutStats)
    assert out[1:] == [getattr(RolloutStats, f).offset for f in fields]


def test_summary_on_cpu_tensors():
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
    s = EpisodeStats(3, 4)                                  # 3 VFs, 4 envs, CPU
    s.episodes.copy_(torch.tensor([1, 1, 0, 2], dtype=torch.int32))
    s.goals.copy_(torch.tensor([1, 0, 0, 1], dtype=torch.int32))
    s.len_sum.copy_(torch.tensor([10, 60, 0, 30], dtype=torch.int32))
    s.ret_sum.copy_(torch.tensor([9990.0, -300.0, 0.0, 9000.5], dtype=torch.float64))
    s.vf_steps.copy_(torch.tensor([[5, 60, 7, 20], [5, 0, 0, 10], [0, 0, 3, 0]], dtype=torch.int32))
    s.entries.copy_(torch.tensor([[0, 0, 0, 0], [1, 0, 0, 2], [0, 0, 1, 0]], dtype=torch.int32))
    s.declines.copy_(torch.tensor([[0, 0, 0, 0], [0, 3, 0, 1], [0, 0, 0, 0]], dtype=torch.int32))
    s.successes.copy_(torch.tensor([[0, 0, 0, 0], [1, 0, 0, 1], [0, 0, 0, 0]], dtype=torch.int32))
    r = s.summary()
    assert r["episodes"] == 4
    assert r["success_rate"] == 0.5
    assert r["mean_return"] == ((9990.0 + -300.0) + 0.0 + 9000.5) / 4
    assert r["mean_length"] == 100 / 4
    assert r["steps_share"] == [92 / 110, 15 / 110, 3 / 110]
    assert r["entries"] == [0, 3, 1] and r["declines"] == [0, 4, 0] and r["successes"] == [0, 2, 0]
    e = EpisodeStats(2, 3).summary()                        # nothing recorded yet
    assert e["episodes"] == 0 and math.isnan(e["success_rate"]) and math.isnan(e["mean_length"])
    assert s.zero_().summary()["episodes"] == 0


def test_rollout_constants_match_header():
    from skill_chaining_with_graphs_amd import _lib
    src = open(HEADER).read()
    assert _lib.ROLLOUT_BEGIN == 1 and _lib.ROLLOUT_ONE_EPISODE == 2
    assert f"#define SCG_ROLLOUT_MAX_STEPS {_lib.ROLLOUT_MAX_STEPS}" in src
