"""SPEC §10 recorded rollouts and trials, host side (no GPU): the header and every build carry the two recording entry points and
SCG_ROLLOUT_BEGIN_AT, the ctypes scg_record has the C layout, a null ctx is refused, and Trajectory's segments / summary /
append work on hand-made rows."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scg_abi.h")
ENTRY_POINTS = ("scg_rollout_record", "scg_option_trials_record")


def test_header_declares_record_entry_points():
    src = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(rf"int\s+{name}\s*\(", src), name
    assert "} scg_record;" in src
    assert "#define SCG_ROLLOUT_BEGIN_AT 4u" in src
    assert "#define SCG_ABI_VERSION 5" in src


def test_every_build_exports_record_entry_points():
    from skill_chaining_with_graphs_amd import _lib
    assert _lib.ROLLOUT_BEGIN_AT == 4
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED_SYMBOLS
    for blk in _lib.BLOCK_ENVS_BUILDS:
        path = _lib.lib_path(blk)
        assert os.path.exists(path), f"{path} not built"
        lib = C.CDLL(path)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), (path, name)


def test_record_struct_layout_matches_c():
    from skill_chaining_with_graphs_amd._lib import Record
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler to build the layout probe")
    fields = [f for f, _ in Record._fields_]
    probe = "#include <stddef.h>\n#include <stdio.h>\n#include \"scg_abi.h\"\nint main(void) {\n"
    probe += '    printf("%zu\\n", sizeof(scg_record));\n'
    probe += "".join(f'    printf("%zu\\n", offsetof(scg_record, {f}));\n' for f in fields)
    probe += "    return 0;\n}\n"
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        c_path, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(c_path, "w") as fh:
            fh.write(probe)
        subprocess.run([cc, "-std=c99", "-I", os.path.dirname(HEADER), "-o", exe, c_path], check=True)
        out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(Record)
    assert out[1:] == [getattr(Record, f).offset for f in fields]


def test_null_ctx_is_invalid_without_a_device():
    from skill_chaining_with_graphs_amd import _lib
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    from skill_chaining_with_graphs_amd.trials import TrialResult
    lib = _lib.load(256)
    tr = Trajectory(4, 3)
    rec = tr.c_struct()
    p = C.c_void_p(tr.x.data_ptr())                         # any non-null address: nothing is launched
    st = EpisodeStats(2, 4).c_struct()
    args = [p] * 13 + [C.c_uint32(0b10), C.c_uint64(0), C.c_int32(2), C.c_uint32(_lib.ROLLOUT_BEGIN_AT), C.byref(st),
                       C.byref(rec), None]
    assert lib.scg_rollout_record(None, *args) == -1
    assert lib.scg_rollout_record(None, *args[:-2], None, None) == -1
    res = TrialResult(4)
    cs = res.c_struct()
    targs = [C.c_int32(4)] + [p] * 7 + [C.c_uint32(0b10), C.c_uint64(0), C.byref(cs), C.byref(rec), None]
    assert lib.scg_option_trials_record(None, *targs) == -1
    assert lib.scg_option_trials_record(None, *targs[:-2], None, None) == -1


def _launch(rows, n, cols):
    """A hand-made launch: cols maps a field to a list (per env) of row lists; len = each env's row count."""
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    out = {"len": torch.tensor([len(cols["vf"][r]) for r in range(n)], dtype=torch.int32)}
    for f in Trajectory.FIELDS:
        a = torch.full((rows, n), 77, dtype=Trajectory.DTYPES[f])        # rows at or beyond len hold junk
        for r in range(n):
            v = cols.get(f, [[0] * len(cols["vf"][r])] * n)[r]
            if v:
                a[: len(v), r] = torch.tensor(v, dtype=Trajectory.DTYPES[f])
        out[f] = a
    return out


def test_trajectory_segments_summary_append():
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    tr = Trajectory(2, 6)
    # env 0: begin row, two root steps (the second an offer of option 2 declined: option_id -2), option 1 for 3 steps ending in
    # SUCCESS, then in launch 2 option 2 for 2 steps, the last one the goal (EPISODE_END, done 1)
    # env 1: begin row straight into option 1 (begin row under the root), which times out after 2 steps; launch 2: nothing
    l1 = _launch(6, 2, {
        "vf":        [[0, 0, 0, 1, 1, 1], [0, 1, 1]],
        "option_id": [[0, 0, -2, 1, 1, 0], [1, 1, 0]],
        "term":      [[0, 0, 0, 0, 0, 1], [0, 0, 4]],
        "done":      [[2, 0, 0, 0, 0, 0], [2, 0, 0]],
        "action":    [[255, 1, 2, 3, 0, 4], [255, 2, 2]],
        "reward":    [[0.0, -1.0, -1.0, -1.0, -1.0, -1.0], [0.0, -1.0, -1.0]],
    })
    l2 = _launch(6, 2, {
        "vf":        [[2, 2], []],
        "option_id": [[2, 0], []],
        "term":      [[0, 2], []],
        "done":      [[0, 1], []],
        "action":    [[1, 1], []],
        "reward":    [[-1.0, 10000.0], []],
    })
    tr.append(l1).append(l2)
    e0 = tr.per_env(0)
    assert tr.length(0) == 8 and tr.length(1) == 3
    assert list(e0["vf"]) == [0, 0, 0, 1, 1, 1, 2, 2]
    assert list(e0["option_id"]) == [0, 0, -2, 1, 1, 0, 2, 0]
    assert float(np.cumsum(e0["reward"].astype(np.float64))[-1]) == 10000.0 - 6.0
    assert tr.segments(0) == [
        {"vf": 0, "start": 0, "end": 2, "steps": 3, "term": 0, "done": 0},
        {"vf": 1, "start": 3, "end": 5, "steps": 3, "term": 1, "done": 0},
        {"vf": 2, "start": 6, "end": 7, "steps": 2, "term": 2, "done": 1},
    ]
    assert tr.segments(1) == [
        {"vf": 0, "start": 0, "end": 0, "steps": 1, "term": 0, "done": 0},
        {"vf": 1, "start": 1, "end": 2, "steps": 2, "term": 4, "done": 0},
    ]
    assert tr.describe(0) == "root×3 → 1×3 SUCCESS → 2×2 EPISODE_END(goal)"
    assert tr.describe(1) == "root×1 → 1×2 TIMEOUT"
    s = tr.summary()
    assert s["segments"] == [2, 2, 1]
    assert s["mean_steps"][0] == (2 + 0) / 2                 # begin rows are not steps
    assert s["mean_steps"][1] == (3 + 2) / 2 and s["mean_steps"][2] == 2.0
    assert s["term_hist"][1] == [0, 1, 0, 0, 1] and s["term_hist"][2] == [0, 0, 1, 0, 0] and s["term_hist"][0] == [2, 0, 0, 0, 0]
    assert s["declined_rows"] == 1 and s["episodes"] == 1 and s["goals"] == 1 and s["goal_rate"] == 1.0


def test_trajectory_episode_boundaries_and_empty():
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    tr = Trajectory(1, 5, first=3)
    # without ONE_EPISODE: a root episode that times out (done 2), then the next one under the root
    tr.append(_launch(5, 1, {"vf": [[0, 0, 0, 0, 0]], "done": [[0, 0, 2, 0, 0]], "action": [[0, 1, 2, 3, 4]]}))
    assert [(g["start"], g["end"], g["done"]) for g in tr.segments(0)] == [(0, 2, 2), (3, 4, 0)]
    assert tr.describe(0) == "root×3 EPISODE_END → root×2"
    s = tr.summary()
    assert s["episodes"] == 1 and s["goals"] == 0 and s["goal_rate"] == 0.0
    out = tr.to_numpy()
    assert list(out["offsets"]) == [0, 5] and int(out["first"]) == 3
    e = Trajectory(2, 4).summary()
    assert e["episodes"] == 0 and math.isnan(e["goal_rate"]) and e["segments"] == [0]
    w = Trajectory(1, 5, n_vf=4)                               # per-VF lists sized by the context, not by what was seen
    w.append(_launch(5, 1, {"vf": [[0, 1, 1]], "term": [[0, 0, 3]], "action": [[255, 0, 0]], "done": [[2, 0, 0]]}))
    ws = w.summary()
    assert ws["segments"] == [1, 1, 0, 0] and len(ws["mean_steps"]) == 4 and len(ws["term_hist"]) == 4
    assert ws["term_hist"][1] == [0, 0, 0, 1, 0] and math.isnan(ws["mean_steps"][3])
    with pytest.raises(ValueError):
        Trajectory(0, 4)
