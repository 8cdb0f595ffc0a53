"""SPEC §9 option trials, host side (no GPU): the header and every build carry scg_option_trials, the ctypes struct has the C
layout, argument errors are refused without a device, and TrialResult.summary() aggregates hand-made outputs."""
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


def test_header_declares_trials():
    src = open(HEADER).read()
    assert re.search(r"int\s+scg_option_trials\s*\(", src)
    assert "} scg_trial_out;" in src
    for macro in ("SCG_TRIAL_SUCCESS 1u", "SCG_TRIAL_EPISODE_END 2u", "SCG_TRIAL_LEFT_INITIATION 3u", "SCG_TRIAL_TIMEOUT 4u",
                  "SCG_TRIAL_MAX_STEPS SCG_ROLLOUT_MAX_STEPS"):
        assert f"#define {macro}" in src, macro
    assert "#define SCG_ABI_VERSION 5" in src


def test_trial_constants_match_header():
    from skill_chaining_with_graphs_amd import _lib
    assert (_lib.TRIAL_SUCCESS, _lib.TRIAL_EPISODE_END, _lib.TRIAL_LEFT_INITIATION, _lib.TRIAL_TIMEOUT) == (1, 2, 3, 4)
    assert _lib.TRIAL_MAX_STEPS == _lib.ROLLOUT_MAX_STEPS == 1024


def test_every_build_exports_trials():
    from skill_chaining_with_graphs_amd import _lib
    assert "scg_option_trials" in _lib.EXPORTED_SYMBOLS
    for blk in _lib.BLOCK_ENVS_BUILDS:
        path = _lib.lib_path(blk)
        assert os.path.exists(path), f"{path} not built"
        assert hasattr(C.CDLL(path), "scg_option_trials"), path


def test_trial_out_layout_matches_c():
    from skill_chaining_with_graphs_amd._lib import TrialOut
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler to build the layout probe")
    fields = [f for f, _ in TrialOut._fields_]
    probe = "#include <stddef.h>\n#include <stdio.h>\n#include \"scg_abi.h\"\nint main(void) {\n"
    probe += '    printf("%zu\\n", sizeof(scg_trial_out));\n'
    probe += "".join(f'    printf("%zu\\n", offsetof(scg_trial_out, {f}));\n' for f in fields)
    probe += "    return 0;\n}\n"
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        c_path, exe = os.path.join(d, "probe.c"), os.path.join(d, "probe")
        with open(c_path, "w") as fh:
            fh.write(probe)
        subprocess.run([cc, "-std=c99", "-I", os.path.dirname(HEADER), "-o", exe, c_path], check=True)
        out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(TrialOut)
    assert out[1:] == [getattr(TrialOut, f).offset for f in fields]


def test_null_ctx_is_invalid_without_a_device():
    from skill_chaining_with_graphs_amd import _lib
    from skill_chaining_with_graphs_amd.trials import TrialResult
    lib = _lib.load(256)
    res = TrialResult(4)
    cs = res.c_struct()
    p = C.c_void_p(res.ret.data_ptr())                      # any non-null address: nothing is launched
    args = [C.c_int32(4)] + [p] * 7 + [C.c_uint32(0b10), C.c_uint64(0), C.byref(cs), None]
    assert lib.scg_option_trials(None, *args) == -1
    assert lib.scg_option_trials(None, C.c_int32(0), *args[1:]) == -1
    assert lib.scg_option_trials(None, *args[:-2], None, None) == -1


def test_summary_on_cpu_tensors():
    from skill_chaining_with_graphs_amd.trials import TrialResult
    r = TrialResult(7, option=[1, 2, 1, 0, 1, 2, 9])
    r.outcome.copy_(torch.tensor([1, 3, 4, 0, 1, 2, 0], dtype=torch.uint8))
    r.steps.copy_(torch.tensor([10, 1, 25, 0, 30, 7, 0], dtype=torch.int32))
    r.disc_ret.copy_(torch.tensor([9000.0, -5.0, -100.5, 0.0, 8000.25, -30.0, 0.0]))
    r.v0.copy_(torch.tensor([1.5, -2.0, 0.25, 0.0, 0.5, 3.0, 0.0]))
    s = r.summary()
    assert sorted(s) == [1, 2]                               # options with a run trial only
    a = s[1]
    assert a["trials"] == 3
    assert (a["success"], a["episode_end"], a["left_initiation"], a["timeout"]) == (2 / 3, 0.0, 0.0, 1 / 3)
    assert a["mean_steps_success"] == 20.0
    assert a["mean_disc_ret"] == ((9000.0 + -100.5) + 8000.25) / 3
    assert a["mean_v0"] == ((1.5 + 0.25) + 0.5) / 3
    b = s[2]
    assert b["trials"] == 2 and b["left_initiation"] == 0.5 and b["episode_end"] == 0.5 and b["success"] == 0.0
    assert math.isnan(b["mean_steps_success"])
    assert b["mean_disc_ret"] == -17.5 and b["mean_v0"] == 0.5
    assert TrialResult(3).summary() == {}
