"""tools/: every script imports without effect and without a device, answers --help, and gets its bench lines through rig.bench_line,
which raises on a failed child so that a sweep ends at its first failed run. No GPU."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import ab_trees  # noqa: E402
import rig  # noqa: E402

SCRIPTS = sorted(glob.glob(os.path.join(TOOLS, "*.py")))
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
LINE = {"value": 8.0e8, "ms_per_step": 0.08, "roofline": {"kernel_ms": 0.07}}

IMPORT_ALL = """
import importlib.util, io, json, sys, contextlib
sys.path.insert(0, sys.argv[1])
buf, argv = io.StringIO(), list(sys.argv)
with contextlib.redirect_stdout(buf):
    for path in sys.argv[2:]:
        spec = importlib.util.spec_from_file_location("tool_" + str(len(sys.modules)), path)
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
print(json.dumps({"stdout": buf.getvalue(), "torch": "torch" in sys.modules, "argv": sys.argv == argv}))
"""


def test_there_are_tools():
    assert len(SCRIPTS) >= 30 and os.path.join(TOOLS, "rig.py") in SCRIPTS


def test_every_tool_imports_without_effect_and_without_a_device():
    p = subprocess.run([sys.executable, "-c", IMPORT_ALL, TOOLS, *SCRIPTS], env=NO_GPU, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got == {"stdout": "", "torch": False, "argv": True}       # nothing printed, torch not even imported, argv left alone


@pytest.mark.parametrize("path", [s for s in SCRIPTS if "argparse" in open(s).read()], ids=os.path.basename)
def test_help(path):
    p = subprocess.run([sys.executable, path, "--help"], env=NO_GPU, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("usage:"), p.stderr[-2000:]


def stub_tree(tmp_path, name, body):
    """A source tree whose bench.py is `body` behind a line that logs the start."""
    tree = tmp_path / name
    tree.mkdir()
    log = tmp_path / "starts.txt"
    (tree / "bench.py").write_text(f"import json, sys, time\nopen({str(log)!r}, 'a').write({name!r} + '\\n')\n{body}\n")
    return str(tree), log


def test_bench_line_parses_the_last_line(tmp_path):
    tree, _ = stub_tree(tmp_path, "ok", f"print('noise'); print(json.dumps(dict({LINE!r}, argv=sys.argv[1:])))")
    d = rig.bench_line(tree, "--steps", 5, "--no-extras")
    assert d["argv"] == ["--steps", "5", "--no-extras"] and rig.bench_row(d) == (800.0, 80.0, 70.0)


def test_bench_line_sets_or_removes_SCG_LIB(tmp_path, monkeypatch):
    tree, _ = stub_tree(tmp_path, "env", "import os; print(json.dumps({'lib': os.environ.get('SCG_LIB')}))")
    monkeypatch.setenv("SCG_LIB", "/somewhere/else.so")
    assert rig.bench_line(tree)["lib"] is None
    assert rig.bench_line(tree, lib=str(tmp_path / "x.so"))["lib"] == str(tmp_path / "x.so")


@pytest.mark.parametrize("body, timeout, says", [
    ("print(json.dumps({'value': 1})); sys.stderr.write('the reason'); sys.exit(1)", 60, "the reason"),
    ("time.sleep(60)", 0.5, "ran past 0.5 s"),
    ("print('no result line here')", 60, "exit 0"),
    ("pass", 60, "exit 0"),
], ids=["exit-1", "time-limit", "no-json", "no-output"])
def test_bench_line_raises_on_a_failed_child(tmp_path, body, timeout, says):
    tree, _ = stub_tree(tmp_path, "bad", body)
    with pytest.raises(RuntimeError, match="bench failed") as e:
        rig.bench_line(tree, timeout=timeout)
    assert says in str(e.value)


def test_ab_trees_prints_every_run_and_the_medians(tmp_path, capsys):
    a, log = stub_tree(tmp_path, "a", f"print(json.dumps({LINE!r}))")
    b, _ = stub_tree(tmp_path, "b", f"print(json.dumps({LINE!r}))")
    ab_trees.main(["--rounds", "2", "--steps", "3", f"a={a}", f"b={b}"])
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 6 and log.read_text().split() == ["a", "b", "a", "b"]          # interleaved
    assert out[0] == f"{'a':24s}   800.0 M/s    80.00 us/step  td  70.00 us"
    assert out[4:] == [f"median {n:24s}   800.0 M/s    80.00 us/step  td  70.00 us" for n in "ab"]


def test_ab_bench_is_ab_trees_with_its_own_median_line(tmp_path, capsys, monkeypatch):
    import ab_bench
    tree, _ = stub_tree(tmp_path, "t", f"import os; print(json.dumps(dict({LINE!r}, value=1e6 * len(os.environ['SCG_LIB']))))")
    monkeypatch.setattr(rig, "ROOT", tree)
    lib = str(tmp_path / "lib1.so")
    ab_bench.main(["--rounds", "1", lib])
    out = capsys.readouterr().out.splitlines()
    assert out == [f"{'lib1.so':28s} {len(lib):7.1f} M/s    80.00 us/step  td  70.00 us", f"median {'lib1.so':28s} {len(lib):7.1f} M/s  td  70.00 us"]


def test_a_failed_run_ends_ab_trees_and_starts_no_later_arm(tmp_path):
    a, log = stub_tree(tmp_path, "a", f"print(json.dumps({LINE!r}))")
    b, _ = stub_tree(tmp_path, "b", "sys.stderr.write('the card fell over'); sys.exit(134)")
    c, _ = stub_tree(tmp_path, "c", f"print(json.dumps({LINE!r}))")
    p = subprocess.run([sys.executable, os.path.join(TOOLS, "ab_trees.py"), "--rounds", "2", f"a={a}", f"b={b}", f"c={c}"],
                       env=NO_GPU, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "bench failed" in p.stderr and "the card fell over" in p.stderr and "exit 134" in p.stderr
    assert log.read_text().split() == ["a", "b"]                    # neither c nor a second round
    assert len(p.stdout.splitlines()) == 1 and "median" not in p.stdout
