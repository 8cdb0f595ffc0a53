"""The measurement tools' one rig: the headline workload's set-up, the timing builds and their stamp layouts, the
synchronised timing loop, bench.py run as a child, and what the report and *_bench tools shared by copy. Importing it touches no
GPU: torch and the package are imported by the functions that need them."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402  (constants and chain_discs; bench.py imports torch only when it runs)

_TIMING = {"lite": ("SCG_LITE_LIB", "libscg_hip_lite.so"), "rstamps": ("SCG_RSTAMPS_LIB", "libscg_hip_rstamps.so")}
STAMP_SLOTS = 48      # csrc/scg_step_kernel.hpp STAMP_SLOTS: [0..31] four waves x eight boundaries, [32] [33] the block's start / end
#                       on the 100 MHz clock, [34..41] HW_REG_HW_ID of the 16 waves, [42] the block's pair groups
RED_NCOL = 102        # csrc/scg_reduce_kernel.hpp RED_NCOL = ceil(1620 / RED_C): the reduce grid is RED_NCOL x (row slots + n_vf)
RED_WAVES = 4         # csrc/scg_reduce_kernel.hpp RED_WAVES: waves of a slab workgroup
RED_STAMP_SLOTS = 24  # csrc/scg_reduce_kernel.hpp RED_STAMP_SLOTS


def headline_agent(envs=bench.ENVS_PER_GPU, options=bench.N_OPTIONS, *, seed=0, hp=None, enabled=None, w_std=1e-3, reset_seed=1000,
                   warm=0, library=None, trace=0):
    """bench.py's workload: the chain classifiers (options > 0), options 1..enabled on (default: all), W ~ N(0, w_std) from `seed`
    (None: W stays 0), random states from `reset_seed` (None: no reset), a trace ring of `trace` rows, `warm` step-batches."""
    import torch
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    kw = {} if library is None else {"library": library}
    ag = SkillChainingAgent(bench.MAP, envs, options, seed=seed, **(bench.HP if hp is None else hp), **kw)
    if options:
        ag.clf.copy_(torch.as_tensor(bench.chain_discs(ag.map, options)))
    for k in range(1, (options if enabled is None else enabled) + 1):
        ag.enable_option(k)
    if w_std is not None:
        ag.init_weights(std=w_std, seed=seed)
    if reset_seed is not None:
        ag.domain.reset_random(seed=reset_seed, v_max=1.0)
    if trace:
        ag.enable_tracing(trace)
    for _ in range(warm):
        ag.step_batch()
    torch.cuda.synchronize()
    return ag


def timing_library(kind):
    """Path of the `lite` / `rstamps` timing build (SCG_LITE_LIB / SCG_RSTAMPS_LIB name another one)."""
    var, name = _TIMING[kind]
    csrc = os.path.join(ROOT, "skill-chaining-with-graphs_amd", "csrc")
    path = os.environ.get(var) or os.path.join(csrc, name)
    if not os.path.exists(path):
        raise SystemExit(f"{path} is missing: make -C {os.path.relpath(csrc)} {kind}")
    return path


def _diag(ctx, name, restype):
    fn = getattr(ctx.lib, name, None)
    if fn is None:
        raise SystemExit(f"{name}: not exported by this library: not that timing build")
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int32], restype
    return fn


def read_step_stamps(ctx, reset):
    """[blocks, STAMP_SLOTS] uint64 of the light timing build: the cycle stamps summed since the last reset, the rest of the last launch."""
    import numpy as np
    out = np.zeros((-(-ctx.n_envs // ctx.block_envs), STAMP_SLOTS), np.uint64)
    _diag(ctx, "scg_diag_stamps", C.c_int)(ctx._ctx, out.ctypes.data_as(C.c_void_p), int(reset))
    return out


def read_reduce_stamps(ctx, reset, ncol=RED_NCOL):
    """[workgroups, RED_STAMP_SLOTS] uint64 of the reduce timing build's last launch, in grid order (y major: the row slots, then
    one line of `ncol` slab workgroups per value function; another `ncol` reads a library with another grid width)."""
    import numpy as np
    fn = _diag(ctx, "scg_diag_reduce_stamps", C.c_int)
    nwg, nrow = fn(ctx._ctx, None, 0), -(-ctx.n_envs // 256)
    assert nwg == ncol * (ctx.n_vf + -(-nrow // ncol)), "not a reduce timing build of this grid width, or RED_NCOL moved"
    out = np.zeros((nwg, RED_STAMP_SLOTS), np.uint64)
    fn(ctx._ctx, out.ctypes.data_as(C.c_void_p), int(reset))
    return out


def kernel_events(ctx, every=None):
    """The fused kernel's HIP events inside the library: `every` = n starts a pair round every n-th launch; without it, read what
    they measured -> (ms per launch, launches)."""
    if every is not None:
        return ctx._call("scg_profile_reset", every)
    ms, cnt = C.c_double(0.0), C.c_int64(0)
    ctx._call("scg_profile_read", C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value


def timed(fn, reps):
    """Seconds per call: synchronise, `reps` calls, synchronise."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def bench_line(tree, *flags, lib=None, timeout=600):
    """The result line of `python <tree>/bench.py <flags>`, run as a fresh child with SCG_LIB = lib (unset without one). Raises on a
    time-out, a non-zero exit or a last line that is no JSON: callers do not catch it, so a sweep ends at its first failed run."""
    env = dict(os.environ)
    env.pop("SCG_LIB", None)
    if lib:
        env["SCG_LIB"] = os.path.abspath(lib)
    tree = os.path.abspath(tree)
    cmd = [sys.executable, os.path.join(tree, "bench.py"), *map(str, flags)]
    try:
        p = subprocess.run(cmd, env=env, cwd=tree, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        raise RuntimeError(f"bench failed: {' '.join(cmd)} ran past {timeout} s: {str(e.stderr or '')[-400:]}") from None
    try:
        if p.returncode == 0:
            return json.loads(p.stdout.strip().splitlines()[-1])
    except (IndexError, ValueError):
        pass
    raise RuntimeError(f"bench failed: {' '.join(cmd)} (exit {p.returncode}): {p.stderr[-400:]}")


def bench_row(d):
    """(M env-steps/s, us per step-batch, the fused kernel's event time in us) of a bench line."""
    return d["value"] / 1e6, d["ms_per_step"] * 1e3, d["roofline"]["kernel_ms"] * 1e3


def discovery_hp(envs):
    """The hyper-parameters of the discovery reports (tools/chain_evidence.py's defaults)."""
    return dict(alpha=0.02, epsilon=0.05, gamma=0.99, max_episode_steps=2000, max_option_steps=200, r_option_success=0.0,
                update_count_floor=envs // 16, reoffer_period=4)


def fmt_eval(r, declines=True):
    """One line of an evaluate() result; the interrupts only where it acted with interruption."""
    line = (f"success {r['success_rate']:.4f} return {r['mean_return']:9.2f} length {r['mean_length']:7.1f} "
            f"share {[round(v, 3) for v in r['steps_share']]} entries {r['entries']}")
    if declines:
        line += f" declines {r['declines']}"
        if "interrupts" in r:
            line += f" interrupts {r['interrupts']}"
    return line


def delta_eval(x, y):
    return json.dumps({"success": round(y["success_rate"] - x["success_rate"], 4),
                       "return": round(y["mean_return"] - x["mean_return"], 2),
                       "length": round(y["mean_length"] - x["mean_length"], 1)})


def chain_classifiers(m, n_options):
    """Option k's initiation set: a disc round the goal of radius 0.18 + 0.17 (k - 1) (each holds the one before)."""
    return bench.chain_discs(m, n_options)


def state_on(ctx, m, n, seed=1):
    """An EnvState of n free positions (margin 2) and velocities in [-1, 1] from `seed`."""
    import numpy as np
    import torch
    from skill_chaining_with_graphs_amd.core import EnvState
    rng = np.random.default_rng(seed)
    st = EnvState(n, ctx.device, m)
    pos = m.sample_free(n, rng, margin=2.0)
    v = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    for t, a in zip((st.x, st.y, st.vx, st.vy), (pos[:, 0], pos[:, 1], v[:, 0], v[:, 1])):
        t.copy_(torch.as_tensor(np.ascontiguousarray(a, np.float32), device=ctx.device))
    return st
