"""SPEC §11 interrupting rollouts on the GPU: one scg_rollout_interrupt launch equals tests/acting_emulator.py's emulator on
already-verified entry points (gpu_util.GpuBackend: scg_rollout_record one step at a time, scg_q_values for V_0,
scg_classifier_predict for the candidate; V_o read from the option's qcache), and the same emulator on the oracle; every launch
geometry and block build agree; with every W_k == W_0 nothing is interrupted; the record marks interrupted rows INTERRUPTED; the
agent's evaluate(interrupt=True) / record_episodes(interrupt=True) leave training alone; and the C-ABI's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import skill_chaining_with_graphs_amd as scg
from acting_emulator import oracle_emulator
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
from skill_chaining_with_graphs_amd.trajectory import Trajectory
from gpu_util import (as_bytes, assert_same_bits, clone_state, crossing_agent, dev, gpu_emulator, make_context, make_pair,
                      spy_calls, state_to_device)
from util import HP, chain_classifiers, crossing_weights, oracle_state, random_env_state, wide_chain

pytestmark = pytest.mark.gpu

STATS = EpisodeStats.FIELDS


def _setup(name, n, n_opt, parents=None, gest=0, seed=3, block=None, **hp):
    m = scg.load_map(name)
    ctx = make_context(m, n, n_opt, block, parents, gest, seed, **hp)
    clf = dev(wide_chain(m, n_opt)).view(-1)
    W = dev(crossing_weights(n_opt + 1, seed)).view(-1)
    return ctx, m, W, clf


def _state(ctx, m, n, n_opt, seed):
    return state_to_device(random_env_state(m, n, n_opt, seed, id_lo=-n_opt, id_hi=n_opt, opt_steps_hi=10,
                                            max_episode_steps=ctx.cfg.max_episode_steps), ctx)


CASES = [
    # map, n, options, enabled, gestating, parents, epsilon, steps per launch
    ("pinball_simple", 4096, 3, 0b1110, 0, None, 0.0, (24,)),
    ("pinball_simple", 4096, 3, 0b1010, 0b0100, [0, 0, 1, 1], 0.1, (7, 9, 16)),
    ("pinball_maze", 4096, 4, 0b11110, 0, [0, 0, 1, 1, 2], 0.1, (32,)),
    ("pinball_maze", 4096, 2, 0b110, 0, None, 0.0, (5, 11)),
]


def _run_case(name, n, n_opt, mask, gest, parents, eps, splits, mode, seed=3, t0=500, **hp):
    if mode == "begin" and eps == 0.0:
        eps = 0.05            # greedy episodes from the map's few start states would all be one and the same episode
    ctx, m, W, clf = _setup(name, n, n_opt, parents, gest, seed=seed, epsilon=eps, reoffer_period=4, max_episode_steps=40,
                            max_option_steps=20, **hp)
    st = _state(ctx, m, n, n_opt, seed=n + n_opt)
    twin = clone_state(st)
    n_vf = n_opt + 1
    s_ref, s_int = EpisodeStats(n_vf, n, ctx.device), EpisodeStats(n_vf, n, ctx.device)
    begin, at, one = mode == "begin", mode == "begin_at", mode in ("begin", "begin_at", "one_episode")
    emu = gpu_emulator(ctx, st, W, clf, mask, gest, stats=s_ref, one_episode=one, interrupt=True, v_option="qcache")
    t = t0
    for i, K in enumerate(splits):
        first = i == 0
        emu.run(t, K, begin=begin and first, begin_at=at and first)
        ctx.rollout(twin, W, clf, mask, t, K, s_int, begin=begin and first, begin_at=at and first, one_episode=one,
                    interrupt=True)
        t += K + (1 if (begin or at) and first else 0)
    torch.cuda.synchronize()
    assert_same_bits(twin, st, EnvState.FIELDS, f"{name} {mode}")
    assert_same_bits(s_int, s_ref, STATS, f"{name} {mode} stats")
    assert np.array_equal(s_int.interrupts.cpu().numpy(), emu.interrupts), f"{name} {mode}: interrupts differ"
    assert emu.interrupted > 0 and emu.kept > emu.interrupted, \
        f"the case never interrupts, or never keeps an option (kept {emu.kept}, interrupted {emu.interrupted})"
    assert int(s_ref.entries.sum()) > 0, "the case never enters an option"
    return ctx, emu


@pytest.mark.parametrize("mode", ["plain", "begin", "one_episode", "begin_at"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-o{c[2]}-e{c[6]}")
def test_interrupt_equals_emulator(case, mode):
    _run_case(*case, mode)


def test_interrupt_equals_emulator_large():
    _run_case("pinball_simple", 65536, 3, 0b1110, 0, None, 0.1, (6,), "begin")


def test_interrupt_equals_oracle_emulator():
    """The emulator on the oracle (acting step, q_values, classifier_predict) against one launch: the kernel tied to the oracle."""
    n, n_opt, mask = 1000, 3, 0b1110
    ctx, orc, m = make_pair("pinball_simple", n, n_options=n_opt, seed=9, enabled_mask=mask, reoffer_period=4)
    clf = chain_classifiers(m, n_opt)
    W = crossing_weights(n_opt + 1, 4)
    n_vf = n_opt + 1
    st_o = oracle_state(random_env_state(m, n, n_opt, 5, id_lo=-n_opt, id_hi=n_opt, opt_steps_hi=10,
                                         max_episode_steps=HP["max_episode_steps"]), m)
    st_d = state_to_device(st_o, ctx)
    K, t0 = 20, 77
    emu = oracle_emulator(orc, st_o, W, clf, mask, interrupt=True, v_option="qcache")     # W not applied: acting only
    emu.run(t0, K)
    intr = torch.zeros((n_vf, n), dtype=torch.int32, device=ctx.device)
    ctx.rollout(st_d, dev(W).view(-1), dev(clf).view(-1), mask, t0, K, interrupt=True, interrupts=intr)
    torch.cuda.synchronize()
    assert emu.interrupted > 0
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(st_d, f)), as_bytes(st_o[f])), f"oracle emulator: {f} differs"
    assert np.array_equal(intr.cpu().numpy(), emu.interrupts)


def _interrupt_launch(name, n, n_opt, mask, block=None, W=None, seed=3, rec=False):
    """Two interrupting launches (BEGIN, then a continuation) with tree parents; returns the state, the stats and the record."""
    ctx, m, W0, clf = _setup(name, n, n_opt, [0, 0, 1, 1], seed=seed, block=block, epsilon=0.1, reoffer_period=4)
    W = W0 if W is None else W
    st = _state(ctx, m, n, n_opt, seed=11)
    stats = EpisodeStats(n_opt + 1, n, ctx.device)
    tr = Trajectory(n, 30, 0, ctx.device) if rec else None
    ctx.rollout(st, W, clf, mask, 300, 29, stats, begin=True, interrupt=True, record=tr)
    ctx.rollout(st, W, clf, mask, 330, 17, stats, interrupt=True)
    torch.cuda.synchronize()
    return st, stats, tr


def test_every_launch_geometry_and_block_build(monkeypatch):
    n, n_opt, mask = 3000, 3, 0b1110
    ref_st, ref_stats, _ = _interrupt_launch("pinball_simple", n, n_opt, mask)
    assert int(ref_stats.interrupts.sum()) > 0
    for epw in (2, 4, 8, 16, 32):
        monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
        st, stats, _ = _interrupt_launch("pinball_simple", n, n_opt, mask)
        assert_same_bits(st, ref_st, EnvState.FIELDS, f"epw {epw}")
        assert_same_bits(stats, ref_stats, STATS + ("interrupts",), f"epw {epw} stats")
    monkeypatch.delenv("SCG_ROLLOUT_EPW")
    for block in (64, 128, 256):
        st, stats, _ = _interrupt_launch("pinball_simple", n, n_opt, mask, block=block)
        assert_same_bits(st, ref_st, EnvState.FIELDS, f"block {block}")
        assert_same_bits(stats, ref_stats, STATS + ("interrupts",), f"block {block} stats")


def test_ties_never_interrupt():
    """With every W_k == W_0 the values tie everywhere: an interrupting rollout is scg_rollout, bit for bit."""
    n, n_opt, mask = 4096, 3, 0b1110
    ctx, m, W, clf = _setup("pinball_simple", n, n_opt, epsilon=0.1)
    Wt = W.view(n_opt + 1, -1)[0].repeat(n_opt + 1).contiguous()
    st = _state(ctx, m, n, n_opt, seed=21)
    twin, third = clone_state(st), clone_state(st)
    a, b = EpisodeStats(n_opt + 1, n, ctx.device), EpisodeStats(n_opt + 1, n, ctx.device)
    ctx.rollout(st, Wt, clf, mask, 40, 48, a, begin=True)
    ctx.rollout(twin, Wt, clf, mask, 40, 48, b, begin=True, interrupt=True)
    emu = gpu_emulator(ctx, third, Wt, clf, mask, interrupt=True, v_option="qcache")    # the host rule holds a tie as well
    emu.run(40, 48, begin=True)
    torch.cuda.synchronize()
    assert_same_bits(twin, st, EnvState.FIELDS, "ties")
    assert_same_bits(third, st, EnvState.FIELDS, "ties, emulated")
    assert emu.interrupted == 0 and emu.kept > 0
    assert_same_bits(b, a, STATS, "ties stats")
    assert int(b.interrupts.sum()) == 0 and b.summary()["interrupts"] == [0] * (n_opt + 1)
    assert int(a.vf_steps[1:].sum()) > 0, "no option ran: the tie check is vacuous"


@pytest.mark.parametrize("mode", ["begin", "one_episode"])
def test_record_rows_equal_emulator(mode):
    n, n_opt, mask = 4096, 3, 0b1110
    ctx, m, W, clf = _setup("pinball_simple", n, n_opt, epsilon=0.1, reoffer_period=4, max_episode_steps=30)
    st = _state(ctx, m, n, n_opt, seed=31)
    twin, plain = clone_state(st), clone_state(st)
    s_ref, s_int, s_plain = (EpisodeStats(n_opt + 1, n, ctx.device) for _ in range(3))
    one = mode == "one_episode"
    K = 40
    emu = gpu_emulator(ctx, st, W, clf, mask, stats=s_ref, one_episode=one, interrupt=True, v_option="qcache")
    emu.run(9, K, begin=True)
    tr = Trajectory(n, K + 1, 0, ctx.device)
    ctx.rollout(twin, W, clf, mask, 9, K, s_int, begin=True, one_episode=one, interrupt=True, record=tr)
    ctx.rollout(plain, W, clf, mask, 9, K, s_plain, begin=True, one_episode=one, interrupt=True)
    torch.cuda.synchronize()
    assert_same_bits(twin, st, EnvState.FIELDS, "recorded")
    assert_same_bits(plain, twin, EnvState.FIELDS, "recording changed the outputs")
    assert_same_bits(s_plain, s_int, STATS + ("interrupts",), "recording changed the counters")
    assert np.array_equal(s_int.interrupts.cpu().numpy(), emu.interrupts)
    rows, ln = emu.record()
    got_len = tr.len.cpu().numpy()
    assert np.array_equal(got_len, ln), "len"
    if one:
        assert (got_len < K + 1).any(), "no episode ended: ONE_EPISODE's prefix is not exercised"
    valid = np.arange(K + 1)[:, None] < got_len[None, :]
    for f in tr.fields:
        g = getattr(tr, f).cpu().numpy()
        assert np.array_equal(as_bytes(g[valid]), as_bytes(rows[f][valid])), f"record field {f}"
    term = tr.term.cpu().numpy()
    cut = (term == _lib.ROLLOUT_TERM_INTERRUPTED) & valid
    assert int(cut.sum()) == int(s_int.interrupts.sum()) > 0
    assert (tr.vf.cpu().numpy()[cut] >= 1).all() and not (tr.done.cpu().numpy()[cut] != 0).any()
    tr.append()
    e = int(np.nonzero(cut.any(axis=0))[0][0])
    assert "INTERRUPTED" in tr.describe(e)
    assert sum(tr.summary()["interrupted"]) == int(cut.sum())


def test_c_abi_refusals():
    n, n_opt = 64, 2
    ctx, m, W, clf = _setup("pinball_simple", n, n_opt)
    st = _state(ctx, m, n, n_opt, seed=1)
    lib = ctx.lib
    arr = [C.c_void_p(getattr(st, f).data_ptr()) for f in EnvState.FIELDS] + [C.c_void_p(W.data_ptr()), C.c_void_p(clf.data_ptr())]
    stats = EpisodeStats(n_opt + 1, n, ctx.device)
    cs = stats.c_struct()
    nofin = EpisodeStats(n_opt + 1, n, ctx.device).c_struct()
    nofin.finished = None
    tr = Trajectory(n, 2, 0, ctx.device)
    good, noln, short = tr.c_struct(), tr.c_struct(), tr.c_struct()
    noln.len = None
    short.rows = 1
    intr = C.c_void_p(stats.interrupts.data_ptr())

    def call(fn, flags, n_steps, s=cs, rec=None, extra=()):
        args = arr + [C.c_uint32(0b110), C.c_uint64(0), C.c_int32(n_steps), C.c_uint32(flags), C.byref(s), *extra,
                      None if rec is None else C.byref(rec), None]
        rc = getattr(lib, fn)(ctx._ctx, *args)
        return rc, lib.scg_last_error(ctx._ctx).decode()

    B, O, A = _lib.ROLLOUT_BEGIN, _lib.ROLLOUT_ONE_EPISODE, _lib.ROLLOUT_BEGIN_AT
    for flags, n_steps, s, rec in ((0x80, 1, cs, None), (B | A, 1, cs, None), (0, _lib.ROLLOUT_MAX_STEPS + 1, cs, None),
                                   (0, -1, cs, None), (0, 0, cs, None), (O, 1, nofin, None), (0, 1, cs, noln),
                                   (B, 2, cs, short)):
        rc_i, msg_i = call("scg_rollout_interrupt", flags, n_steps, s, rec, (intr,))
        rc_r, msg_r = call("scg_rollout_record", flags, n_steps, s, rec)
        assert rc_i == rc_r == -1, (flags, n_steps)
        assert msg_i == msg_r.replace("scg_rollout_record", "scg_rollout_interrupt"), (msg_i, msg_r)
        assert msg_i.startswith("scg_rollout_interrupt: ")
    rc, _ = call("scg_rollout_interrupt", B, 1, cs, good, (intr,))
    assert rc == 0
    rc = lib.scg_rollout(ctx._ctx, *arr, C.c_uint32(0b110), C.c_uint64(0), C.c_int32(1), C.c_uint32(A), C.byref(cs), None)
    assert rc == -1 and "unknown flag" in lib.scg_last_error(ctx._ctx).decode()     # scg_rollout still refuses BEGIN_AT


def test_agent_evaluate_and_record_interrupt():
    a = crossing_agent()
    W0, t0 = a.W.clone(), a.t
    st0 = {f: getattr(a.state, f).clone() for f in EnvState.FIELDS}
    with spy_calls(a.ctx) as (calls, _):
        kw = dict(n_episodes=1000, steps_per_launch=32, epsilon=0.05)      # (greedy: one start state, one episode)
        plain = a.evaluate(**kw)
        off = a.evaluate(**kw, interrupt=False)
        on = a.evaluate(**kw, interrupt=True)
        traj, rs = a.record_episodes(**kw, interrupt=True)
        _, rs_plain = a.record_episodes(**kw)
    torch.cuda.synchronize()
    assert calls == [], f"evaluate(interrupt=True) called into the training context: {calls}"
    assert torch.equal(a.W, W0) and a.t == t0
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(a.state, f), st0[f]), f
    assert plain == off and "interrupts" not in plain
    assert rs_plain == plain
    assert list(on) == list(plain) + ["interrupts"] and on["episodes"] == 1000
    assert rs == on
    assert sum(on["interrupts"]) > 0 and on["interrupts"][0] == 0
    ts = traj.summary()
    assert ts["interrupted"] == on["interrupts"]
