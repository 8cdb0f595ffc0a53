"""SPEC §11 interrupting rollouts on the GPU: one scg_rollout_interrupt launch equals an emulator built from already-verified
entry points (scg_rollout one step at a time, scg_q_values for V_0, scg_classifier_predict for the candidate), and the same
emulator on the oracle; every launch geometry and block build agree; with every W_k == W_0 nothing is interrupted; the record
marks interrupted rows INTERRUPTED; the agent's evaluate(interrupt=True) / record_episodes(interrupt=True) leave training
alone; and the C-ABI's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import interrupt_learning_model as ilm
import sc_oracle
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
from skill_chaining_with_graphs_amd.trajectory import Trajectory
from gpu_util import (as_bytes, assert_same_bits, clone_state, crossing_agent, dev, make_context, make_pair, spy_calls,
                      state_to_device)
from util import HP, chain_classifiers, random_env_state, random_states

pytestmark = pytest.mark.gpu

STATS = EpisodeStats.FIELDS


def _setup(name, n, n_opt, parents=None, gest=0, seed=3, block=None, **hp):
    m = scg.load_map(name)
    ctx = make_context(m, n, n_opt, block, parents, gest, seed, **hp)
    clf = dev(ilm.wide_chain(m, n_opt)).view(-1)
    W = dev(ilm.crossing_weights(n_opt + 1, seed)).view(-1)
    return ctx, m, W, clf


def _state(ctx, m, n, n_opt, seed):
    return state_to_device(random_env_state(m, n, n_opt, seed, id_lo=-n_opt, id_hi=n_opt, opt_steps_hi=10,
                                            max_episode_steps=ctx.cfg.max_episode_steps), ctx)


def _candidates(predict, x, y, n_vf, known, enabled, parents):
    """SPEC §4.2's cand at s' = (x, y), by ilm.candidates from the known options' membership bits (no bit for the others)."""
    in_n = np.zeros((n_vf, len(x)), bool)
    for k in range(1, n_vf):
        if (known >> k) & 1:
            in_n[k] = predict(k, x, y) != 0
    return ilm.candidates(in_n, enabled, parents, n_vf)


class Emulator:
    """SPEC §11 from scg_rollout_record launches of ONE step each (begin: a launch of 0 steps), patched after every step."""

    def __init__(self, ctx, W, clf, mask, gest):
        self.ctx, self.W, self.clf, self.mask = ctx, W, clf, mask
        self.known = mask | gest
        self.n, self.n_vf = ctx.n_envs, ctx.n_vf
        self.parents = [int(p) for p in ctx.parents]
        self.W0 = W.view(self.n_vf, -1)[0].contiguous()
        self.W8 = clf.view(self.n_vf, -1)
        self.kept = self.interrupted = 0
        self.rows, self.lens = [], []              # per pseudo-step: the record's row (host) and len

    def _predict(self, k, x, y):
        return self.ctx.classifier_predict(dev(x), dev(y), self.W8[k].contiguous()).cpu().numpy()

    def _launch(self, st, t, n_steps, stats, **kw):
        tr = Trajectory(self.n, 1, 0, self.ctx.device)
        self.ctx.rollout(st, self.W, self.clf, self.mask, t, n_steps, stats, record=tr, **kw)
        return tr

    def _keep_row(self, tr):
        self.rows.append({f: getattr(tr, f)[0].cpu().numpy().copy() for f in tr.fields})
        self.lens.append(tr.len.cpu().numpy().copy())

    def run(self, st, t0, K, stats, interrupts, begin=False, begin_at=False, one_episode=False):
        t = t0
        if begin or begin_at:
            self._keep_row(self._launch(st, t0, 0, stats, begin=begin, begin_at=begin_at, one_episode=one_episode))
            t = t0 + 1
        n_vf = self.n_vf
        for j in range(K):
            o_b, s_b = st.option_id.cpu().numpy(), st.opt_steps.cpu().numpy()
            tr = self._launch(st, t + j, 1, stats, one_episode=one_episode)
            row = {f: getattr(tr, f)[0].cpu().numpy().copy() for f in tr.fields}
            s_a = st.opt_steps.cpu().numpy()
            kept = (o_b >= 1) & (o_b < n_vf) & (s_a == s_b + 1)
            idx = np.nonzero(kept)[0]
            self.kept += len(idx)
            if len(idx):
                it = torch.as_tensor(idx, device=self.ctx.device)
                s = [getattr(st, f)[it].contiguous() for f in ("x", "y", "vx", "vy")]
                q0 = self.ctx.q_values(s, self.W0).cpu().numpy()
                qo = st.qcache.view(5, self.n)[:, it].cpu().numpy()
                cut = ~(ilm.vmax(qo) >= ilm.vmax(q0))
                if cut.any():
                    xs, ys = s[0].cpu().numpy(), s[1].cpu().numpy()
                    c = _candidates(self._predict, xs[cut], ys[cut], n_vf, self.known, self.mask, self.parents)
                    e = idx[cut]
                    et = torch.as_tensor(e, device=self.ctx.device)
                    st.option_id[et] = torch.as_tensor(-c.astype(np.int32), device=self.ctx.device)
                    st.opt_steps[et] = 0
                    qc = st.qcache.view(5, self.n)
                    qc[:, et] = torch.as_tensor(q0[:, cut], device=self.ctx.device)
                    np.add.at(interrupts, (o_b[e], e), 1)
                    row["option_id"][e] = -c.astype(np.int8)
                    row["term"][e] = _lib.ROLLOUT_TERM_INTERRUPTED
                    self.interrupted += len(e)
            self.rows.append(row)
            self.lens.append(tr.len.cpu().numpy().copy())

    def record(self):
        """The rows a recorded launch of all these pseudo-steps holds: [rows][n] per field, and len."""
        ln = np.sum(self.lens, axis=0)
        return {f: np.stack([r[f] for r in self.rows]) for f in self.rows[0]}, ln


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
    ref_int = np.zeros((n_vf, n), np.int64)
    emu = Emulator(ctx, W, clf, mask, gest)
    begin, at, one = mode == "begin", mode == "begin_at", mode in ("begin", "begin_at", "one_episode")
    t = t0
    for i, K in enumerate(splits):
        first = i == 0
        emu.run(st, t, K, s_ref, ref_int, begin=begin and first, begin_at=at and first, one_episode=one)
        ctx.rollout(twin, W, clf, mask, t, K, s_int, begin=begin and first, begin_at=at and first, one_episode=one,
                    interrupt=True)
        t += K + (1 if (begin or at) and first else 0)
    torch.cuda.synchronize()
    assert_same_bits(twin, st, EnvState.FIELDS, f"{name} {mode}")
    assert_same_bits(s_int, s_ref, STATS, f"{name} {mode} stats")
    assert np.array_equal(s_int.interrupts.cpu().numpy(), ref_int), f"{name} {mode}: interrupts differ"
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
    W = ilm.crossing_weights(n_opt + 1, 4)
    n_vf = n_opt + 1
    st_o = sc_oracle.new_state(n, m)
    rng = np.random.default_rng(5)
    st_o["x"][:], st_o["y"][:], st_o["vx"][:], st_o["vy"][:] = random_states(m, n, 5, vmax=1.5)
    st_o["option_id"][:] = rng.integers(-n_opt, n_opt + 1, n)
    st_o["opt_steps"][:] = rng.integers(0, 10, n)
    st_o["ep_steps"][:] = rng.integers(0, HP["max_episode_steps"], n)
    st_o["qcache"][:] = rng.standard_normal((5, n)).astype(np.float32)
    st_d = state_to_device(st_o, ctx)
    parents = [int(p) for p in ctx.parents]
    ref_int = np.zeros((n_vf, n), np.int64)
    K, t0, cuts = 20, 77, 0
    for t in range(t0, t0 + K):
        o_b, s_b = st_o["option_id"].copy(), st_o["opt_steps"].copy()
        orc.step(st_o, W, clf, t)                          # W not applied: acting only
        kept = (o_b >= 1) & (o_b < n_vf) & (st_o["opt_steps"] == s_b + 1)
        idx = np.nonzero(kept)[0]
        if not len(idx):
            continue
        s = [np.ascontiguousarray(st_o[f][idx]) for f in ("x", "y", "vx", "vy")]
        q0 = orc.q_values(*s, W[0])
        cut = ~(ilm.vmax(st_o["qcache"][:, idx]) >= ilm.vmax(q0))
        c = _candidates(lambda k, x, y: orc.classifier_predict(x, y, clf[k]), s[0][cut], s[1][cut], n_vf, mask, mask, parents)
        e = idx[cut]
        st_o["option_id"][e] = -c
        st_o["opt_steps"][e] = 0
        st_o["qcache"][:, e] = q0[:, cut]
        np.add.at(ref_int, (o_b[e], e), 1)
        cuts += len(e)
    intr = torch.zeros((n_vf, n), dtype=torch.int32, device=ctx.device)
    ctx.rollout(st_d, dev(W).view(-1), dev(clf).view(-1), mask, t0, K, interrupt=True, interrupts=intr)
    torch.cuda.synchronize()
    assert cuts > 0
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(st_d, f)), as_bytes(st_o[f])), f"oracle emulator: {f} differs"
    assert np.array_equal(intr.cpu().numpy(), ref_int)


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
    twin = clone_state(st)
    a, b = EpisodeStats(n_opt + 1, n, ctx.device), EpisodeStats(n_opt + 1, n, ctx.device)
    ctx.rollout(st, Wt, clf, mask, 40, 48, a, begin=True)
    ctx.rollout(twin, Wt, clf, mask, 40, 48, b, begin=True, interrupt=True)
    torch.cuda.synchronize()
    assert_same_bits(twin, st, EnvState.FIELDS, "ties")
    assert_same_bits(b, a, STATS, "ties stats")
    assert int(b.interrupts.sum()) == 0 and b.summary()["interrupts"] == [0] * (n_opt + 1)
    assert int(a.vf_steps[1:].sum()) > 0, "no option ran: the tie check is vacuous"


@pytest.mark.parametrize("mode", ["begin", "one_episode"])
def test_record_rows_equal_emulator(mode):
    n, n_opt, mask = 4096, 3, 0b1110
    ctx, m, W, clf = _setup("pinball_simple", n, n_opt, epsilon=0.1, reoffer_period=4, max_episode_steps=30)
    st = _state(ctx, m, n, n_opt, seed=31)
    twin, plain = clone_state(st), clone_state(st)
    emu = Emulator(ctx, W, clf, mask, 0)
    s_ref, s_int, s_plain = (EpisodeStats(n_opt + 1, n, ctx.device) for _ in range(3))
    ref_int = np.zeros((n_opt + 1, n), np.int64)
    one = mode == "one_episode"
    K = 40
    emu.run(st, 9, K, s_ref, ref_int, begin=True, one_episode=one)
    tr = Trajectory(n, K + 1, 0, ctx.device)
    ctx.rollout(twin, W, clf, mask, 9, K, s_int, begin=True, one_episode=one, interrupt=True, record=tr)
    ctx.rollout(plain, W, clf, mask, 9, K, s_plain, begin=True, one_episode=one, interrupt=True)
    torch.cuda.synchronize()
    assert_same_bits(twin, st, EnvState.FIELDS, "recorded")
    assert_same_bits(plain, twin, EnvState.FIELDS, "recording changed the outputs")
    assert_same_bits(s_plain, s_int, STATS + ("interrupts",), "recording changed the counters")
    assert np.array_equal(s_int.interrupts.cpu().numpy(), ref_int)
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
