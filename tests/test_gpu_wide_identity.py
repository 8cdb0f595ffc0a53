"""SPEC §2's 64-bit run identity on the HIP path: the seed, the step counter t and the global env id past 2^32.

The five kernels that draw random numbers (the fused step, the three rollouts, the trials) each assemble env_draw()'s
arguments on their own (t, t0 + j, t0 + steps; env_base + e, env_base + i), and the re-offer stagger is a second consumer of
the same values. Here every one of them runs with non-zero bits in every upper word — a 64-bit seed, counters at and across
2^32, 2^40, 2^63 and 2^64 - 1, env ids that cross bit 31 and the 2^32 wrap inside one block — against the draw model
(tests/draw_model.py, shown to tell a wide value from its truncation in tests/test_wide_identity.py), the oracle bit for bit,
the float64 model with its own tolerances, and each other. Every comparison is exact or uses the tolerances ref64 derives."""
import numpy as np
import pytest
import torch

import sc_oracle
import skill_chaining_with_graphs_amd as scg
import test_gpu_interrupt as gi
import test_gpu_trials as gt
from draw_model import draws_batch, grid, seven_start_map
from gpu_util import block_envs                               # noqa: F401  (the fixture)
from gpu_util import assert_same_bits, assert_state_equal, clone_state, dev, host_state, make_pair, state_to_device
from skill_chaining_with_graphs_amd.core import EnvState, ScgContext
from skill_chaining_with_graphs_amd.trajectory import BEGIN_ACTION, Trajectory
from test_gpu_ref64 import GpuRunner
from test_gpu_ref64_interrupt import IntGpuRunner
from test_ref64_interrupt import interrupt_sweep_case
from test_ref64_oracle import edge_reoffer_stagger_uses_global_id, sweep_case
from test_wide_identity import (N, W_BASE, W_SEED, WIDE_STEPS, WIDE_SWEEP, SWEEP_IDS, assert_draws, draw_case_state, greedy_qcache,
                                grid_id)
from util import HP, chain_classifiers, random_states, random_weights

pytestmark = pytest.mark.gpu


def _draw_ctx(m, n, seed, base, eps, block=256, n_options=0, **hp):
    return ScgContext(n, n_options, m, device=0, seed=seed, env_id_base=base, block_envs=block,
                      **dict(HP, epsilon=eps, **hp))


def _zeros(n_vf):
    return dev(np.zeros((n_vf, 5, 1296), np.float32)).view(-1), dev(np.zeros((n_vf, 8), np.float32)).view(-1)


# ---------------------------------------------------------------------------------------------------- a. the fused step

@pytest.mark.parametrize("n", [N, 1])
@pytest.mark.parametrize("block", [64, 128, 256])
def test_step_draws_match_the_model_over_the_grid(block, n):
    """eps = 1 and max_episode_steps = 1: the action is a_rand and every env is reset to starts[start], for every cell of
    the wide grid; N = 1000 leaves the last block ragged and puts the 2^32 wrap inside a block."""
    m = seven_start_map()
    W, clf = _zeros(1)
    for cell in grid(N):
        seed, base, t = cell
        if n == 1:
            base = {2 ** 31 - N // 2: 2 ** 31, 2 ** 32 - N // 2: 2 ** 32 - 1}.get(base, base)
        ctx = _draw_ctx(m, n, seed, base, 1.0, block, max_episode_steps=1)
        st = state_to_device(draw_case_state(m, n), ctx)
        ctx.step(st, W, clf, 0, t)
        torch.cuda.synchronize()
        assert_draws(m, host_state(st), n, seed, base, t, msg=f"B={block} {grid_id(cell)}")
        ctx.close()


@pytest.mark.parametrize("eps", [0.2, 0.7])
@pytest.mark.parametrize("block", [64, 256])
def test_step_explore_comparison_at_wide_identities(block, eps):
    m = seven_start_map()
    W, clf = _zeros(1)
    for seed, base, t in [(W_SEED, W_BASE, 2 ** 32 - 1), (W_SEED, W_BASE, 2 ** 64 - 1), (2 ** 64 - 1, 2 ** 40 + 3, 2 ** 32)]:
        ctx = _draw_ctx(m, N, seed, base, eps, block, max_episode_steps=1)
        pre = draw_case_state(m, N)
        pre["qcache"][:], greedy = greedy_qcache(N)
        st = state_to_device(pre, ctx)
        ctx.step(st, W, clf, 0, t)
        torch.cuda.synchronize()
        assert_draws(m, host_state(st), N, seed, base, t, eps=eps, greedy=greedy, msg=f"B={block} t={t}")


@pytest.mark.parametrize("block_envs", [64, 128, 256], indirect=True)
def test_learning_step_equals_the_oracle_at_wide_identities(block_envs):
    """scg_step(LEARN | APPLY) chained over t = 2^32 - 1, 2^32, 2^64 - 1: state, G, n_k and W bit for bit the oracle's."""
    n, n_opt, mask = N, 3, 0b1110
    ctx, orc, m = make_pair("pinball_simple", n, n_options=n_opt, seed=W_SEED, env_id_base=W_BASE, enabled_mask=mask)
    clf = chain_classifiers(m, n_opt)
    st_o = sc_oracle.new_state(n, m)
    st_o["x"][:], st_o["y"][:], st_o["vx"][:], st_o["vy"][:] = random_states(m, n, 1, vmax=1.0)
    st_o["ep_steps"][:] = np.random.default_rng(2).integers(0, HP["max_episode_steps"], n)
    W_o = random_weights(n_opt + 1, 2, std=0.05)
    st_d, W_d, clf_d = state_to_device(st_o, ctx), dev(W_o.copy()), dev(clf)
    G_d, nk_d = ctx.grad_buffers()
    for t in WIDE_STEPS:
        G, n_k = orc.step(st_o, W_o, clf, t)
        orc.apply(W_o, G, n_k)
        ctx.step(st_d, W_d.view(-1), clf_d.view(-1), mask, t)
        torch.cuda.synchronize()
        assert_state_equal(st_d, st_o, msg=f"B={block_envs} t={t}")
        assert np.array_equal(nk_d.cpu().numpy(), n_k), f"n_k at t={t}"
        assert np.array_equal(G_d.cpu().numpy(), G), f"G at t={t}"
        assert np.array_equal(W_d.cpu().numpy(), W_o), f"W at t={t}"
    assert int((st_o["option_id"] != 0).sum()) > 0 and int(n_k[1:].sum()) > 0


WIDE_GPU = [(c, b) for b in (256, 128, 64) for c in WIDE_SWEEP]


@pytest.mark.parametrize("cfg,block_envs", WIDE_GPU, indirect=["block_envs"],
                         ids=[f"b{b}-{i}" for b in (256, 128, 64) for i in SWEEP_IDS])
def test_hip_step_matches_the_float64_model_at_wide_identities(cfg, block_envs):
    sweep_case(GpuRunner, cfg, block_envs, steps=WIDE_STEPS, seed=W_SEED)


@pytest.mark.parametrize("block_envs", [256], indirect=True)
def test_hip_interrupting_step_matches_the_float64_model_at_wide_identities(block_envs):
    interrupt_sweep_case(IntGpuRunner, WIDE_SWEEP[-1], block_envs, steps=WIDE_STEPS, seed=W_SEED)


@pytest.mark.parametrize("period", [4, 8])
@pytest.mark.parametrize("block_envs", [256, 64], indirect=True)
def test_hip_reoffer_stagger_across_the_wrap(block_envs, period):
    edge_reoffer_stagger_uses_global_id(GpuRunner, seed=W_SEED, env_id_base=2 ** 32 - 128, period=period,
                                        steps=(2 ** 32 - 1, 2 ** 32))


def test_step_keeps_refusing_a_bad_counter_on_the_cached_fast_path():
    m = seven_start_map()
    W, clf = _zeros(1)
    ctx = _draw_ctx(m, 64, W_SEED, W_BASE, 1.0)
    st = state_to_device(draw_case_state(m, 64), ctx)
    ctx.step(st, W, clf, 0, 2 ** 64 - 2)
    ctx.step(st, W, clf, 0, 2 ** 64 - 1)                       # the second call goes through the cached arguments
    assert ctx._step_args is not None
    torch.cuda.synchronize()
    before = host_state(st)
    for t in (-1, 2 ** 64):
        with pytest.raises(scg.ScgError, match="64-bit unsigned step counter"):
            ctx.step(st, W, clf, 0, t)
    torch.cuda.synchronize()
    after = host_state(st)
    assert all(np.array_equal(before[f], after[f]) for f in EnvState.FIELDS)
    with pytest.raises(scg.ScgError, match="64-bit"):
        ScgContext(64, 0, m, seed=2 ** 64)


# ---------------------------------------------------------------------------------------------------- b. rollouts

def _rollout_pair(n=N, n_opt=3, mask=0b1110, eps=0.1, base=W_BASE):
    ctx, orc, m = make_pair("pinball_simple", n, n_options=n_opt, seed=W_SEED, env_id_base=base, enabled_mask=mask, epsilon=eps,
                            reoffer_period=4)
    clf = chain_classifiers(m, n_opt)
    W = random_weights(n_opt + 1, 4, std=0.1)
    st_o = sc_oracle.new_state(n, m)
    rng = np.random.default_rng(5)
    st_o["x"][:], st_o["y"][:], st_o["vx"][:], st_o["vy"][:] = random_states(m, n, 5, vmax=1.5)
    st_o["option_id"][:] = rng.integers(-n_opt, n_opt + 1, n)
    st_o["ep_steps"][:] = rng.integers(0, HP["max_episode_steps"], n)
    st_o["qcache"][:] = rng.standard_normal((5, n)).astype(np.float32)
    return ctx, orc, m, W, clf, st_o


@pytest.mark.parametrize("epw", [2, 32])
@pytest.mark.parametrize("t0", [2 ** 32 - 3, 2 ** 40, 2 ** 64 - 3], ids=["2^32-3", "2^40", "2^64-3"])
def test_rollout_across_the_counter_boundary(t0, epw, monkeypatch):
    """One launch of 8 steps whose counter crosses 2^32 (2^64: t0 + j wraps) equals 8 acting scg_step calls and the oracle's
    step loop, in a small and a large launch geometry."""
    monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
    mask, K = 0b1110, 8
    ctx, orc, m, W, clf, st_o = _rollout_pair()
    st = state_to_device(st_o, ctx)
    twin = clone_state(st)
    W_d, clf_d = dev(W).view(-1), dev(clf).view(-1)
    ctx.rollout(st, W_d, clf_d, mask, t0, K)
    for j in range(K):
        t = (t0 + j) % 2 ** 64
        ctx.step(twin, W_d, clf_d, mask, t, learn=False)
        orc.step(st_o, W, clf, t)                              # W not applied: acting only
    torch.cuda.synchronize()
    assert_same_bits(st, twin, msg=f"rollout({K}) at t0={t0} vs {K} acting steps")
    assert_state_equal(st, st_o, msg=f"rollout({K}) at t0={t0} vs the oracle")
    assert int((st_o["option_id"] > 0).sum()) > 0


def test_begin_draws_on_either_side_of_the_boundary():
    """BEGIN at t0 = 2^32 - 1: the begin draw is the last below the boundary, the first step (t0 + 1 = 2^32) the first above."""
    m = seven_start_map()
    t0 = 2 ** 32 - 1
    W, clf = _zeros(1)
    S = np.asarray(m.starts, np.float32)
    ctx = _draw_ctx(m, N, W_SEED, W_BASE, 1.0, max_episode_steps=1)
    st = state_to_device(draw_case_state(m, N), ctx)
    ctx.rollout(st, W, clf, 0, t0, 0, begin=True)
    torch.cuda.synchronize()
    start = draws_batch(W_BASE, N, W_SEED, t0, 7)[2]
    h = host_state(st)
    assert np.array_equal(h["x"].view(np.uint32), S[start, 0].view(np.uint32)), "BEGIN's start positions (x)"
    assert np.array_equal(h["y"].view(np.uint32), S[start, 1].view(np.uint32)), "BEGIN's start positions (y)"
    st = state_to_device(draw_case_state(m, N), ctx)
    ctx.rollout(st, W, clf, 0, t0, 1, begin=True)              # max_episode_steps = 1: the step at t0 + 1 resets again
    torch.cuda.synchronize()
    assert_draws(m, host_state(st), N, W_SEED, W_BASE, t0 + 1, msg="the step after BEGIN")


@pytest.mark.parametrize("begin", [False, True])
def test_recorded_actions_are_the_models_draws(begin):
    """scg_rollout_record with eps = 1: row j's action is a_rand at (g, t0 + j); with BEGIN row 0 is the begin row (its
    position starts[start] at t0) and step row j >= 1 ran at t0 + j (SPEC §8)."""
    m = seven_start_map()
    t0, K = 2 ** 32 - 3, 8
    W, clf = _zeros(1)
    ctx = _draw_ctx(m, N, W_SEED, W_BASE, 1.0)
    st = state_to_device(draw_case_state(m, N), ctx)
    rows = K + (1 if begin else 0)
    tr = Trajectory(N, rows, 0, ctx.device)
    ctx.rollout(st, W, clf, 0, t0, K, begin=begin, record=tr)
    torch.cuda.synchronize()
    assert np.all(tr.len.cpu().numpy() == rows)
    act = tr.action.cpu().numpy()
    for j in range(rows):
        if begin and j == 0:
            start = draws_batch(W_BASE, N, W_SEED, t0, 7)[2]
            S = np.asarray(m.starts, np.float32)
            assert np.all(act[0] == BEGIN_ACTION)
            assert np.array_equal(tr.x.cpu().numpy()[0], S[start, 0]) and np.array_equal(tr.y.cpu().numpy()[0], S[start, 1])
            continue
        a_rand = draws_batch(W_BASE, N, W_SEED, t0 + j, 7)[1]
        assert np.array_equal(act[j].astype(np.int64), a_rand), f"row {j} (t = t0 + {j}): {np.sum(act[j] != a_rand)} actions differ"


def test_interrupting_rollout_equals_the_emulator_across_the_boundary():
    """scg_rollout_interrupt against test_gpu_interrupt's emulator (one-step launches): BEGIN at 2^32 - 9, then launches of 7,
    9 and 16 steps, the second of which crosses 2^32. (The emulator's one-step launches run the same kernel: this ties the
    multi-step launch's t0 + j to single steps at the same counters; test_rollout_across_the_counter_boundary ties those to
    the oracle.)"""
    gi._run_case(*gi.CASES[1], "begin", seed=W_SEED, t0=2 ** 32 - 9, env_id_base=2 ** 32 - 2048)


# ---------------------------------------------------------------------------------------------------- c. trials

TRIAL_T0 = 2 ** 32 - 2


@pytest.mark.parametrize("eps", [1.0, 0.2])
def test_trials_across_the_counter_boundary(eps):
    """t0 = 2^32 - 2 and up to 7 steps per trial: the launch equals test_gpu_trials' step loop, and with a record every row's
    action equals the step loop's draw — for eps = 1 the draw model's a_rand at (env_id_base + i, t0 + j)."""
    n, base = 257, 2 ** 32 - 128
    case = ("pinball_simple", n, 3, 0b1010, 0b0100, [0, 0, 1, 1], eps, 0.0, 7, 60, base)
    ctx, m, W, clf = gt._setup(case, seed=W_SEED)
    *s0, opt = gt._starts(m, n, 3, seed=n + 3)
    got = gt._trials(ctx, s0, opt, W, clf, case[3], TRIAL_T0)
    model, run = gt._model_for(ctx, case, s0, opt, W, clf, TRIAL_T0)
    gt._assert_trials_equal(got, model, run, "trials at t0 = 2^32 - 2 vs the step loop")
    assert run.any() and int(got["steps"][run].max()) >= 4, "no trial crosses the boundary by more than a step"
    res = scg.TrialResult(n, opt, ctx.device)
    tr = Trajectory(n, 7, 0, ctx.device)
    ctx.option_trials(*[dev(v) for v in s0], res.option, W, clf, case[3], TRIAL_T0, res, record=tr)
    torch.cuda.synchronize()
    ln, act = tr.len.cpu().numpy(), tr.action.cpu().numpy()
    assert np.array_equal(ln[run], got["steps"][run]) and np.all(ln[~run] == 0)
    if eps == 1.0:
        for j in range(7):
            a_rand = draws_batch(base, n, W_SEED, TRIAL_T0 + j, 7)[1]
            live = ln > j
            assert np.array_equal(act[j][live].astype(np.int64), a_rand[live]), f"row {j}: actions differ from the draw model"


# ---------------------------------------------------------------------------------------------------- d. sharding across the wrap

def test_two_shards_meeting_at_2_pow_32_equal_one_context():
    """Two contexts of N/2 envs at bases B and B + N/2 = 2^32 equal one context of N envs at B on every acting output, and their
    summed packed gradients equal the oracle's two shards, at a wide t and seed."""
    ns, n_opt, mask = N // 2, 2, 0b110
    B = 2 ** 32 - ns
    ranks = [make_pair("pinball_simple", ns, n_options=n_opt, seed=W_SEED, env_id_base=B + r * ns, enabled_mask=mask)
             for r in range(2)]
    m = ranks[0][2]
    full = ScgContext(N, n_opt, m, device=0, seed=W_SEED, env_id_base=B, block_envs=256, **HP)
    x, y, vx, vy = random_states(m, N, 11, vmax=1.0)
    clf = chain_classifiers(m, n_opt)
    W_o = random_weights(n_opt + 1, 4, std=0.05)
    st_o, st_d, W_d, gp = [], [], [], []
    for r, (ctx, orc, _) in enumerate(ranks):
        st = sc_oracle.new_state(ns, m)
        sl = slice(r * ns, (r + 1) * ns)
        st["x"][:], st["y"][:], st["vx"][:], st["vy"][:] = x[sl], y[sl], vx[sl], vy[sl]
        st_o.append(st); st_d.append(state_to_device(st, ctx)); W_d.append(dev(W_o.copy())); gp.append(ctx.grad_packed())
    st_all = sc_oracle.new_state(N, m)
    st_all["x"][:], st_all["y"][:], st_all["vx"][:], st_all["vy"][:] = x, y, vx, vy
    st_full = state_to_device(st_all, full)
    clf_d = dev(clf)
    nw = (n_opt + 1) * 5 * 1296
    for t in (2 ** 32 - 1, 2 ** 32, 2 ** 63):
        full.step(st_full, W_d[0].view(-1), clf_d.view(-1), mask, t, learn=False)      # (before the update: the step's frozen W)
        G, n = [], []
        for r, (ctx, orc, _) in enumerate(ranks):
            g_r, n_r = orc.step(st_o[r], W_o, clf, t)
            G.append(g_r); n.append(n_r)
            ctx.step(st_d[r], W_d[r].view(-1), clf_d.view(-1), mask, t, learn=True, apply=False)
        total = gp[0] + gp[1]                                       # the all-reduce
        for r, (ctx, orc, _) in enumerate(ranks):
            assert np.array_equal(gp[r][:nw].cpu().numpy().reshape(n_opt + 1, 5, 1296), G[r]), f"rank {r} gradient, t={t}"
            gp[r].copy_(total)
            ctx.apply_update_packed(W_d[r].view(-1), gp[r])
        ranks[0][1].apply(W_o, G[0] + G[1], n[0] + n[1])
        torch.cuda.synchronize()
        assert np.array_equal(total[nw:].cpu().numpy(), (n[0] + n[1]).astype(np.float32))
        for r in range(2):
            assert_state_equal(st_d[r], st_o[r], msg=f"rank {r} t={t}")
        hf = host_state(st_full)
        for f in EnvState.FIELDS:
            both = np.concatenate([getattr(st_d[r], f).cpu().numpy() for r in range(2)], axis=-1)
            assert np.array_equal(hf[f].view(np.uint8), both.view(np.uint8)), f"t={t}: {f} of the two shards differs from one context"
        assert torch.equal(W_d[0], W_d[1])
        assert np.array_equal(W_d[0].cpu().numpy(), W_o), f"weights differ from the oracle's two-shard result at t={t}"


# ---------------------------------------------------------------------------------------------------- e. the agent

def _agent(m, n=N, n_opt=2, **hp):
    from skill_chaining_with_graphs_amd.agent import SkillChainingAgent
    ag = SkillChainingAgent(m, n, n_opt, seed=W_SEED, env_id_base=2 ** 32 - n // 2, block_envs=256, **dict(HP, **hp))
    ag.init_weights(std=0.05, seed=3)
    ag.clf.copy_(dev(chain_classifiers(m, n_opt)))
    ag.enable_option(1)
    ag.enable_option(2)
    x, y, vx, vy = random_states(m, n, 7, vmax=1.0)
    for t, v in zip(ag.state.state(), (x, y, vx, vy)):
        t.copy_(dev(v))
    ag.ctx.invalidate_order()
    return ag


def test_agent_checkpoint_across_the_counter_boundary(tmp_path):
    """seed = 2^63 + 3, agent.t from 2^32 - 2: two step-batches, save, three more; a second agent loads the file and runs three:
    state and W bit-identical, t a Python int throughout."""
    m = scg.load_map("pinball_simple")
    a = _agent(m)
    a.t = 2 ** 32 - 2
    a.rollout(2)
    path = str(tmp_path / "ckpt.pt")
    a.save(path)
    assert a.t == 2 ** 32 and type(a.state_dict()["t"]) is int
    a.rollout(3)
    b = _agent(m)
    b.W.zero_()
    b.load(path)
    assert b.t == 2 ** 32 and type(b.t) is int
    b.rollout(3)
    torch.cuda.synchronize()
    assert a.t == b.t == 2 ** 32 + 3
    assert torch.equal(a.W, b.W), "the resumed run's weights differ"
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(a.state, f), getattr(b.state, f)), f"the resumed run's state differs ({f})"


def test_agent_evaluation_seeds_past_2_pow_32():
    """evaluate(seed = 2^40 + 1) and evaluate(seed = 1) start (and, with max_episode_steps = 1, end) their episodes at
    different start positions — each the draw model's — and record_episodes' begin rows are the draw model's starts."""
    m = seven_start_map()
    S = np.asarray(m.starts, np.float32)
    n = 256
    a = _agent(m, max_episode_steps=1)
    ends = {}
    for seed in (2 ** 40 + 1, 1):
        out = a.evaluate(n_episodes=n, epsilon=1.0, seed=seed, steps_per_launch=4)
        assert out["episodes"] == n
        st = a._eval_ctx[n][1]
        torch.cuda.synchronize()
        start = draws_batch(0, n, seed, 1, 7)[2]               # the one step of each episode runs at t = 1 and resets
        assert np.array_equal(st.x.cpu().numpy(), S[start, 0]) and np.array_equal(st.y.cpu().numpy(), S[start, 1]), f"seed {seed}"
        ends[seed] = st.x.cpu().numpy().copy()
        traj, _ = a.record_episodes(n_episodes=n, epsilon=1.0, seed=seed, steps_per_launch=4)
        begin = draws_batch(0, n, seed, 0, 7)[2]
        bx = np.array([traj.per_env(i)["x"][0] for i in range(n)], np.float32)
        by = np.array([traj.per_env(i)["y"][0] for i in range(n)], np.float32)
        assert np.array_equal(bx, S[begin, 0]) and np.array_equal(by, S[begin, 1]), f"begin rows, seed {seed}"
        a_rand = draws_batch(0, n, seed, 1, 7)[1]
        act = np.array([traj.per_env(i)["action"][1] for i in range(n)], np.int64)
        assert np.array_equal(act, a_rand), f"first step's actions, seed {seed}"
    assert np.mean(ends[2 ** 40 + 1] != ends[1]) >= 0.5
