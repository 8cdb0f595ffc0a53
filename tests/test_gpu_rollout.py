"""SPEC §8 acting rollouts (scg_rollout) on the GPU: K steps in one launch equal K acting scg_step calls bit for bit, the
oracle's step, a numpy model of the episode counters, BEGIN / ONE_EPISODE, and SkillChainingAgent.evaluate()."""
import math

import numpy as np
import pytest
import torch

import option_rules as rules
import sc_oracle
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
from gpu_util import (GpuBackend, assert_same_bits, assert_state_equal, clone_state, dev, gestating_agent, host_state, make_context,
                      make_pair, named_map, spy_calls, state_to_device)
from util import HP, chain_classifiers, dense_map, random_env_state, random_states, random_weights

pytestmark = pytest.mark.gpu

def _state(ctx, m, n, n_opt, seed):
    """Option ids in [-n_opt - 1, n_opt + 1]: out-of-range ids included."""
    return state_to_device(random_env_state(m, n, n_opt, seed, id_lo=-n_opt - 1, id_hi=n_opt + 1, opt_steps_hi=20,
                                            max_episode_steps=ctx.cfg.max_episode_steps), ctx)


def _setup(m, n, n_opt, block=None, parents=None, gest=0, seed=3, **hp):
    ctx = make_context(m, n, n_opt, block, parents, gest, seed, **hp)
    clf = dev(chain_classifiers(m, n_opt)).view(-1)
    W = dev(random_weights(n_opt + 1, seed, std=0.1)).view(-1)
    return ctx, W, clf


CASES = [
    # map, n, options, enabled, gestating, parents, reoffer, epsilon, env_id_base, block
    ("pinball_simple", 4096, 3, 0b1010, 0b0100, None, 4, 0.1, 0, None),
    ("pinball_simple", 1000, 3, 0b1110, 0, [0, 0, 1, 1], 1, 0.0, 12345, 64),
    ("pinball_simple", 257, 3, 0b1110, 0, [0, 0, 1, 2], 8, 0.1, 7, 128),
    ("dense", 1000, 2, 0b110, 0, None, 4, 0.1, 0, 256),
    ("hub", 257, 2, 0b110, 0, None, 4, 0.0, 3, None),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-b{c[9]}-r{c[6]}")
def test_rollout_equals_step_loop(case):
    name, n, n_opt, mask, gest, parents, reoffer, eps, base, block = case
    m = named_map(name)
    ctx, W, clf = _setup(m, n, n_opt, block, parents, gest, reoffer_period=reoffer, epsilon=eps, env_id_base=base)
    st = _state(ctx, m, n, n_opt, seed=n)
    twin = clone_state(st)
    W0 = W.clone()
    K, t0 = 24, 1000
    ctx.rollout(st, W, clf, mask, t0, K)
    for t in range(t0, t0 + K):
        ctx.step(twin, W, clf, mask, t, learn=False)
    torch.cuda.synchronize()
    assert_same_bits(st, twin, msg=f"rollout({K}) vs {K} acting steps")
    assert torch.equal(W, W0), "a rollout wrote W"
    assert int((twin.done != 0).sum()) > 0, "the case ends no episode: it tests less than it should"


def _auto_epw(n):
    """The launch geometry scg_rollout picks for n envs (envs per wave; csrc/scg_kernels.hip, scg_rollout)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    epw = 2
    while epw < 32 and n >= cus * 8 * epw * 2:
        epw *= 2
    return epw


LARGE_CASES = [
    # the geometries of larger env counts, as scg_rollout picks them (on a 256-CU chip: 4, 8, 8, 16, 32 envs per wave); the
    # dense map gives waves of 8 .. 32 envs several 64-slot groups of (env, edge) pairs per step
    ("pinball_simple", 10000, 3, 0b1010, 0b0100, [0, 0, 1, 1], 4, 0.1, 3, None),
    ("dense", 16384, 2, 0b110, 0, None, 4, 0.1, 0, None),
    ("pinball_simple", 20000, 3, 0b1110, 0, [0, 0, 1, 2], 8, 0.1, 99, None),
    ("hub", 40000, 2, 0b110, 0, None, 1, 0.1, 0, None),
    ("dense", 65536, 3, 0b1010, 0b0100, None, 4, 0.1, 0, None),
]


@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_rollout_equals_step_loop_large(case):
    n = case[1]
    if n >= 16384:
        assert _auto_epw(n) >= 8, "this case no longer runs a larger launch geometry"
    test_rollout_equals_step_loop(case)


def test_rollout_every_launch_geometry(monkeypatch):
    """Every envs-per-wave geometry (SCG_ROLLOUT_EPW pins it) gives the step loop's bits: workgroups of 16 .. 256 envs, a
    ragged tail, dense-map waves with several pair groups, unit lists of many units."""
    m = dense_map()
    n, n_opt, mask, gest = 5000, 3, 0b1010, 0b0100
    ctx, W, clf = _setup(m, n, n_opt, None, [0, 0, 1, 1], gest, reoffer_period=4, epsilon=0.1, env_id_base=17)
    st0 = _state(ctx, m, n, n_opt, seed=41)
    twin = clone_state(st0)
    K, t0 = 24, 500
    for t in range(t0, t0 + K):
        ctx.step(twin, W, clf, mask, t, learn=False)
    for epw in (2, 4, 8, 16, 32):
        monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
        st = clone_state(st0)
        ctx.rollout(st, W, clf, mask, t0, K)
        torch.cuda.synchronize()
        assert_same_bits(st, twin, msg=f"epw {epw}")
    monkeypatch.setenv("SCG_ROLLOUT_EPW", "3")
    with pytest.raises(scg.ScgError):
        ctx.rollout(clone_state(st0), W, clf, mask, t0, K)


def test_rollout_split_launches_and_block_builds():
    """3 launches of 21 steps = one of 63; and the three block builds' libraries give the same rollout (nothing of the block
    size reaches the rollout kernel: this checks that the three libraries carry the same entry point; the launch geometry is
    covered by test_rollout_every_launch_geometry)."""
    m = scg.load_map("pinball_simple")
    outs = []
    for block in (64, 128, 256):
        ctx, W, clf = _setup(m, 1000, 3, block, gest=0b0100, epsilon=0.1)
        st = _state(ctx, m, 1000, 3, seed=11)
        ctx.rollout(st, W, clf, 0b1010, 5, 63)
        outs.append(st)
        if block == 256:                                   # 3 x 21 steps = one launch of 63
            st3 = _state(ctx, m, 1000, 3, seed=11)
            for i in range(3):
                ctx.rollout(st3, W, clf, 0b1010, 5 + 21 * i, 21)
            torch.cuda.synchronize()
            assert_same_bits(st3, st, msg="3 x 21 vs 63")
    torch.cuda.synchronize()
    assert_same_bits(outs[0], outs[2], msg="block 64 vs 256")
    assert_same_bits(outs[1], outs[2], msg="block 128 vs 256")


def _oracle_case():
    """257 envs on a context / oracle pair, two chain options, one running state on both sides."""
    n, n_opt, mask = 257, 2, 0b110
    ctx, orc, m = make_pair("pinball_simple", n, n_options=n_opt, seed=9, enabled_mask=mask)
    st_o = sc_oracle.new_state(n, m)
    rng = np.random.default_rng(5)
    st_o["x"][:], st_o["y"][:], st_o["vx"][:], st_o["vy"][:] = random_states(m, n, 5, vmax=1.5)
    st_o["option_id"][:] = rng.integers(-n_opt, n_opt + 1, n)
    st_o["ep_steps"][:] = rng.integers(0, HP["max_episode_steps"], n)
    st_o["qcache"][:] = rng.standard_normal((5, n)).astype(np.float32)
    return ctx, orc, n, mask, chain_classifiers(m, n_opt), random_weights(n_opt + 1, 4, std=0.1), st_o, state_to_device(st_o, ctx)


@pytest.mark.parametrize("epw", [None, 8, 32])
def test_rollout_equals_oracle(epw, monkeypatch):
    if epw:
        monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
    ctx, orc, n, mask, clf, W, st_o, st_d = _oracle_case()
    K, t0 = 12, 77
    for t in range(t0, t0 + K):
        orc.step(st_o, W, clf, t)                          # W not applied: acting only
    ctx.rollout(st_d, dev(W).view(-1), dev(clf).view(-1), mask, t0, K)
    torch.cuda.synchronize()
    assert_state_equal(st_d, st_o, msg="rollout vs oracle")


def test_begin_equals_oracle_reset_step():
    n, n_opt, mask = 1000, 3, 0b1110
    ctx, orc, m = make_pair("pinball_simple", n, n_options=n_opt, seed=2, enabled_mask=mask, epsilon=0.1)
    clf = chain_classifiers(m, n_opt)
    W = random_weights(n_opt + 1, 8, std=0.1)
    st_o = sc_oracle.new_state(n, m)
    st_o["x"][:], st_o["y"][:], st_o["vx"][:], st_o["vy"][:] = random_states(m, n, 8, vmax=1.5)
    st_o["ep_steps"][:] = HP["max_episode_steps"] - 1
    st_o["qcache"][:] = np.random.default_rng(8).standard_normal((5, n)).astype(np.float32)
    st_d = state_to_device(st_o, ctx)
    stats = EpisodeStats(n_opt + 1, n, ctx.device)
    stats.ep_return.fill_(3.0); stats.finished.fill_(1)
    t0 = 4242
    orc.step(st_o, W, clf, t0)
    ctx.rollout(st_d, dev(W).view(-1), dev(clf).view(-1), mask, t0, 0, stats, begin=True)
    torch.cuda.synchronize()
    assert_state_equal(st_d, st_o, keys=("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "qcache"), msg="BEGIN")
    assert int(stats.ep_return.abs().sum()) == 0 and int(stats.finished.sum()) == 0
    assert int(stats.vf_steps.sum()) == 0 and int(stats.episodes.sum()) == 0
    ent = (st_o["option_id"] > 0)
    dec = (st_o["option_id"] < 0)
    assert int(stats.entries.sum()) == int(ent.sum()) and int(stats.declines.sum()) == int(dec.sum())


def _counter_model(ctx, st, W, clf, mask, gest, t0, K):
    """Counters of SPEC §8 from the per-step outputs of K acting scg_step calls (st advanced in place)."""
    n, n_vf = ctx.n_envs, ctx.n_vf
    known = mask | gest
    parents = [int(p) for p in ctx.parents]
    rmask = max(ctx.cfg.reoffer_period, 1) - 1
    gid = ctx.cfg.env_id_base + np.arange(n, dtype=np.int64)
    c = {f: np.zeros((n_vf, n), np.int64) for f in ("vf_steps", "entries", "declines", "successes")}
    ep_ret = np.zeros(n, np.float32)
    ret_sum = np.zeros(n, np.float64)
    episodes, goals, len_sum = (np.zeros(n, np.int64) for _ in range(3))
    cols = np.arange(n)
    B = GpuBackend(ctx, W, clf, mask)                          # (its classifiers only: the loop is ctx.step's)
    for t in range(t0, t0 + K):
        before = host_state(st)
        entry = [getattr(st, f).clone() for f in ("x", "y", "vx", "vy")]
        ctx.step(st, W, clf, mask, t, learn=False)
        after = host_state(st)
        ctx.pinball_step(entry, st.action.clone())         # s' (before the reset) from the entry state and the action taken
        sx, sy = entry[0], entry[1]
        oid_b, oid_a = before["option_id"], after["option_id"]
        o = rules.vf_of(oid_b, n_vf)
        np.add.at(c["vf_steps"], (o, cols), 1)
        dn = after["done"]
        ent = (oid_a >= 1) & (after["opt_steps"] == 0)
        np.add.at(c["entries"], (np.maximum(oid_a, 0), cols), ent.astype(np.int64))
        stay = (dn == 0) & (oid_b == oid_a) & (((t + gid) & rmask) != 0)
        decl = (oid_a < 0) & ~stay
        np.add.at(c["declines"], (np.maximum(-oid_a, 0), cols), decl.astype(np.int64))
        goal = dn == 1
        end = rules.option_end(rules.membership(B.predict, sx.cpu().numpy(), sy.cpu().numpy(), n_vf, known), goal, dn, oid_b,
                               before["opt_steps"], parents, known, ctx.cfg.max_option_steps)
        np.add.at(c["successes"], (o, cols), (end["succ"] & (o >= 1)).astype(np.int64))
        r = ep_ret + after["reward"]
        rec = dn != 0
        episodes += rec; goals += goal; len_sum += np.where(rec, before["ep_steps"] + 1, 0)
        ret_sum = np.where(rec, ret_sum + r.astype(np.float64), ret_sum)
        ep_ret = np.where(rec, np.float32(0), r).astype(np.float32)
    return dict(c, ep_return=ep_ret, ret_sum=ret_sum, episodes=episodes, goals=goals, len_sum=len_sum)


@pytest.mark.parametrize("epw", [None, 32])
def test_counters_match_numpy_model(epw, monkeypatch):
    if epw:
        monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
    m = scg.load_map("pinball_simple")
    n, n_opt, mask, gest = 1000, 3, 0b1010, 0b0100
    ctx, W, clf = _setup(m, n, n_opt, None, [0, 0, 1, 1], gest, reoffer_period=4, epsilon=0.1, env_id_base=5)
    st = _state(ctx, m, n, n_opt, seed=21)
    twin = clone_state(st)
    stats = EpisodeStats(n_opt + 1, n, ctx.device)
    t0, K = 300, 40
    ctx.rollout(st, W, clf, mask, t0, 25, stats)               # two launches add up into one set of counters
    ctx.rollout(st, W, clf, mask, t0 + 25, K - 25, stats)
    model = _counter_model(ctx, twin, W, clf, mask, gest, t0, K)
    torch.cuda.synchronize()
    assert_same_bits(st, twin, msg="counter run")
    for f in ("vf_steps", "entries", "declines", "successes"):
        got = getattr(stats, f).cpu().numpy()
        assert np.array_equal(got, model[f]), f"{f}: {np.sum(got != model[f])} entries differ"
    for f in ("episodes", "goals", "len_sum"):
        assert np.array_equal(getattr(stats, f).cpu().numpy(), model[f]), f
    assert np.array_equal(stats.ep_return.cpu().numpy().view(np.uint32), model["ep_return"].view(np.uint32))
    assert np.array_equal(stats.ret_sum.cpu().numpy().view(np.uint64), model["ret_sum"].view(np.uint64))
    assert np.array_equal(stats.finished.cpu().numpy(), (model["episodes"] > 0).astype(np.uint8))
    assert model["entries"].sum() > 0 and model["declines"].sum() > 0 and model["successes"].sum() > 0
    assert model["episodes"].sum() > 0 and model["vf_steps"][1:].sum() > 0


@pytest.mark.parametrize("epw", [None, 32])
def test_one_episode(epw, monkeypatch):
    if epw:
        monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
    m = scg.load_map("pinball_simple")
    n, n_opt, mask, max_ep, spl = 1000, 2, 0b110, 30, 8
    ctx, W, clf = _setup(m, n, n_opt, None, max_episode_steps=max_ep, epsilon=0.1)
    st = _state(ctx, m, n, n_opt, seed=31)
    stats = EpisodeStats(n_opt + 1, n, ctx.device)
    launches = math.ceil(max_ep / spl)
    prev = None
    for i in range(launches):
        ctx.rollout(st, W, clf, mask, 0 if i == 0 else 1 + i * spl, spl, stats, begin=(i == 0), one_episode=True)
        cur = host_state(st)
        fin = stats.finished.cpu().numpy().astype(bool)
        if prev is not None:
            for f in EnvState.FIELDS:
                a, b = prev[0][f], cur[f]
                sel = prev[1]
                assert np.array_equal(a[..., sel].view(np.uint8), b[..., sel].view(np.uint8)), f"finished env's {f} changed"
        prev = (cur, fin)
    eps = stats.episodes.cpu().numpy()
    assert np.all(eps == 1), f"{np.sum(eps != 1)} envs did not record exactly one episode"
    assert np.all(stats.finished.cpu().numpy() == 1)
    lens = stats.len_sum.cpu().numpy()
    assert lens.min() >= 1 and lens.max() <= max_ep
    assert int(stats.vf_steps.sum()) == int(lens.sum())


def test_evaluate_leaves_training_alone():
    a, b = gestating_agent(), gestating_agent()
    for ag in (a, b):
        ag.ctx.set_trace_buffers(64)
    calls = []                                             # every call evaluate() makes on the TRAINING context

    def evaluate(**kw):
        with spy_calls(a.ctx, calls):
            return a.evaluate(**kw)

    for i in range(40):
        if i in (0, 17, 39):
            evaluate(n_episodes=1000, steps_per_launch=32)
        a.step_batch()
        b.step_batch()
    torch.cuda.synchronize()
    assert calls == [], f"evaluate() called into the training context: {calls}"      # (the peer exchange counter is its own)
    assert torch.equal(a.W, b.W), "evaluate() changed the training weights"
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(a.state, f), getattr(b.state, f)), f"evaluate() changed the training state ({f})"
    for x, y in zip(a.ctx._trace, b.ctx._trace):
        assert torch.equal(x, y), "evaluate() changed the trace buffers"
    assert torch.equal(a.gest_counts, b.gest_counts), "evaluate() changed the gestation success counts"
    assert int(a.gest_counts[2]) > 0, "the gestating option saw no success: the check above is vacuous"
    assert a.t == b.t == 40
    r1 = evaluate(n_episodes=1000, steps_per_launch=32)
    r2 = evaluate(n_episodes=1000, steps_per_launch=32)
    assert r1 == r2
    assert r1["episodes"] == 1000 and 0.0 <= r1["success_rate"] <= 1.0
    assert 1.0 <= r1["mean_length"] <= 100.0 and len(r1["entries"]) == 3
    assert abs(sum(r1["steps_share"]) - 1.0) < 1e-9
    s, per = a.evaluate(n_episodes=1000, steps_per_launch=32, per_env=True)
    assert s == r1 and int(per["episodes"].sum()) == 1000
    big = evaluate(n_episodes=20000, steps_per_launch=64)            # a larger launch geometry
    assert big["episodes"] == 20000
    for sd in (5, 6, 7):                                             # other seeds replace the cached context, not add to it
        assert evaluate(n_episodes=1000, seed=sd)["episodes"] == 1000
    assert sorted(a._eval_ctx) == [1000, 20000]
    assert calls == []
