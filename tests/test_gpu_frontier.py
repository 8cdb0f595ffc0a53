"""SPEC §13 on the GPU: scg_collect_frontier bit for bit against the numpy model on the oracle's trace, against the existing
goal collector, its refusals, and grow_skill_tree() end to end (a tree, a branch chain_skills cannot make)."""
import ctypes as C

import numpy as np
import pytest

import gpu_util
import sc_oracle
from frontier_model import collect_frontier_oracle
from gpu_util import assert_state_equal, dev, make_pair, state_to_device
from util import chain_classifiers, disc_weights, random_states, random_weights

pytestmark = pytest.mark.gpu


def _dev_bufs(n_vf, cap):
    import torch
    return (torch.zeros((n_vf, cap, 2), dtype=torch.float32, device="cuda:0"),
            torch.zeros((n_vf, cap), dtype=torch.uint8, device="cuda:0"),
            torch.zeros(n_vf, dtype=torch.int32, device="cuda:0"))


def _random_masks(rng, n_vf):
    """A cover of options 1..n_options (bit 0 never) and targets: the goal at will, options only from the cover."""
    cover = int(rng.integers(0, 1 << n_vf)) & ~1
    target = (int(rng.integers(0, 2)) | (int(rng.integers(0, 1 << n_vf)) & cover)) or 1
    return target, cover


def _frontier_rollout(n, steps, H, l_pos, l_neg, cap, seed):
    import torch
    nopt = 5
    enabled, gest, parents = 0b010110, 0b101000, [0, 0, 0, 1, 2, 3]      # 1, 2, 4 run; 3, 5 gestate; a tree
    ctx, orc, m = make_pair("pinball_simple", n, n_options=nopt, seed=seed, enabled_mask=enabled, max_episode_steps=40)
    ctx.set_option_parents(parents); orc.set_parents(parents)
    orc.set_gestation(gest); ctx.set_gestation(gest)
    orc.set_trace(H); ctx.set_trace_buffers(H)
    st_o = sc_oracle.new_state(n, m)
    x, y, vx, vy = random_states(m, n, seed + 1, vmax=1.5)
    st_o["x"][:], st_o["y"][:], st_o["vx"][:], st_o["vy"][:] = x, y, vx, vy
    W_o, clf = random_weights(nopt + 1, seed + 2, std=0.05), chain_classifiers(m, nopt)
    clf[4] = disc_weights(0.5, 0.5, 0.25)                              # a set away from the goal's neighbourhood
    st_d, W_d, clf_d = state_to_device(st_o, ctx), dev(W_o.copy()), dev(clf)
    xy_o, lab_o, cnt_o = np.zeros((nopt + 1, cap, 2), np.float32), np.zeros((nopt + 1, cap), np.uint8), np.zeros(nopt + 1, np.int32)
    xy_d, lab_d, cnt_d = _dev_bufs(nopt + 1, cap)
    rng = np.random.default_rng(seed + 3)
    for t in range(steps):
        G, n_k = orc.step(st_o, W_o, clf, t)
        orc.apply(W_o, G, n_k)
        ctx.step(st_d, W_d.view(-1), clf_d.view(-1), enabled, t)
        target, cover = _random_masks(rng, nopt + 1)
        collect_frontier_oracle(orc, target, cover, clf, l_pos, l_neg, xy_o, lab_o, cnt_o)
        ctx.collect_frontier(target, cover, clf_d.view(-1), l_pos, l_neg, xy_d.view(-1), lab_d.view(-1), cnt_d)
    torch.cuda.synchronize()
    assert_state_equal(st_d, st_o, msg="frontier rollout")
    ring_x, ring_y, events, ev_len = ctx._trace
    assert np.array_equal(events.cpu().numpy(), orc.events) and np.array_equal(ev_len.cpu().numpy(), orc.ev_len)
    assert np.array_equal(ring_x.cpu().numpy(), orc.ring_x) and np.array_equal(ring_y.cpu().numpy(), orc.ring_y)
    assert np.array_equal(cnt_d.cpu().numpy(), cnt_o), (cnt_d.cpu().numpy(), cnt_o)
    assert np.array_equal(xy_d.cpu().numpy(), xy_o) and np.array_equal(lab_d.cpu().numpy(), lab_o)
    return cnt_o


@pytest.mark.parametrize("block_envs", [256, 64])
def test_frontier_collect_bit_exact_against_the_model(block_envs):
    with gpu_util.block_build(block_envs):
        cnt = _frontier_rollout(4000, 30, 32, 12, 12, 30000, seed=50)             # roomy buffers
        assert cnt.min() > 0, cnt
        cnt = _frontier_rollout(2000, 16, 8, 6, 7, 150, seed=60)                  # ring_len 8 < L = 13; caps overflow
        assert (cnt == 150).sum() >= 2, cnt


def test_frontier_goal_node_equals_the_existing_goal_collector():
    """target 1 / cover 0: node 0's buffer is scg_collect_examples(1, prev_in)'s on the same context and steps. That trigger is
    announced to the step (its one-launch path): the row totals the step leaves must survive the frontier call in between."""
    import torch
    n, nopt, H, cap = 6000, 2, 32, 50000
    ctx, orc, m = make_pair("pinball_simple", n, n_options=nopt, seed=70, enabled_mask=0b110, max_episode_steps=40)
    ctx.set_trace_buffers(H)
    st_o = sc_oracle.new_state(n, m)
    x, y, vx, vy = random_states(m, n, 71, vmax=1.5)
    st_o["x"][:], st_o["y"][:], st_o["vx"][:], st_o["vy"][:] = x, y, vx, vy
    st_d, W_d = state_to_device(st_o, ctx), dev(random_weights(nopt + 1, 72, std=0.05))
    clf_d = dev(chain_classifiers(m, nopt))
    z = lambda dt: torch.zeros(cap, dtype=dt, device="cuda:0")
    ex = {True: (torch.zeros((cap, 2), device="cuda:0"), z(torch.uint8), torch.zeros(1, dtype=torch.int32, device="cuda:0"),
                 torch.zeros(n, dtype=torch.uint8, device="cuda:0"))}
    xy_f, lab_f, cnt_f = _dev_bufs(nopt + 1, cap)
    for t in range(25):
        ctx.step(st_d, W_d.view(-1), clf_d.view(-1), 0b110, t)
        ctx.collect_frontier(1, 0, clf_d.view(-1), 10, 9, xy_f.view(-1), lab_f.view(-1), cnt_f)
        for r, (xy, lab, cnt, prev) in ex.items():
            ctx.collect_examples(1, prev, 10, 9, xy.view(-1), lab, cnt, rearm=r)
    ctx.disarm_collect()
    torch.cuda.synchronize()
    k = int(cnt_f[0])
    assert k > 0 and cnt_f[1:].tolist() == [0, 0]
    for xy, lab, cnt, _ in ex.values():
        assert int(cnt.item()) == k
        assert torch.equal(xy[:k], xy_f[0, :k]) and torch.equal(lab[:k], lab_f[0, :k])


def test_frontier_refusals_launch_nothing():
    import torch
    n, nopt, cap = 512, 2, 64
    ctx, _, m = make_pair("pinball_simple", n, n_options=nopt, seed=80)
    xy, lab, cnt = _dev_bufs(nopt + 1, cap)
    clf = dev(chain_classifiers(m, nopt))
    xy.fill_(-3.0); lab.fill_(9); cnt.fill_(5)
    fn = ctx.lib.scg_collect_frontier
    P = lambda t: C.c_void_p(t.data_ptr())
    args = lambda tm, cm, lp=4, ln=4, cp=cap, c_=clf, x_=xy, l_=lab, n_=cnt: (
        ctx._ctx, C.c_uint32(tm), C.c_uint32(cm), None if c_ is None else P(c_), lp, ln, None if x_ is None else P(x_),
        None if l_ is None else P(l_), None if n_ is None else P(n_), cp, None)
    assert fn(*args(1, 0)) == -4                                  # SCG_ERR_STATE: no trace buffers
    ctx.set_trace_buffers(16)
    bad = [args(1 << 3, 0), args(1 << 8, 0), args(1, 0b001), args(1, 0b1000), args(0b010, 0b100), args(0b110, 0b010),
           args(1, 0, cp=0), args(1, 0, lp=-1), args(1, 0, ln=-1), args(1, 0, lp=0, ln=0), args(1, 0, c_=None),
           args(1, 0, x_=None), args(1, 0, l_=None), args(1, 0, n_=None),
           args(1, 0, lp=2 ** 31 - 1, ln=1), args(1, 0, lp=2 ** 30, ln=2 ** 30)]        # the sum is formed in 64 bits
    for a in bad:
        assert fn(*a) == -1, a                                    # SCG_ERR_INVALID
    from skill_chaining_with_graphs_amd import ScgError
    with pytest.raises(ScgError):
        ctx.collect_frontier(0b010, 0, clf.view(-1), 4, 4, xy.view(-1), lab.view(-1), cnt)
    torch.cuda.synchronize()
    assert bool((xy == -3.0).all()) and bool((lab == 9).all()) and cnt.tolist() == [5, 5, 5]
    assert fn(*args(0b011, 0b010)) == 0                           # valid: goal + set 1 with set 1 covered


def _grow_agent(n, nopt, seed, **kw):
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    agent = SkillChainingAgent("pinball_simple", n, nopt, seed=seed, epsilon=1.0, alpha=1e-4, max_episode_steps=400, **kw)
    agent.enable_tracing(64)
    agent.domain.reset_random(seed=seed + 1, v_max=0.5)
    return agent


def test_grow_skill_tree_end_to_end():
    import torch
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    agent = _grow_agent(8192, 3, seed=90)
    seen = {}
    fit_and_gestate = agent._fit_and_gestate

    def spy(k, *a):                                                  # the state at the decision, before the fit
        node_xy, node_lab, node_cnt = agent._frontier
        p = int(agent.ctx.parents[k])
        n = int(node_cnt[p])
        xy, lab = agent.examples(k)
        seen[k] = dict(parent=p, enabled=agent.enabled_mask, same=bool(torch.equal(xy, node_xy[p, :n]) and torch.equal(lab, node_lab[p, :n])))
        return fit_and_gestate(k, *a)

    agent._fit_and_gestate = spy
    report = agent.grow_skill_tree(steps_per_option=150, min_examples=2000, max_examples=20000, start_coverage=2.0)
    assert len(report) >= 2, report
    for r in report:
        k, p = r["option"], r["parent"]
        assert p < k and (p == 0 or (seen[k]["enabled"] >> p) & 1), r
        assert seen[k]["same"] and seen[k]["parent"] == p and r["examples"] == r["node_examples"][p] >= 2000, r
        assert (agent.enabled_mask >> k) & 1
    g = agent.skill_graph()
    import networkx as nx
    assert nx.is_tree(g.to_undirected()) and all(nx.has_path(g, k, 0) for k in g.nodes)
    stats = agent.evaluate(512)
    assert stats is not None
    d = agent.state_dict()
    other = SkillChainingAgent("pinball_simple", 8192, 3, seed=90, epsilon=1.0, alpha=1e-4, max_episode_steps=400)
    other.load_state_dict(d)
    assert list(other.ctx.parents) == list(agent.ctx.parents)
    for r in report:
        a, b = agent.examples(r["option"]), other.examples(r["option"])
        assert torch.equal(a[0].cpu(), b[0].cpu()) and torch.equal(a[1].cpu(), b[1].cpu())
    with pytest.raises(ValueError):
        _bad = SkillChainingAgent.__new__(SkillChainingAgent)
        _bad.group = object()
        _bad.grow_skill_tree()


def test_grow_skill_tree_branches_off_the_goal():
    """Option 1 covers one side of the goal only (a small disc to its left). Random exploration enters the goal from the
    uncovered sides far more often than set 1, so the grown option 2 targets the goal: a sibling of option 1, which
    chain_skills (2 -> 1 always) cannot make."""
    agent = _grow_agent(8192, 2, seed=95)
    tx, ty, r = agent.map.target
    agent.options[1].initiation_classifier.set_weights(disc_weights(tx - 0.05, ty, 0.015))
    agent.enable_option(1)
    report = agent.grow_skill_tree(steps_per_option=120, min_examples=1000, max_examples=40000, start_coverage=2.0)
    assert len(report) == 1, report
    r = report[0]
    assert r["option"] == 2 and r["node_examples"][0] > r["node_examples"][1], r
    assert r["parent"] == 0 and int(agent.ctx.parents[2]) == 0 and int(agent.ctx.parents[1]) == 0
    assert sorted(agent.skill_graph().edges()) == [(1, 0), (2, 0)]
