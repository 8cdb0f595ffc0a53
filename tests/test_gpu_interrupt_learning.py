"""SPEC §12 interrupting learner on the GPU: scg_step(LEARN | INTERRUPT) acts like one scg_rollout_interrupt step (every block
build), its G, n_k, W and env arrays equal the oracle-built emulator of tests/interrupt_learning_model.py bit for bit (both env
order layouts, several step-batches with APPLY), nothing changes when nothing can be interrupted, the folded next order equals a
fresh sort, INTERRUPT without LEARN is refused, and the agent's interrupt_learning switch."""
import numpy as np
import pytest
import torch

import interrupt_learning_model as ilm
from gpu_util import (as_bytes, assert_same_bits, block_build, clone_state, crossing_agent, dev, make_pair, set_block_envs,
                      spy_calls, state_to_device)
from ref64 import env_order_layout
from skill_chaining_with_graphs_amd import ScgError
from skill_chaining_with_graphs_amd.core import EnvState
from util import HP, crossing_weights, entry_state, wide_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_block():
    with block_build(None):             # _setup picks each test's build; the default is back after the test
        yield


def _setup(name, n, n_opt, block=None, seed=3, run_share=0.4, gest=0, same_w=False):
    set_block_envs(block)
    n_vf = n_opt + 1
    mask = ((1 << n_vf) - 1) & ~1 & ~gest
    ctx, orc, m = make_pair(name, n, n_options=n_opt, seed=seed, enabled_mask=mask, reoffer_period=4)
    if gest:
        ctx.set_gestation(gest)
        orc.set_gestation(gest)
    st = entry_state(m, n, n_opt, seed, run_share, HP["max_episode_steps"])
    W = crossing_weights(n_vf, seed)
    if same_w:
        W[1:] = W[0]
    return ctx, orc, m, st, W, wide_chain(m, n_opt), mask


@pytest.mark.parametrize("block", [64, 128, 256])
def test_acting_outputs_equal_one_interrupting_rollout_step(block):
    n, n_opt = 3000, 5
    ctx, orc, m, st_h, W_h, clf_h, mask = _setup("pinball_simple", n, n_opt, block=block, seed=5)
    st = state_to_device(st_h, ctx)
    W, clf = dev(W_h).view(-1), dev(clf_h).view(-1)
    intr = torch.zeros((n_opt + 1, n), dtype=torch.int32, device=ctx.device)
    for t in range(100, 106):
        twin, W_before = clone_state(st), W.clone()
        ctx.step(st, W, clf, mask, t, learn=True, apply=True, interrupt=True)
        ctx.rollout(twin, W_before, clf, mask, t, 1, interrupt=True, interrupts=intr)
        torch.cuda.synchronize()
        assert_same_bits(st, twin, msg=f"block {block} t {t}")
        assert not torch.equal(W, W_before)
    assert int(intr.sum()) >= 100, f"only {int(intr.sum())} interrupts"


CASES = [
    # map, envs, options, block, seed, share of envs running an option, gestating, layout
    ("pinball_simple", 4096, 5, 256, 1, 0.35, 0, "chunked"),
    ("pinball_simple", 1000, 5, 256, 2, 0.6, 0, "padded"),
    ("pinball_maze", 1536, 4, 128, 3, 0.5, 0b10000, "chunked"),
    ("pinball_maze", 300, 5, 64, 4, 0.9, 0, "padded"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-n{c[1]}-b{c[3]}-{c[7]}")
def test_G_and_counts_equal_the_emulator(case):
    name, n, n_opt, block, seed, share, gest, layout = case
    ctx, orc, m, st_h, W_h, clf_h, mask = _setup(name, n, n_opt, block=block, seed=seed, run_share=share, gest=gest)
    assert env_order_layout(st_h["option_id"], n_opt + 1, block) == layout
    st = state_to_device(st_h, ctx)
    G_d, n_d = ctx.grad_buffers()
    W = dev(W_h).view(-1)
    ctx.step(st, W, dev(clf_h).view(-1), mask, 21, learn=True, apply=False, interrupt=True)
    post, G, n_k, info = ilm.step(orc, st_h, W_h, clf_h, 21, mask, gest=gest)
    torch.cuda.synchronize()
    assert info["interrupted"].sum() >= 5, int(info["interrupted"].sum())
    assert_same_bits(st, post, msg=name)
    assert np.array_equal(n_d.cpu().numpy(), n_k)
    Gd = G_d.cpu().numpy()
    for k in range(n_opt + 1):
        assert np.array_equal(Gd[k], G[k]), f"VF {k}: {np.sum(Gd[k] != G[k])} elements differ"
    assert np.array_equal(W.cpu().numpy().reshape(W_h.shape), W_h)          # no APPLY


def test_eight_learning_steps_equal_the_emulator():
    n, n_opt = 2048, 4
    ctx, orc, m, st_h, W_h, clf_h, mask = _setup("pinball_simple", n, n_opt, seed=8, run_share=0.4)
    st, W, clf = state_to_device(st_h, ctx), dev(W_h).view(-1), dev(clf_h).view(-1)
    cuts = 0
    for t in range(40, 48):
        ctx.step(st, W, clf, mask, t, learn=True, apply=True, interrupt=True)
        st_h, G, n_k, info = ilm.step(orc, st_h, W_h, clf_h, t, mask)
        W_h = ilm.apply(orc, W_h, G, n_k)
        cuts += int(info["interrupted"].sum())
        torch.cuda.synchronize()
        assert_same_bits(st, st_h, msg=f"t {t}")
        assert np.array_equal(as_bytes(W), as_bytes(W_h.reshape(-1))), f"t {t}: W differs"
    assert cuts >= 40, cuts


def test_nothing_to_interrupt_is_the_plain_step():
    """With every W_k == W_0 no option is interrupted (ties keep it): G, n_k, W after APPLY, the env arrays and the prepared next
    order (a second, plain step on both contexts) equal scg_step(LEARN)'s."""
    n, n_opt = 4096, 5
    out = []
    for intr in (False, True):
        ctx, orc, m, st_h, W_h, clf_h, mask = _setup("pinball_simple", n, n_opt, seed=6, same_w=True)
        st, W, clf = state_to_device(st_h, ctx), dev(W_h).view(-1), dev(clf_h).view(-1)
        G_d, n_d = ctx.grad_buffers()
        ctx.step(st, W, clf, mask, 9, learn=True, apply=True, interrupt=intr)
        first = (clone_state(st), W.clone(), G_d.clone(), n_d.clone())
        ctx.step(st, W, clf, mask, 10, learn=True, apply=True)
        torch.cuda.synchronize()
        out.append((first, (clone_state(st), W.clone(), G_d.clone(), n_d.clone())))
    for (a, b), what in zip(zip(out[0], out[1]), ("first step", "second step")):
        assert_same_bits(a[0], b[0], msg=what)
        for x, y, name in zip(a[1:], b[1:], ("W", "G", "n_k")):
            assert np.array_equal(as_bytes(x), as_bytes(y)), f"{what}: {name} differs"
    assert int((out[0][0][0].option_id > 0).sum()) > 500


def test_folded_next_order_equals_a_fresh_sort():
    n, n_opt = 4096, 5
    res = []
    for fresh in (False, True):
        ctx, orc, m, st_h, W_h, clf_h, mask = _setup("pinball_maze", n, n_opt, seed=12)
        st, W, clf = state_to_device(st_h, ctx), dev(W_h).view(-1), dev(clf_h).view(-1)
        G_d, n_d = ctx.grad_buffers()
        intr = torch.zeros((n_opt + 1, n), dtype=torch.int32, device=ctx.device)
        twin = clone_state(st)
        ctx.rollout(twin, W, clf, mask, 30, 1, interrupt=True, interrupts=intr)
        ctx.step(st, W, clf, mask, 30, learn=True, apply=True, interrupt=True)
        if fresh:
            ctx.invalidate_order()
        ctx.step(st, W, clf, mask, 31, learn=True, apply=True, interrupt=True)
        torch.cuda.synchronize()
        assert int(intr.sum()) > 50
        res.append((clone_state(st), W.clone(), G_d.clone(), n_d.clone()))
    assert_same_bits(res[0][0], res[1][0], msg="after the folded order")
    for x, y, name in zip(res[0][1:], res[1][1:], ("W", "G", "n_k")):
        assert np.array_equal(as_bytes(x), as_bytes(y)), f"{name} differs"


def test_interrupt_without_learn_is_refused():
    n, n_opt = 1024, 3
    ctx, orc, m, st_h, W_h, clf_h, mask = _setup("pinball_simple", n, n_opt, seed=2)
    st, W, clf = state_to_device(st_h, ctx), dev(W_h).view(-1), dev(clf_h).view(-1)
    G_d, n_d = ctx.grad_buffers()
    G_d.fill_(7.0)
    before = (clone_state(st), W.clone(), G_d.clone(), n_d.clone())
    with pytest.raises(ScgError, match="SCG_STEP_INTERRUPT without SCG_STEP_LEARN"):
        ctx.step(st, W, clf, mask, 3, learn=False, interrupt=True)
    torch.cuda.synchronize()
    assert_same_bits(st, before[0], msg="refused step")
    for x, y, name in zip((W, G_d, n_d), before[1:], ("W", "G", "n_k")):
        assert torch.equal(x, y), name
    ctx.step(st, W, clf, mask, 3, learn=False)                              # the context is fine afterwards
    torch.cuda.synchronize()


def test_agent_interrupt_learning():
    plain, default, intr = crossing_agent(interrupt_learning=False), crossing_agent(), crossing_agent(interrupt_learning=True)
    assert default.interrupt_learning is False and intr.interrupt_learning is True
    with spy_calls(default.ctx) as (_, default_steps), spy_calls(intr.ctx) as (_, intr_steps):
        for a in (plain, default, intr):
            a.rollout(6)
            a.step_batch(learn=False)
    torch.cuda.synchronize()
    assert default_steps == [(True, False)] * 6 + [(False, False)]
    assert intr_steps == [(True, True)] * 6 + [(False, False)]             # acting-only steps never interrupt
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(plain.state, f), getattr(default.state, f)), f
    assert torch.equal(plain.W, default.W)
    assert not torch.equal(intr.W, default.W)
    assert not torch.equal(intr.state.opt_steps, default.state.opt_steps)
    sd = intr.state_dict()
    assert not any("interrupt" in k for k in sd)                           # a setting, like the hyper-parameters


def test_chain_skills_with_interrupt_learning():
    """The outer loop (tests/test_outer_loop.py's set-up) with an interrupting learner: every learning step-batch interrupts,
    options are created, and the weights stay finite."""
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    ag = SkillChainingAgent("pinball_empty", 8192, 3, seed=5, epsilon=1.0, alpha=1e-4, max_episode_steps=400,
                            interrupt_learning=True)
    ag.enable_tracing(64)
    ag.domain.reset_random(seed=11, v_max=0.5)
    with spy_calls(ag.ctx) as (_, calls):
        rep = ag.chain_skills(steps_per_option=250, min_examples=2000, max_examples=20000, start_coverage=2.0)
        ag.rollout(50)
    torch.cuda.synchronize()
    assert len(rep) >= 1 and ag.enabled_mask != 0, rep
    assert calls and all(c == (True, True) for c in calls)
    assert bool(torch.isfinite(ag.W).all())
