"""The commit rows of the reduce launch (SPEC §4.2, §5, §7): what a step leaves in the caller's arrays, and the next
step's env order, against the CPU oracle bit for bit on the 64-env block build.

A commit wave owns 64 consecutive envs. It reads each env's result line and, for every env, the two words of the root's
Q(s', .) beside it (`qalt`), and keeps the latter only where the line carries the declined mark. The cases:
  reoffer_period = 1 on three blocks with the chain classifiers and option weights that cross the root's both ways: one wave
  holds envs that decline an option, envs that enter one and envs that stay with the root, over four learning step-batches;
  the same run with no option enabled: nothing ever writes qalt, and what the waves read there must not show;
  one acting-only step (the commit without a reduce launch);
  an announced example trigger: the commit rows leave the per-row example totals that the collector's own count launch would.
The env order is internal to the library; it is held through the sums: G of a step is added in the order the step before it
left (SPEC §5), so a misplaced env changes bits of G one step later. Every output array, qcache included, is compared after
every step. The reference of a case is computed once."""
import numpy as np
import pytest
import torch

import interrupt_learning_model as ilm
from bits import assert_bits_equal
from gpu_util import assert_state_equal, block_build, dev, make_pair, state_to_device
from util import HP, chain_classifiers, copy_state, crossing_weights, entry_state, make_oracle

pytestmark = pytest.mark.gpu

B = 64
N = 3 * B - 5                      # three blocks, the last one partial: one row of 256 envs, its last wave partial
STEPS = 4
# name -> (enabled mask, share of the envs that run an option at entry)
CASES = {"reoffer_every_step": (0b110, 0.3), "no_option_enabled": (0b000, 0.0)}
_REF = {}


def _reference(case):
    """Four learning step-batches on the oracle: entry state, weights, classifiers and per step (option ids at entry, G, n_k, W
    after the apply, state after the step)."""
    if case not in _REF:
        enabled, share = CASES[case]
        with block_build(B):
            orc, m = make_oracle("pinball_simple", N, n_options=2, seed=11, enabled_mask=enabled, n_threads=4, reoffer_period=1)
            st0 = entry_state(m, N, 2, 72, share, HP["max_episode_steps"])
            W0, clf = crossing_weights(3, 72), chain_classifiers(m, 2)
            st, W, steps = copy_state(st0), W0.copy(), []
            for t in range(STEPS):
                before = st["option_id"].copy()
                G, n_k = orc.step(st, W, clf, 40 + t)
                W_next = ilm.apply(orc, W, G, n_k)
                steps.append((before, G, n_k, W_next, copy_state(st)))
                W = W_next
        _REF[case] = (st0, W0, clf, steps)
    return _REF[case]


def _run(case, learn_steps=STEPS):
    enabled, _ = CASES[case]
    st0, W0, clf, steps = _reference(case)
    with block_build(B):
        ctx, orc, m = make_pair("pinball_simple", N, n_options=2, seed=11, enabled_mask=enabled, reoffer_period=1)
        st = state_to_device(st0, ctx)
        W_d, clf_d = dev(W0.copy()).view(-1), dev(clf).view(-1)
        G_d, nk_d = ctx.grad_buffers()
        for t, (_, G, n_k, W_next, st_next) in enumerate(steps[:learn_steps]):
            ctx.step(st, W_d, clf_d, enabled, 40 + t, learn=True, apply=True)
            torch.cuda.synchronize()
            assert_state_equal(st, st_next, msg=f"{case} step {t}")
            assert np.array_equal(nk_d.cpu().numpy(), n_k), (case, t)
            assert_bits_equal(G_d.cpu().numpy(), G, msg=f"{case} step {t} G:")
            assert_bits_equal(W_d.cpu().numpy().reshape(W_next.shape), W_next, msg=f"{case} step {t} W:")
        assert ctx.async_status(synchronize=True) == 0
        ctx.close()
    return steps


def test_declined_entering_and_root_envs_in_one_wave():
    """Every env in an initiation set is offered its option in every step: one commit wave (64 consecutive envs) holds envs that
    decline (option_id -k), envs that enter (k from none) and envs that stay with the root, in one step."""
    steps = _run("reoffer_every_step")
    mixed = []
    for before, G, n_k, W, st in steps:
        after = st["option_id"]
        for w in range(-(-N // 64)):
            b, a = before[64 * w:64 * w + 64], after[64 * w:64 * w + 64]
            mixed.append(bool((a < 0).any() and ((a > 0) & (b <= 0)).any() and ((a == 0) & (b == 0)).any()))
    assert any(mixed), "no wave with declined, entering and root envs together: the case tests less than it should"
    assert sum(int((st["option_id"] < 0).sum()) for *_, st in steps) >= 8


def test_no_option_enabled_leaves_the_alternative_values_unwritten():
    """No option is enabled: no env is offered one, nothing writes the root's alternative Q values, and every env's qcache is its
    result line's."""
    steps = _run("no_option_enabled")
    for before, G, n_k, W, st in steps:
        assert (st["option_id"] <= 0).all() and n_k[1] == 0 and n_k[2] == 0


def test_acting_only_step_commits_the_same_state():
    """learn=False: the commit runs alone, without a reduce launch, and leaves the state the oracle's step leaves."""
    enabled, _ = CASES["reoffer_every_step"]
    st0, W0, clf, steps = _reference("reoffer_every_step")
    with block_build(B):
        ctx, orc, m = make_pair("pinball_simple", N, n_options=2, seed=11, enabled_mask=enabled, reoffer_period=1)
        st = state_to_device(st0, ctx)
        W_d, clf_d = dev(W0.copy()).view(-1), dev(clf).view(-1)
        ctx.step(st, W_d, clf_d, enabled, 40, learn=False)
        torch.cuda.synchronize()
        assert_state_equal(st, steps[0][4], msg="acting step")
        assert_bits_equal(W_d.cpu().numpy().reshape(W0.shape), W0, msg="acting step W:")
        assert ctx.async_status(synchronize=True) == 0
        ctx.close()


def test_announced_trigger_rows_equal_the_count_launch():
    """An announced trigger (the commit rows count the examples per row of 256 envs) against the collector counting for itself:
    two agents on the same seed hold identical example buffers, counts and prev_in after every collect, over three rows of
    envs, the last one partial."""
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    n, ags = 9 * B - 5, []
    for _ in range(2):
        ag = SkillChainingAgent("pinball_simple", n, 2, seed=9, block_envs=B, reoffer_period=1, **dict(HP, max_episode_steps=60))
        ag.clf.copy_(torch.as_tensor(chain_classifiers(ag.map, 2), device="cuda:0"))
        ag.enable_option(1)
        ag.init_weights(std=1e-2)
        ag.domain.reset_random(seed=4, v_max=1.5)
        ag.enable_tracing(ring_len=32, max_examples=1 << 14)
        ags.append(ag)
    a, b = ags
    for t in range(16):
        for ag in ags:
            ag.step_batch()
        xy, lab, cnt, prev = a._ex_buffers(2)
        a.ctx.collect_examples(1 << 1, prev, 8, 8, xy.view(-1), lab, cnt, rearm=True)
        xy, lab, cnt, prev = b._ex_buffers(2)
        b.ctx.collect_examples(1 << 1, prev, 8, 8, xy.view(-1), lab, cnt, rearm=False)
    torch.cuda.synchronize()
    na, nb = a.examples_held(2), b.examples_held(2)
    assert na == nb and na > 20, (na, nb)
    for ta, tb in zip(a._ex_buffers(2), b._ex_buffers(2)):
        assert torch.equal(ta, tb)
    for f in SkillChainingAgent._STATE_FIELDS:
        assert torch.equal(getattr(a.state, f), getattr(b.state, f)), f
