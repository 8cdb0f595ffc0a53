"""The reduce launch's slab sum (SPEC §5's two levels): G, n_k and W after two learning step-batches against the
CPU oracle, bit for bit, at the block counts where the sum's structure changes.

The 64-env block build keeps the shapes small: a wave of a slab workgroup sums one segment of 16 blocks, a round of the kernel is
32 segments, and wave 0 adds the round's 32 segment sums — every one of them, the empty ones' +0 rows too. The cases: 1, 15, 16,
17, 31, 32 and 33 blocks with the last block partial (n = 64 nblk - 5); 529 blocks (a second round of one segment, which holds one
block); an option whose envs all sit in one block of a middle segment (every other segment of its value function is empty, the
first one included); an option that nobody runs (n_k = 0, G all +0, W untouched); the 33-block case on the packed-operand path
(apply = 0: G and the float counts in one buffer, the update by scg_apply_update_packed); and overflowing weights, which put Inf
and NaN into the slabs.

`_block_counts` restates SPEC §5's env order on the host and counts every value function's update items per block (no option
gestates: an item of VF k >= 1 is an env running k, every env is an item of the root); each case asserts from those counts that
the structure it is named for occurred, and that they add up to the oracle's n_k. The reference of a case is computed once."""
import numpy as np
import pytest
import torch

import interrupt_learning_model as ilm
import option_rules as rules
from bits import assert_bits_equal
from gpu_util import block_build, dev, make_pair, state_to_device
from util import HP, chain_classifiers, copy_state, crossing_weights, entry_state, make_oracle, random_weights

pytestmark = pytest.mark.gpu

B, SEG, ROUND = 64, 16, 32         # envs per block, blocks per segment, segments per round of the kernel
STEPS = 2
NW1 = 5 * 1296


def _n(nblk):
    return B * nblk - 5


def _block_counts(option_id, n_vf):
    """[nblk][n_vf] update items per block and value function, for the option ids at entry."""
    oid = np.asarray(option_id, np.int64)
    perm = rules.env_order(oid, n_vf, B)
    o = rules.vf_of(oid, n_vf)[perm]
    nblk = -(-len(o) // B)
    cnt = np.zeros((nblk, n_vf), np.int64)
    for b in range(nblk):
        ob = o[b * B:(b + 1) * B]
        cnt[b, 0] = len(ob)
        for k in range(1, n_vf):
            cnt[b, k] = int((ob == k).sum())
    return cnt


def _segments(cnt_k):
    """Which segments of one value function hold a slab."""
    return [bool((cnt_k[s:s + SEG] > 0).any()) for s in range(0, len(cnt_k), SEG)]


def _mixed_ids(n, n_opt, seed):
    def make(m):
        return entry_state(m, n, n_opt, seed, 0.4, HP["max_episode_steps"])
    return make


def _seated_ids(n, n_opt, seed, runs):
    """`runs` = {option: envs running it}; every other env runs none. Env ids are shuffled over the seats."""
    def make(m):
        st = entry_state(m, n, n_opt, seed, 0.0, HP["max_episode_steps"])
        envs = np.random.default_rng(seed).permutation(n)
        st["option_id"][:] = 0
        lo = 0
        for k, c in runs.items():
            st["option_id"][envs[lo:lo + c]] = k
            lo += c
        return st
    return make


# name -> (n, n_options, enabled mask, entry state, weights)
def _weights(n_vf, seed):
    return lambda: crossing_weights(n_vf, seed)


def _overflow_weights():
    """tests/test_gpu_edges.py's overflow: option 1's weights at 2^125, Inf and 3e38 entries in option 2's."""
    W = random_weights(3, 2, std=1.0)
    W[1] = (W[1].astype(np.float64) * 2.0 ** 125).astype(np.float32)
    W[2, 0, 5], W[2, 1, 7], W[2, 2, 9] = np.float32(3e38), np.inf, -np.inf
    return W


CASES = {f"blocks{b}": (_n(b), 2, 0b110, _mixed_ids(_n(b), 2, 30 + b), _weights(3, 30 + b)) for b in (1, 15, 16, 17, 31, 32, 33)}
CASES["blocks529"] = (_n(529), 2, 0b110, _mixed_ids(_n(529), 2, 41), _weights(3, 41))
# options 1 and 3 run in about 38 blocks each (the chunked layout spreads them), option 2's ten envs are one chunk between the two
CASES["one_block"] = (_n(80), 3, 0b1110, _seated_ids(_n(80), 3, 42, {1: 1000, 2: 10, 3: 1000}), _weights(4, 42))
CASES["nobody"] = (_n(33), 2, 0b010, _seated_ids(_n(33), 2, 43, {1: 700}), _weights(3, 43))
CASES["overflow"] = (_n(33), 2, 0b110, _seated_ids(_n(33), 2, 44, {1: 300, 2: 1000}), _overflow_weights)      # option 2: blocks in two segments

_REF = {}


def _reference(case):
    """Two learning step-batches on the oracle: the entry state, the weights, the classifiers and per step (G, n_k, W after the
    apply, per-block counts at entry). Computed once per case; nothing hands out a view that a test writes to."""
    if case not in _REF:
        n, n_opt, enabled, make_state, make_w = CASES[case]
        with block_build(B):
            orc, m = make_oracle("pinball_simple", n, n_options=n_opt, seed=7, enabled_mask=enabled, n_threads=8)
            st0 = make_state(m)
            W, clf = make_w(), chain_classifiers(m, n_opt)
            st, steps = copy_state(st0), []
            for t in range(STEPS):
                cnt = _block_counts(st["option_id"], n_opt + 1)
                with np.errstate(all="ignore"):
                    G, n_k = orc.step(st, W, clf, 20 + t)
                    W_next = ilm.apply(orc, W, G, n_k)
                assert np.array_equal(cnt.sum(0), n_k), (case, t, cnt.sum(0), n_k)
                steps.append((G, n_k, W_next, cnt))
                W = W_next
        _REF[case] = (st0, make_w(), clf, steps)
    return _REF[case]


def _run(case, packed=False, free_nan=False):
    """The case on the device, step by step against the reference by bits; returns the per-step reference for the structure checks."""
    n, n_opt, enabled, _, _ = CASES[case]
    st0, W0, clf, steps = _reference(case)
    NW = (n_opt + 1) * NW1
    with block_build(B):
        ctx, orc, m = make_pair("pinball_simple", n, n_options=n_opt, seed=7, enabled_mask=enabled)
        st = state_to_device(st0, ctx)
        W_d, clf_d = dev(W0.copy()).view(-1), dev(clf).view(-1)
        if packed:
            gp = ctx.grad_packed()
        else:
            G_d, nk_d = ctx.grad_buffers()
        for t, (G, n_k, W_next, _) in enumerate(steps):
            ctx.step(st, W_d, clf_d, enabled, 20 + t, learn=True, apply=not packed)
            if packed:
                flat = gp.cpu().numpy()
                got_G, got_nk = flat[:NW].reshape(G.shape), flat[NW:]
                assert_bits_equal(got_nk, n_k.astype(np.float32), msg=f"{case} step {t} nk_f:")
                ctx.apply_update_packed(W_d, gp)
            else:
                torch.cuda.synchronize()
                got_G, got_nk = G_d.cpu().numpy(), nk_d.cpu().numpy()
                assert np.array_equal(got_nk, n_k), (case, t, got_nk, n_k)
            assert_bits_equal(got_G, G, allow_nan=free_nan, msg=f"{case} step {t} G:")
            assert_bits_equal(W_d.cpu().numpy().reshape(W_next.shape), W_next, allow_nan=free_nan, msg=f"{case} step {t} W:")
        assert ctx.async_status(synchronize=True) == 0
        ctx.close()
    return steps


def _check_blocks(steps, nblk):
    """nblk blocks, the last one partial; the root holds a slab in every block, the options in some blocks and (from 2 blocks on) not in others."""
    for G, n_k, W, cnt in steps:
        assert len(cnt) == nblk and cnt[-1, 0] == B - 5 and (cnt[:-1, 0] == B).all(), cnt[:, 0]
        assert _segments(cnt[:, 0]) == [True] * (-(-nblk // SEG))
    n_k, cnt = steps[0][1], steps[0][3]
    assert (cnt[:, 1:] > 0).any() and (n_k[1:] > 0).any(), cnt
    if nblk >= 2:
        assert (cnt[:, 1:] == 0).any(), cnt


@pytest.mark.parametrize("nblk", [1, 15, 16, 17, 31, 32, 33])
def test_block_counts_round_the_segment_and_the_round(nblk):
    """One block; a segment one block short, full, one block over; a round one block short, full, one block over."""
    _check_blocks(_run(f"blocks{nblk}"), nblk)


def test_second_round_with_a_partial_last_segment():
    """529 blocks = 34 segments: the kernel's loop over rounds runs twice, the second round holds two segments, the last of one block."""
    steps = _run("blocks529")
    _check_blocks(steps, 529)
    nseg = -(-529 // SEG)
    assert nseg == ROUND + 2 and 529 - SEG * (nseg - 1) == 1
    cnt = steps[0][3]                                          # the options come first in the env order: option 2's run reaches into the second
    assert any(_segments(cnt[:, 2])[ROUND:]) and not all(_segments(cnt[:, 2])), _segments(cnt[:, 2])      # round, behind empty segments


def test_option_in_one_block_of_a_middle_segment():
    """Option 2's envs all sit in one block; its segment lies in the middle: the first segment is empty, whole segments before and behind it are."""
    steps = _run("one_block")
    cnt2 = steps[0][3][:, 2]
    blocks = np.nonzero(cnt2)[0]
    seg = _segments(cnt2)
    assert len(blocks) == 1 and cnt2[blocks[0]] == 10 and len(seg) == 5, (blocks, seg)
    s = int(blocks[0]) // SEG
    assert 2 <= s <= len(seg) - 2 and seg == [i == s for i in range(len(seg))], (s, seg)       # two empty segments before it, one or more behind
    assert steps[0][1][2] == 10


def test_option_that_nobody_runs():
    """Option 2 is disabled and nobody runs it: no block holds a slab of its value function. n_k = 0, G all +0, W untouched."""
    steps = _run("nobody")
    _, W0, _, _ = _reference("nobody")
    for G, n_k, W, cnt in steps:
        assert (cnt[:, 2] == 0).all() and n_k[2] == 0 and n_k[1] > 0
        assert not G[2].view(np.uint32).any()                   # +0 everywhere (a -0 would show)
        assert np.array_equal(W[2].view(np.uint32), W0[2].view(np.uint32))
        assert not np.array_equal(W[1], W0[1])


@pytest.mark.parametrize("packed", [False, True], ids=["apply", "packed"])
def test_33_blocks_on_both_apply_paths(packed):
    """A round one block over, with the update inside the reduce launch and on the packed-operand path (apply = 0): G and the float
    counts land behind one another in the caller's operand, scg_apply_update_packed makes the same W."""
    _check_blocks(_run("blocks33", packed=packed), 33)


def test_inf_and_nan_in_the_slabs():
    """Overflowing weights: the slabs hold Inf and NaN, and the sum that adds every segment's row carries them as the oracle's does."""
    steps = _run("overflow", free_nan=True)
    _check_blocks(steps, 33)
    G, cnt = steps[0][0], steps[0][3]
    assert np.isnan(G[1]).any() and np.isinf(G[2]).any() and np.isnan(G[2]).any(), "no Inf / no NaN in G: the case tests less than it should"
    assert sum(_segments(cnt[:, 2])) >= 2, _segments(cnt[:, 2])       # option 2's Inf and NaN pass through both levels of the sum
