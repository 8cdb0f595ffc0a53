"""The reduce launch's slab sum where its lane groups change (SPEC §5's two levels): G, n_k, W and the committed
state after two learning step-batches against the CPU oracle, bit for bit.

A slab workgroup owns 16 float4 columns; a wave of it is four lane groups, each of which sums one segment of 16 blocks per pass,
so a wave covers 64 blocks, the workgroup's four waves 16 segments (a pass), and a round is two passes. With the 64-env block
build the block counts stay small. The cases (n = 64 nblk - 5, the last block partial):
  47, 48, 49     the third lane group's segment one block short, full, and the fourth group's first block;
  63, 64, 65     a wave's last group one block short, full, and the next wave's first block;
  127, 128, 129  the same at the second wave's end;
  255, 256, 257  a pass one block short, full, and the first block of the groups' second segments;
  an option whose envs all sit in one block of a wave's SECOND lane group (its first group's segment holds nothing of it, nor
  does any other segment): the wave issues a slab load that only one of its groups executes;
  Inf and NaN in the slabs at 65 blocks (two waves);
  320 blocks with five options: on a device of 256 compute units this launch is past the size up to which the sixteen-load
  form of the kernel is used, so it runs the eight-load form (two batches per segment), as the headline workload does.
tests/test_gpu_reduce_sum.py holds 1..33 and 529 blocks (the round's edge) on the same rig; its host-side block counts and case
builders are used here. Each case asserts from those counts that the structure it is named for occurred; the reference of a case
is computed once."""
import numpy as np
import pytest
import torch

import interrupt_learning_model as ilm
import test_gpu_reduce_sum as rs
from bits import assert_bits_equal
from gpu_util import assert_state_equal, block_build, dev, make_pair, state_to_device
from util import chain_classifiers, copy_state, make_oracle

pytestmark = pytest.mark.gpu

B, SEG = rs.B, rs.SEG
GROUPS_PER_WAVE, WAVES = 4, 4          # lane groups per wave, waves per slab workgroup: 16 segments per pass, two passes per round
STEPS = 2
EDGES = (47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257)

# name -> (n, n_options, enabled mask, entry state, weights)
CASES = {f"blocks{b}": (rs._n(b), 2, 0b110, rs._mixed_ids(rs._n(b), 2, 60 + b), rs._weights(3, 60 + b)) for b in EDGES}
# option 2's ten envs are one chunk behind option 1's run of 23 blocks: block 23, the second segment
CASES["second_group"] = (rs._n(80), 3, 0b1110, rs._seated_ids(rs._n(80), 3, 52, {1: 600, 2: 10, 3: 1400}), rs._weights(4, 52))
CASES["overflow65"] = (rs._n(65), 2, 0b110, rs._seated_ids(rs._n(65), 2, 54, {1: 600, 2: 2200}), rs._overflow_weights)
CASES["blocks320_five_options"] = (rs._n(320), 5, 0b111110, rs._mixed_ids(rs._n(320), 5, 55), rs._weights(6, 55))

_REF = {}


def _reference(case):
    """Two learning step-batches on the oracle: entry state, weights, classifiers and per step (G, n_k, W after the apply, the
    per-block counts at entry, the state after the step). Computed once per case; the tests only read it."""
    if case not in _REF:
        n, n_opt, enabled, make_state, make_w = CASES[case]
        with block_build(B):
            orc, m = make_oracle("pinball_simple", n, n_options=n_opt, seed=7, enabled_mask=enabled, n_threads=8)
            st0 = make_state(m)
            W, clf = make_w(), chain_classifiers(m, n_opt)
            st, steps = copy_state(st0), []
            for t in range(STEPS):
                cnt = rs._block_counts(st["option_id"], n_opt + 1)
                with np.errstate(all="ignore"):
                    G, n_k = orc.step(st, W, clf, 20 + t)
                    W_next = ilm.apply(orc, W, G, n_k)
                assert np.array_equal(cnt.sum(0), n_k), (case, t, cnt.sum(0), n_k)
                steps.append((G, n_k, W_next, cnt, copy_state(st)))
                W = W_next
        _REF[case] = (st0, make_w(), clf, steps)
    return _REF[case]


def _run(case, free_nan=False):
    """The case on the device, step by step against the reference by bits; returns the per-step reference for the structure checks."""
    n, n_opt, enabled, _, _ = CASES[case]
    st0, W0, clf, steps = _reference(case)
    with block_build(B):
        ctx, orc, m = make_pair("pinball_simple", n, n_options=n_opt, seed=7, enabled_mask=enabled)
        st = state_to_device(st0, ctx)
        W_d, clf_d = dev(W0.copy()).view(-1), dev(clf).view(-1)
        G_d, nk_d = ctx.grad_buffers()
        for t, (G, n_k, W_next, _, st_next) in enumerate(steps):
            ctx.step(st, W_d, clf_d, enabled, 20 + t, learn=True, apply=True)
            torch.cuda.synchronize()
            got_nk = nk_d.cpu().numpy()
            assert np.array_equal(got_nk, n_k), (case, t, got_nk, n_k)
            assert_bits_equal(G_d.cpu().numpy(), G, allow_nan=free_nan, msg=f"{case} step {t} G:")
            assert_bits_equal(W_d.cpu().numpy().reshape(W_next.shape), W_next, allow_nan=free_nan, msg=f"{case} step {t} W:")
            if not free_nan:                                        # (the committed state: a NaN's payload is free where the weights overflow)
                assert_state_equal(st, st_next, msg=f"{case} step {t}")
        assert ctx.async_status(synchronize=True) == 0
        ctx.close()
    return steps


def _place(seg):
    """(pass, wave, lane group) of a segment of the first round."""
    assert seg < 2 * WAVES * GROUPS_PER_WAVE
    g = seg % (WAVES * GROUPS_PER_WAVE)
    return seg // (WAVES * GROUPS_PER_WAVE), g // GROUPS_PER_WAVE, g % GROUPS_PER_WAVE


# block count -> (pass, wave, lane group) of the last segment and the blocks it holds
LAST = {47: ((0, 0, 2), 15), 48: ((0, 0, 2), 16), 49: ((0, 0, 3), 1), 63: ((0, 0, 3), 15), 64: ((0, 0, 3), 16), 65: ((0, 1, 0), 1),
        127: ((0, 1, 3), 15), 128: ((0, 1, 3), 16), 129: ((0, 2, 0), 1), 255: ((0, 3, 3), 15), 256: ((0, 3, 3), 16), 257: ((1, 0, 0), 1)}


@pytest.mark.parametrize("nblk", EDGES)
def test_block_counts_round_the_lane_groups(nblk):
    """A lane group's, a wave's and a pass's last segment one block short, full, and one block over."""
    steps = _run(f"blocks{nblk}")
    nseg = -(-nblk // SEG)
    assert (_place(nseg - 1), nblk - SEG * (nseg - 1)) == LAST[nblk]
    for G, n_k, W, cnt, st in steps:                            # the root holds a slab in every block, the last one partial
        assert len(cnt) == nblk and cnt[-1, 0] == B - 5 and (cnt[:-1, 0] == B).all(), cnt[:, 0]
        assert rs._segments(cnt[:, 0]) == [True] * nseg
    n_k, cnt = steps[0][1], steps[0][3]
    assert (n_k[1:] > 0).all() and (cnt[:, 1:] == 0).any(), (n_k, cnt)      # the options: slabs in some blocks, none in others


def test_option_in_one_block_of_a_waves_second_lane_group():
    """Option 2's envs all sit in one block, and that block's segment belongs to the second lane group of its wave: the wave's
    first group (and every other group of the workgroup) has no slab of this value function."""
    steps = _run("second_group")
    cnt2 = steps[0][3][:, 2]
    blocks = np.nonzero(cnt2)[0]
    seg = rs._segments(cnt2)
    assert len(blocks) == 1 and cnt2[blocks[0]] == 10 and len(seg) == 5, (blocks, seg)
    s = int(blocks[0]) // SEG
    assert _place(s)[2] == 1 and seg == [i == s for i in range(len(seg))], (s, seg)
    assert steps[0][1][2] == 10


def test_inf_and_nan_in_the_slabs_of_two_waves():
    """Overflowing weights at 65 blocks: Inf and NaN pass through lane groups that add +0 for the blocks they hold no slab in."""
    steps = _run("overflow65", free_nan=True)
    G, cnt = steps[0][0], steps[0][3]
    assert len(cnt) == 65 and _place(len(rs._segments(cnt[:, 0])) - 1) == (0, 1, 0)
    assert np.isnan(G[1]).any() and np.isinf(G[2]).any() and np.isnan(G[2]).any(), "no Inf / no NaN in G: the case tests less than it should"
    seg2 = rs._segments(cnt[:, 2])
    assert sum(seg2) >= 2 and (cnt[:, 2] == 0).any(), seg2     # option 2: several lane groups, and blocks without a slab


def test_320_blocks_with_five_options_in_the_eight_load_form():
    """The launch the headline workload's kernel form takes: its size in 64-column units (26 per value function and per line of
    26 rows of 256 envs) is past the device's compute units, here with 20 segments, four of them in a wave's second pass."""
    n, n_vf = CASES["blocks320_five_options"][0], 6
    units = 26 * (n_vf + -(-(-(-n // 256)) // 26))
    assert units > torch.cuda.get_device_properties(0).multi_processor_count, units
    steps = _run("blocks320_five_options")
    cnt = steps[0][3]
    assert len(cnt) == 320 and _place(len(rs._segments(cnt[:, 0])) - 1) == (1, 0, 3)
    assert (steps[0][1][1:] > 0).all() and (cnt[:, 1:] == 0).any()
