"""tests/step_gate_model.py on the CPU: the host model of SPEC §26's gated step-batch against the oracle's plain step, and what the
GPU tests' inputs must show (tests/test_gpu_step_gated.py runs the same scenarios on the library)."""
import numpy as np
import pytest

import step_gate_model as M
from util import oracle_block

CASES = [(257, "chain", 4, 0), (300, "tree", 1, 0), (300, "chain", 4, (1 << 33) + 77)]
IDS = ["257-chain-reoffer4", "300-tree-reoffer1", "300-chain-base2^33"]
FIELDS = ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "qcache", "action", "reward", "done")


def _plain(sc, steps=M.STEPS):
    """`steps` learning steps of sco_step alone: per step (post, G, n_k, W after)."""
    orc = M.make_oracle(sc)
    st, W = M.oracle_state(sc), sc["W"].copy()
    out = []
    for j in range(steps):
        G, n_k = orc.step(st, W, sc["clf"], M.T0 + j, M.ENABLED)
        orc.apply(W, G, n_k)
        out.append(({f: np.array(st[f], copy=True) for f in FIELDS}, G, n_k.copy(), W.copy()))
    return out


def _same(got, want, msg):
    for (post, G, n_k, W2), g in zip(want, got):
        for f in FIELDS:
            assert np.array_equal(np.ascontiguousarray(g["post"][f]).view(np.uint8), np.ascontiguousarray(post[f]).view(np.uint8)), f"{msg}: {f}"
        assert np.array_equal(g["G"].view(np.uint32), G.view(np.uint32)) and np.array_equal(g["n_k"], n_k), f"{msg}: G / n_k"
        assert np.array_equal(g["W2"].view(np.uint32), W2.view(np.uint32)), f"{msg}: W"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_shipped_gate_with_every_option_masked_is_sco_step(case):
    sc = M.scenario(*case)
    got = M.run(sc, gate_of=M.shipped, gate_mask=M.full_mask(M.N_OPT + 1))
    assert sum(int(g["info"]["entering"].sum()) for g in got) > 100 and sum(int(g["info"]["plain_declined"].sum()) for g in got) > 20
    assert all(not g["info"]["to_declined"].any() and not g["info"]["to_entered"].any() for g in got)
    _same(got, _plain(sc), f"shipped gate {case}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mask_zero_is_sco_step(case):
    sc = M.scenario(*case)
    got = M.run(sc, gate_of=lambda W: M.noisy_gate(W), gate_mask=0)
    _same(got, _plain(sc), f"mask 0 {case}")


@pytest.mark.parametrize("block", [64, 128, 256])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_noisy_gate_flips_offers_both_ways_on_every_build(case, block):
    """What tests/test_gpu_step_gated.py's third test needs from its inputs: over the run, offers flipped entered -> declined and
    declined -> entered relative to §4.2's decision on W. (The oracle of every block build: the learned W depends on it.)"""
    with oracle_block(block):
        got = M.run(M.scenario(*case), gate_of=lambda W: M.noisy_gate(W), gate_mask=M.full_mask(M.N_OPT + 1))
    to_d, to_e = (sum(int(g["info"][f].sum()) for g in got) for f in ("to_declined", "to_entered"))
    print(f"{case} block {block}: entered -> declined {to_d}, declined -> entered {to_e}")
    assert to_d >= 10 and to_e >= 10
    assert all(g["info"]["to_declined"].any() and g["info"]["to_entered"].any() for g in got[:2])      # the first two steps each (test 4 there)


def test_a_clear_bit_keeps_the_decision_on_w():
    sc = M.scenario(*CASES[0])
    never = np.zeros((M.N_OPT + 1, 2, M.NACT, M.NF), np.float32)
    never[:, 0, :, 0] = -1.0
    got = M.run(sc, gate_of=lambda W: never, gate_mask=0b0100)
    for g in got:
        i = g["info"]
        two = i["entering"] & (i["cand"] == 2)
        assert np.array_equal(i["declined"][two], np.ones(int(two.sum()), bool))
        assert np.array_equal(i["declined"][~two], i["plain_declined"][~two])
        assert (g["post"]["option_id"] != 2)[~i["keep"]].all()
    assert sum(int((g["info"]["entering"] & (g["info"]["cand"] == 2)).sum()) for g in got) > 0
