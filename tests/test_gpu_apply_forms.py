"""The four forms of SPEC §5's update give the same bits: scg_apply_update, scg_apply_update_packed, scg_apply_update_slots (1 and 3
slots) and a one-rank scg_peer_exchange_apply — each against the oracle's apply() on the same G, all 3 x 5 x 1296 weights, exactly.

A context of 256 envs with root + 2 options. The counts cover every branch of the update: one value function with count 0 (its row
stays), one below update_count_floor, one above it; run with floor 0 and with a floor between the two non-zero counts.

The first three forms take the caller's operand: G is random float32, three slots whose sum in slot order (numpy float32, one
addition at a time, the float counts the same way) is the reference G. The peer form reads its operand from the context's peer
region, which only a learning step can fill (the C-ABI hands out no pointer into it): there the operand is the G of one learning step
(option 2 disabled: count 0; option 1: the ten envs an earlier step started in it; the root: all 256), checked against the oracle's
step on the same states, and the packed form is run on the same G beside it."""
import numpy as np
import pytest

import sc_oracle
from gpu_util import dev, make_pair, state_to_device
from util import chain_classifiers, make_oracle, random_states, random_weights

pytestmark = pytest.mark.gpu

N, N_OPT, N_VF = 256, 2, 3
NW = N_VF * 5 * 1296
SLOT_COUNTS = np.array([[100, 0, 2], [150, 0, 4], [50, 0, 1]], np.int32)        # sums: 300 (above the floor), 0, 7 (below it)
STEP_MASK, STEP_T = 0b010, 1                                                      # the learning step: option 1 only


def _slots():
    rng = np.random.default_rng(71)
    slots = (rng.standard_normal((3, NW + N_VF)) * rng.choice([1e-3, 1.0, 1e3], size=(3, 1))).astype(np.float32)
    slots[:, NW:] = SLOT_COUNTS.astype(np.float32)
    return slots


def _slot_sum(slots):
    """The slots added in slot order, one float32 addition at a time (G and the float counts alike)."""
    acc = slots[0].copy()
    for r in range(1, len(slots)):
        acc = (acc + slots[r]).astype(np.float32)
    return acc


def _floor(n_k, between):
    lo, hi = sorted(int(c) for c in n_k if c > 0)
    assert sorted(int(c) for c in n_k)[0] == 0 and lo + 1 < hi, n_k             # one row untouched, one count on each side of the floor
    return (lo + hi) // 2 if between else 0


_STEP = None


def _step_operand():
    """One learning step's inputs (state, W, classifiers) and what the oracle makes of them (G, n_k): once, handed out as copies."""
    global _STEP
    if _STEP is None:
        orc, m = make_oracle("pinball_simple", N, n_options=N_OPT, seed=2, enabled_mask=STEP_MASK)
        st = sc_oracle.new_state(N, m)
        st["x"][:], st["y"][:], st["vx"][:], st["vy"][:] = random_states(m, N, 5, vmax=1.0)
        W0, clf = random_weights(N_VF, 6, std=0.05), chain_classifiers(m, N_OPT)
        orc.step(st, W0, clf, 0)                                                 # (the first step starts the options; the next one updates them)
        G, n_k = orc.step({k: v.copy() for k, v in st.items()}, W0, clf, STEP_T)
        _STEP = (st, W0, clf, G, n_k)
    return tuple(a.copy() if isinstance(a, np.ndarray) else {k: v.copy() for k, v in a.items()} for a in _STEP)


@pytest.mark.parametrize("between", [False, True], ids=["floor0", "floor_between"])
def test_caller_operand_forms_agree_with_the_oracle(between):
    slots = _slots()
    packed = _slot_sum(slots)
    G, n_k = packed[:NW].reshape(N_VF, 5, 1296), packed[NW:].astype(np.int32)
    assert np.array_equal(n_k, SLOT_COUNTS.sum(axis=0))
    ctx, orc, m = make_pair("pinball_simple", N, n_options=N_OPT, seed=2, update_count_floor=_floor(n_k, between))
    W0 = random_weights(N_VF, 8, std=0.05)
    W_o = W0.copy()
    orc.apply(W_o, G, n_k)
    assert np.array_equal(W_o[1], W0[1]) and not np.array_equal(W_o[0], W0[0]) and not np.array_equal(W_o[2], W0[2])
    forms = {
        "apply_update": lambda W: ctx.apply_update(W, dev(G).view(-1), dev(n_k)),
        "apply_update_packed": lambda W: ctx.apply_update_packed(W, dev(packed)),
        "apply_update_slots[1]": lambda W: ctx.apply_update_slots(W, dev(packed[None, :])),
        "apply_update_slots[3]": lambda W: ctx.apply_update_slots(W, dev(slots)),
    }
    for name, form in forms.items():
        W_d = dev(W0.copy())
        form(W_d.view(-1))
        assert np.array_equal(W_d.cpu().numpy(), W_o), name
    ctx.close()


@pytest.mark.parametrize("between", [False, True], ids=["floor0", "floor_between"])
def test_one_rank_peer_exchange_agrees_with_the_oracle(between):
    st_o, W0, clf, G, n_k = _step_operand()
    ctx, orc, m = make_pair("pinball_simple", N, n_options=N_OPT, seed=2, enabled_mask=STEP_MASK,
                            update_count_floor=_floor(n_k, between))
    W_o = W0.copy()
    orc.apply(W_o, G, n_k)
    clf_d = dev(clf).view(-1)
    # the peer form: a group of one rank; the step leaves its operand in the region, the exchange applies it
    ctx.peer_open(1, 0, [ctx.peer_export()])
    ctx.set_peer_timeout(1.0)                                                     # (the device-side wait is bounded; nothing to wait for here)
    W_p = dev(W0.copy())
    ctx.step(state_to_device(st_o, ctx), W_p.view(-1), clf_d, STEP_MASK, STEP_T, learn=True, apply=False)
    ctx.peer_exchange_apply(W_p.view(-1))
    assert ctx.async_status(synchronize=True) == 0
    assert np.array_equal(W_p.cpu().numpy(), W_o), "scg_peer_exchange_apply"
    # the same step's operand through the packed form on a context without a peer region
    ctx2, _, _ = make_pair("pinball_simple", N, n_options=N_OPT, seed=2, enabled_mask=STEP_MASK,
                           update_count_floor=_floor(n_k, between))
    gp = ctx2.grad_packed()
    W_k = dev(W0.copy())
    ctx2.step(state_to_device(st_o, ctx2), W_k.view(-1), clf_d, STEP_MASK, STEP_T, learn=True, apply=False)
    flat = gp.cpu().numpy()
    assert np.array_equal(flat[:NW].reshape(G.shape), G) and np.array_equal(flat[NW:], n_k.astype(np.float32))
    ctx2.apply_update_packed(W_k.view(-1), gp)
    assert np.array_equal(W_k.cpu().numpy(), W_o), "scg_apply_update_packed on the step's operand"
    ctx2.close()
    ctx.close()
