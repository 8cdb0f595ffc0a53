"""SPEC §25.2 / §25.3 on the host: gatefit's pure functions (shapes, which rows are replaced, inputs unwritten), candidate_gates'
labels and order, Trajectory.offer_rows() against a hand-built record, and initfit.choose_table over gate candidates."""
import numpy as np
import pytest
import torch

from skill_chaining_with_graphs_amd import gatefit, initfit
from skill_chaining_with_graphs_amd.trajectory import BEGIN_ACTION, Trajectory, offer_rows, offer_states

A, F = 5, 1296


def _W(n_vf=3, seed=1):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n_vf, A, F)).astype(np.float32))


def test_shipped_always_never():
    W = _W()
    W0 = W.clone()
    g = gatefit.shipped_gate(W)
    assert g.shape == (3, 2, A, F) and g.dtype == torch.float32 and torch.equal(W, W0)
    assert not g[0].any() and all(torch.equal(g[k, 0], W[k]) and torch.equal(g[k, 1], W[0]) for k in (1, 2))
    assert torch.equal(gatefit.shipped_gate(W.reshape(-1)), g)              # the agent's flat view of W
    g[1, 0, 0, 0] += 1.0
    assert torch.equal(W, W0)                                               # a new tensor, not a view of W
    a = gatefit.always_enter(4)
    assert a.shape == (4, 2, A, F) and a.dtype == torch.float32 and not a.any()
    n = gatefit.never_enter(4)
    assert n.shape == (4, 2, A, F) and (n[:, 0, :, 0] == -1.0).all() and int((n != 0).sum()) == 4 * A and not n[:, 1].any()
    with pytest.raises(ValueError):
        gatefit.shipped_gate(torch.zeros(7))


def test_advantage_gate_replaces_the_fitted_rows_alone():
    W = _W(4)
    base = gatefit.shipped_gate(W)
    base0 = base.clone()
    u = {2: np.random.default_rng(3).standard_normal(F)}                    # float64, as fit_gate returns it
    u0 = u[2].copy()
    g = gatefit.advantage_gate(base, u)
    assert torch.equal(base, base0) and np.array_equal(u[2], u0) and g.shape == base.shape
    want = torch.from_numpy(u0.astype(np.float32))
    assert all(torch.equal(g[2, 0, a], want) for a in range(A)) and not g[2, 1].any()
    assert all(torch.equal(g[k], base[k]) for k in (0, 1, 3))
    for bad in ({0: u0}, {4: u0}):
        with pytest.raises(ValueError):
            gatefit.advantage_gate(base, bad)
    with pytest.raises(ValueError):
        gatefit.advantage_gate(base[:, :1], u)
    with pytest.raises(ValueError):
        gatefit.advantage_gate(base, {2: u0[:-1]})


def test_candidate_gates_labels_and_order():
    W = _W(4)
    W0 = W.clone()
    rng = np.random.default_rng(5)
    u = {3: rng.standard_normal(F), 1: rng.standard_normal(F)}
    none = gatefit.candidate_gates(W, {})
    assert [l for l, _ in none] == ["shipped", "always", "never"]
    one = gatefit.candidate_gates(W, {3: u[3]})
    assert [l for l, _ in one] == ["shipped", "always", "never", "3"]
    both = gatefit.candidate_gates(W, u)
    assert [l for l, _ in both] == ["shipped", "always", "never", "1", "3", "all"] and torch.equal(W, W0)
    t = dict(both)
    ship = gatefit.shipped_gate(W)
    assert torch.equal(t["shipped"], ship) and torch.equal(t["always"], gatefit.always_enter(4)) and torch.equal(t["never"], gatefit.never_enter(4))
    assert torch.equal(t["1"], gatefit.advantage_gate(ship, {1: u[1]})) and torch.equal(t["3"], gatefit.advantage_gate(ship, {3: u[3]}))
    assert torch.equal(t["1"][3], ship[3]) and torch.equal(t["3"][1], ship[1]) and torch.equal(t["all"][2], ship[2])
    assert torch.equal(t["all"][1], t["1"][1]) and torch.equal(t["all"][3], t["3"][3])
    assert len({id(v) for v in t.values()}) == 6 and all(v.shape == ship.shape for v in t.values())


# env 0: begin | root, no candidate | 1 declined | stay | re-offer, declined again | stay | moved into 2's set: 2 offered, entered |
#        option 2 kept | option 2 ends, 1 declined (not the root's row) | stay | the episode ends, 1 entered at the restart state
ROWS0 = dict(vf=[0, 0, 0, 0, 0, 0, 0, 2, 2, 0, 0], done=[2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], option_id=[0, 0, -1, -1, -1, -1, 2, 2, -1, -1, 1],
             term=[0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0])
# env 1: begin | 2 declined | stay or re-offer by the schedule | the episode ends
ROWS1 = dict(vf=[0, 0, 0, 0], done=[2, 0, 0, 3], option_id=[0, -2, -2, 0], term=[0, 0, 0, 0])


def _record():
    tr = Trajectory(2, 11, 0, "cpu", n_vf=3)
    launch = {f: np.zeros((11, 2), np.float32) for f in ("x", "y", "vx", "vy", "reward")}
    for f in ("action", "done", "vf", "term"):
        launch[f] = np.zeros((11, 2), np.uint8)
    launch["option_id"] = np.zeros((11, 2), np.int8)
    for e, rows in enumerate((ROWS0, ROWS1)):
        n = len(rows["vf"])
        for f, v in rows.items():
            launch[f][:n, e] = v
        launch["action"][0, e] = BEGIN_ACTION
        launch["x"][:n, e] = 0.01 * np.arange(n) + e
        launch["y"][:n, e] = 0.5 + 0.01 * np.arange(n)
        launch["vx"][:n, e] = np.arange(n)
        launch["vy"][:n, e] = -np.arange(n)
    launch["len"] = np.array([11, 4], np.int32)
    return tr.append(launch)


def test_offer_rows_against_a_hand_built_record():
    tr = _record()
    every = tr.offer_rows()                                                 # period 1: every selected row is an offer
    assert every["env"].tolist() == [0] * 6 + [1] * 2 and every["row"].tolist() == [2, 3, 4, 5, 6, 9, 1, 2]
    assert every["flat"].tolist() == [2, 3, 4, 5, 6, 9, 12, 13] and not every["stay"].any()
    assert every["option"].tolist() == [1, 1, 1, 1, 2, 1, 2, 2] and every["entered"].tolist() == [False] * 4 + [True] + [False] * 3
    r = tr.offer_rows(reoffer_period=4)                                     # t = row, env ids 0 and 1: rows 4 / 3 are on the schedule
    assert r["stay"].tolist() == [False, True, False, True, False, True, False, True]
    for f in ("flat", "env", "row", "option", "entered"):
        assert np.array_equal(r[f], every[f]), f
    r = tr.offer_rows(reoffer_period=4, t0=2, env_ids=[7, 0])               # t + id = row + 9 / row + 2: rows 3 / 2 are on it
    assert r["stay"].tolist() == [False, False, True, True, False, True, False, False]
    r = tr.offer_rows(reoffer_period=2, t0=1)                               # odd rows (env 1: even rows) are on it
    assert r["stay"].tolist() == [False, False, True, False, False, False, False, False]
    for bad in (dict(reoffer_period=3), dict(reoffer_period=0), dict(env_ids=[1, 2, 3])):
        with pytest.raises(ValueError):
            tr.offer_rows(**bad)
    # offer_states: the selection, stays among them, in env order; the flat form is the method's
    flat = tr.to_numpy()
    old = np.nonzero((flat["vf"] == 0) & (flat["done"] == 0) & (flat["option_id"] != 0))[0]      # the report tool's selection
    assert np.array_equal(every["flat"], old)
    x, y, vx, vy = tr.offer_states(5)
    assert x.dtype == np.float32 and np.array_equal(x, flat["x"][old[:5]]) and np.array_equal(vy, flat["vy"][old[:5]])
    assert vx.tolist() == [2.0, 3.0, 4.0, 5.0, 6.0] and len(tr.offer_states()[0]) == 8 and len(tr.offer_states(0)[0]) == 0
    assert all(np.array_equal(a, b) for a, b in zip(offer_states(flat, 5), (x, y, vx, vy)))
    assert np.array_equal(offer_rows(flat, 4)["stay"], tr.offer_rows(4)["stay"])
    one = {f: flat[f][:11] for f in ("vf", "done", "option_id")}            # a dict without offsets: one env
    assert offer_rows(one, 4)["row"].tolist() == [2, 3, 4, 5, 6, 9] and offer_rows(one, 4)["stay"].tolist() == [False, True, False, True, False, True]


def _cand(label, mean, diff=0.0, se=0.0):
    pair = {"mean_diff": diff, "se": se, "n": 64}
    return {"label": label, "epsilon": 0.0, "summary": {"mean_discounted_return": mean, "mean_return": mean, "success_rate": 0.5},
            "paired": {"disc_final": pair, "ret": pair, "goal": {"mean_diff": 0.0, "se": 0.0, "n": 64}}}


def test_choose_table_over_gate_candidates():
    nan = float("nan")
    # se = 0: accepted where the paired difference exceeds 0, whatever z
    pick = initfit.choose_table([_cand("shipped", 1.0), _cand("always", 2.0, 1.0, 0.0), _cand("never", 0.5, -0.5, 0.0)], "discounted", 1e30)
    assert pick == {"index": 1, "label": "always", "chosen": "always", "accepted": True}
    pick = initfit.choose_table([_cand("shipped", 1.0), _cand("always", 2.0, 0.0, 0.0)], "discounted", 2.0)
    assert pick["label"] == "always" and pick["chosen"] == "shipped" and pick["accepted"] is False
    # se > 0: z standard errors
    assert initfit.choose_table([_cand("shipped", 1.0), _cand("never", 2.0, 1.0, 0.6)], "discounted", 2.0)["accepted"] is False
    assert initfit.choose_table([_cand("shipped", 1.0), _cand("never", 2.0, 1.0, 0.4)], "discounted", 2.0)["chosen"] == "never"
    # a NaN mean is never picked, however large its paired difference
    pick = initfit.choose_table([_cand("shipped", 1.0), _cand("always", nan, 9.0, 0.0), _cand("never", 1.5, 0.5, 0.1), _cand("1", nan)], "discounted", 2.0)
    assert pick == {"index": 2, "label": "never", "chosen": "never", "accepted": True}
    pick = initfit.choose_table([_cand("shipped", nan), _cand("always", nan)], "discounted", 2.0)
    assert pick == {"index": None, "label": None, "chosen": "shipped", "accepted": False}
    # ties go to the earlier candidate; a tie with "shipped" keeps it
    pick = initfit.choose_table([_cand("shipped", 1.0), _cand("always", 2.0, 1.0, 0.1), _cand("never", 2.0, 1.0, 0.1), _cand("1", 2.0, 1.0, 0.1)],
                                "discounted", 2.0)
    assert pick["index"] == 1 and pick["chosen"] == "always"
    pick = initfit.choose_table([_cand("shipped", 2.0), _cand("always", 2.0, 0.0, 0.0), _cand("never", 1.0, -1.0, 0.1)], "return", 0.0)
    assert pick == {"index": 0, "label": "shipped", "chosen": "shipped", "accepted": False}
    with pytest.raises(ValueError):
        initfit.choose_table([_cand("always", 1.0), _cand("shipped", 1.0)])
