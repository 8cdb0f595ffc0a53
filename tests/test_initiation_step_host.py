"""SPEC §24.3's two pure functions on the host: initfit.candidate_tables (labels, order, which rows differ, inputs kept) and
initfit.choose_table (§21.4's rule over labelled candidates, against a plain restatement and against valuefit.choose_candidate
on the same rows). No GPU."""
import math

import numpy as np
import pytest
import torch


def _clf():
    return torch.arange(6 * 8, dtype=torch.float32).reshape(6, 8) / 7.0


def test_candidate_tables(pkg):
    from skill_chaining_with_graphs_amd.initfit import candidate_tables
    clf = _clf()
    rows = {4: torch.full((8,), -4.0), 1: np.full(8, -1.0, np.float32), 3: [-3.0] * 8}        # any order, any array type
    clf0, rows0 = clf.clone(), {k: torch.as_tensor(v, dtype=torch.float32).numpy().copy() for k, v in rows.items()}
    out = candidate_tables(clf, rows)
    assert [l for l, _ in out] == ["shipped", "1", "3", "4", "all"]
    assert all(t.shape == clf.shape and t.dtype == clf.dtype for _, t in out)
    tabs = dict(out)
    assert torch.equal(tabs["shipped"], clf0) and tabs["shipped"] is not clf
    for k in (1, 3, 4):
        differs = [r for r in range(6) if not torch.equal(tabs[str(k)][r], clf0[r])]
        assert differs == [k] and torch.equal(tabs[str(k)][k], torch.full((8,), -float(k)))
    assert [r for r in range(6) if not torch.equal(tabs["all"][r], clf0[r])] == [1, 3, 4]
    assert all(torch.equal(tabs["all"][k], tabs[str(k)][k]) for k in (1, 3, 4))
    # neither input is written, and no table shares memory with the input or with another table
    assert torch.equal(clf, clf0) and all(np.array_equal(torch.as_tensor(rows[k], dtype=torch.float32).numpy(), rows0[k]) for k in rows)
    for _, t in out:
        t.fill_(9.0)
    assert torch.equal(clf, clf0)
    # one fitted row: no "all"; none: the shipped table alone
    assert [l for l, _ in candidate_tables(clf, {2: torch.zeros(8)})] == ["shipped", "2"]
    assert [l for l, _ in candidate_tables(clf, {})] == ["shipped"]
    one = dict(candidate_tables(clf, {2: torch.zeros(8)}))["2"]
    assert torch.equal(one[2], torch.zeros(8)) and torch.equal(one[:2], clf[:2]) and torch.equal(one[3:], clf[3:])
    for bad in ({6: torch.zeros(8)}, {-1: torch.zeros(8)}):
        with pytest.raises(ValueError):
            candidate_tables(clf, bad)


def _cand(label, disc, ret, succ, diff, se):
    return {"label": label, "epsilon": 0.0, "summary": {"mean_discounted_return": disc, "mean_return": ret, "success_rate": succ},
            "paired": {k: {"mean_diff": diff, "se": se, "n": 100} for k in ("disc_final", "ret", "goal", "steps")}}


def _plain_rule(cands, mean_key, pair_key, z):
    """§21.4's rule, restated: the first candidate of the highest non-NaN mean; accepted where it is not "shipped" and its paired
    mean difference exceeds z se (se = 0: exceeds 0)."""
    best = None
    for i, c in enumerate(cands):
        m = c["summary"][mean_key]
        if m == m and (best is None or m > cands[best]["summary"][mean_key]):
            best = i
    if best is None:
        return None, False
    p = cands[best]["paired"][pair_key]
    return best, bool(best != 0 and p["mean_diff"] > (z * p["se"] if p["se"] > 0 else 0.0))


def test_choose_table(pkg):
    from skill_chaining_with_graphs_amd.initfit import choose_table
    from skill_chaining_with_graphs_amd.valuefit import choose_candidate
    ship = _cand("shipped", -10.0, -100.0, 0.5, 0.0, 0.0)
    c = [ship, _cand("1", -9.0, -90.0, 0.6, 1.0, 0.4), _cand("2", -8.0, -95.0, 0.55, 2.0, 0.9), _cand("all", -12.0, -80.0, 0.7, -2.0, 0.5)]
    assert choose_table(c, "discounted", 2.0) == {"index": 2, "label": "2", "chosen": "2", "accepted": True}
    # nothing beats "shipped" by z se: it is kept (below z se, and exactly at it)
    assert choose_table(c, "discounted", 2.5) == {"index": 2, "label": "2", "chosen": "shipped", "accepted": False}
    c[2]["paired"]["disc_final"]["se"] = 1.0
    assert choose_table(c, "discounted", 2.0)["chosen"] == "shipped"
    # "shipped" the best: kept whatever z
    worse = [ship, _cand("1", -11.0, 0.0, 0.0, -1.0, 0.1), _cand("2", -10.5, 0.0, 0.0, -0.5, 0.1)]
    for z in (2.0, 0.0, -math.inf):
        assert choose_table(worse, "discounted", z) == {"index": 0, "label": "shipped", "chosen": "shipped", "accepted": False}
    # ties go to the earlier candidate: among the candidates, and "shipped" against all of them
    tie = [ship, _cand("1", -8.0, 0.0, 0.0, 2.0, 0.1), _cand("3", -8.0, 0.0, 0.0, 2.0, 0.1), _cand("all", -8.0, 0.0, 0.0, 2.0, 0.1)]
    assert choose_table(tie, "discounted", 2.0) == {"index": 1, "label": "1", "chosen": "1", "accepted": True}
    assert choose_table([ship, _cand("1", -10.0, 0.0, 0.0, 0.0, 0.0)], "discounted", -math.inf)["index"] == 0
    # a NaN mean is never picked, however large its paired difference
    nan = [ship, _cand("1", float("nan"), 0.0, 0.0, 5.0, 0.1), _cand("2", -9.5, 0.0, 0.0, -0.5, 0.3)]
    assert choose_table(nan, "discounted", 2.0) == {"index": 2, "label": "2", "chosen": "shipped", "accepted": False}
    assert choose_table(nan, "discounted", -math.inf) == {"index": 2, "label": "2", "chosen": "2", "accepted": True}
    allnan = [_cand("shipped", float("nan"), 0.0, 0.0, 0.0, 0.0), _cand("1", float("nan"), 0.0, 0.0, 5.0, 0.1)]
    assert choose_table(allnan, "discounted", 2.0) == {"index": None, "label": None, "chosen": "shipped", "accepted": False}
    # se = 0: accepted only above 0, whatever z
    for diff, want in ((1e-9, True), (0.0, False), (-1e-9, False)):
        flat = [ship, _cand("1", -9.0, 0.0, 0.0, diff, 0.0)]
        assert choose_table(flat, "discounted", 2.0)["accepted"] is want and choose_table(flat, "discounted", math.inf)["accepted"] is want
    # each criterion reads its own mean and its own paired row
    c[3]["paired"]["ret"] = {"mean_diff": 20.0, "se": 1.0, "n": 100}
    assert choose_table(c, "return", 2.0)["chosen"] == "all"
    c[3]["paired"]["goal"] = {"mean_diff": 0.2, "se": 0.15, "n": 100}
    assert choose_table(c, "success", 2.0)["chosen"] == "shipped" and choose_table(c, "success", 1.0)["chosen"] == "all"
    # the restated rule and valuefit.choose_candidate on the same rows, over seeded random candidates
    keys = {"discounted": ("mean_discounted_return", "disc_final"), "return": ("mean_return", "ret"), "success": ("success_rate", "goal")}
    rng = np.random.default_rng(12)
    labels = ["shipped", "1", "2", "3", "4", "5", "all"]
    seen = set()
    for trial in range(300):
        n = int(rng.integers(1, 8))
        cands = []
        for i in range(n):
            v = [float(rng.choice([-1.0, -0.5, 0.0, float("nan")], p=[0.3, 0.3, 0.3, 0.1])) for _ in range(3)]
            cands.append(_cand(labels[i], *v, float(rng.choice([-1.0, 0.0, 0.5, 2.0])), float(rng.choice([0.0, 0.25, 1.0]))))
        cands[0]["paired"] = _cand("", 0, 0, 0, 0.0, 0.0)["paired"]              # "shipped" against itself: exact zeros
        for crit, (mk, pk) in keys.items():
            z = float(rng.choice([0.0, 1.0, 2.0, math.inf, -math.inf]))
            got = choose_table(cands, crit, z)
            idx, acc = _plain_rule(cands, mk, pk, z)
            assert (got["index"], got["accepted"]) == (idx, acc), (trial, crit, z)
            assert got["chosen"] == (cands[idx]["label"] if acc else "shipped")
            ref = choose_candidate([{"lambda": float(i), "summary": k["summary"], "paired": k["paired"]} for i, k in enumerate(cands)], crit, z)
            assert (got["index"], got["accepted"]) == (ref["index"], ref["accepted"])
            seen.add((idx is None, acc, idx == 0))
    assert len(seen) >= 4                                                        # all NaN, kept "shipped", picked and kept, picked and accepted
    with pytest.raises(ValueError, match="criterion"):
        choose_table(c, "length", 2.0)
    with pytest.raises(ValueError, match="shipped"):
        choose_table(c[1:], "discounted", 2.0)
    with pytest.raises(ValueError, match="shipped"):
        choose_table([], "discounted", 2.0)
