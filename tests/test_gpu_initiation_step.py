"""SPEC §24.3 on the GPU: evaluate_policies(clf=) against evaluate() with each table in place; improve_initiation()'s report,
decision, apply and refusals; refit_quadratic; the report's log-loss from scg_classifier_logits. The agent is
tests/test_gpu_population.py's (crossing_agent: options 1 and 2 on the wide chain, 24-step episodes), the trial states
tests/test_gpu_initfit.py's ring round the goal, from which option 1 both succeeds and fails."""
import numpy as np
import pytest
import torch

import test_gpu_population as P
from skill_chaining_with_graphs_amd import _lib, initfit
from skill_chaining_with_graphs_amd.evaluation import paired_differences
from gpu_util import as_bytes, dev, spy_calls
from test_gpu_initfit import near_target_states
from util import disc_weights

pytestmark = pytest.mark.gpu

ZERO = {"mean_diff": 0.0, "se": 0.0, "n": 256}
EVAL_EPS = (0.1, 0.0)       # the decision is taken at 0.1: at 0 every episode of this one-start map is the same one, and se = 0
STEP = dict(n_eval=256, iters=60, lr=2.0, seed=5, eval_epsilons=EVAL_EPS)


def _tables(a):
    """The agent's table (option 1 a disc of radius 0.3 round the goal, option 2 one of 1.05: the whole map), the two discs
    swapped, and option 1's at 1.4 of its radius with option 2's row all zeros (the empty set)."""
    tx, ty, _ = a.map.target
    radii = [0.3, 1.05]
    t1, t2 = a.clf.clone(), a.clf.clone()
    for k, r in enumerate(radii, start=1):
        assert np.array_equal(a.clf[k].cpu().numpy(), disc_weights(tx, ty, r))          # (gpu_util's wide_chain)
        t1[k] = dev(disc_weights(tx, ty, radii[2 - k]))
        t2[k] = dev(disc_weights(tx, ty, 1.4 * r))
    t2[2] = 0.0
    return [a.clf.clone(), t1, t2]


def _evaluate_with(a, table, **kw):
    """evaluate(discounted=True) with `table` copied into the agent's clf, and the agent's own put back."""
    clf0 = a.clf.clone()
    a.clf.copy_(table)
    try:
        return a.evaluate(discounted=True, per_env=True, **kw)
    finally:
        a.clf.copy_(clf0)


def _left_alone(a, before, clf0, calls, msg):
    P._assert_left_alone(a, before, calls, msg)
    assert np.array_equal(as_bytes(a.clf), as_bytes(clf0)), f"{msg}: clf"


def test_evaluate_policies_with_a_table_per_policy_is_evaluate_with_it_in_place():
    a = P._agent()
    tabs = _tables(a)
    before, clf0 = P._before(a), a.clf.clone()
    with spy_calls(a.ctx) as (calls, _):
        summaries, paired, envs = a.evaluate_policies(a.W, 0.1, None, n_episodes=256, seed=5, per_env=True, clf=tabs)
        stacked = a.evaluate_policies(a.W.reshape(1, *a.W.shape).repeat(3, 1, 1, 1), 0.1, None, n_episodes=256, seed=5,
                                      clf=torch.stack(tabs))
    _left_alone(a, before, clf0, calls, "evaluate_policies(clf=)")
    assert stacked == (summaries, paired) and len(summaries) == 3
    for c in range(3):
        want, want_env = _evaluate_with(a, tabs[c], n_episodes=256, epsilon=0.1, seed=5)
        P._assert_same_evaluation(summaries[c], envs[c], want, want_env, f"table {c}")
        assert paired[c] == paired_differences(envs[c], envs[0])
    print("entries per table:", [s["entries"] for s in summaries], "success:", [s["success_rate"] for s in summaries])
    assert all(r == ZERO for r in paired[0].values())
    assert summaries[2]["entries"][2] == 0 and summaries[0]["entries"][2] > 0           # the all-zero row: option 2 is never entered
    assert summaries[0] != summaries[2]                                                  # the tables reached the kernel
    # clf = None and one table for every policy are the two-element population: the parent's results
    W, eps, enabled = P._three_tables(a), [0.0, 0.1, 0.5], [0b110, 0b110, 0b010]
    plain = a.evaluate_policies(W, eps, enabled, n_episodes=256, seed=5, per_env=True)
    for c in range(3):
        want, want_env = P._evaluate_as(a, W[c], enabled[c], n_episodes=256, epsilon=eps[c], seed=5)
        P._assert_same_evaluation(plain[0][c], plain[2][c], want, want_env, f"clf = None, policy {c}")
    one = a.evaluate_policies(W, eps, enabled, n_episodes=256, seed=5, per_env=True, clf=a.clf)
    assert one[:2] == plain[:2]
    for c in range(3):
        for f in plain[2][c]:
            assert np.array_equal(as_bytes(one[2][c][f]), as_bytes(plain[2][c][f])), f
    # the context's rollout: the two-element population is the three-element one with None
    for bad in (dict(clf=tabs[:2]), dict(clf=torch.stack(tabs)[:, :2]), dict(clf=[tabs[0], tabs[1][:2]]), dict(clf=torch.zeros(8))):
        with pytest.raises(ValueError):
            a.evaluate_policies(W, eps, enabled, n_episodes=256, **bad)


def test_improve_initiation():
    a = P._agent()
    states = near_target_states(a.map, 512, 5)
    before, clf0 = P._before(a), a.clf.clone()
    with spy_calls(a.ctx) as (calls, _):
        report, clf_kept = a.improve_initiation(states=states, z=1e30, **STEP)
    _left_alone(a, before, clf0, calls, "improve_initiation(apply=False)")
    assert report["accepted"] is False and report["chosen"] == "shipped" and np.array_equal(as_bytes(clf_kept), as_bytes(clf0))
    assert report["criterion"] == "discounted" and report["z"] == 1e30
    opts = report["options"]
    print([(o["option"], o["successes"], o["skipped"], o["outcomes"]) for o in opts])
    assert [o["option"] for o in opts] == [1, 2] and all(o["n"] == 512 and sum(o["outcomes"].values()) == 512 for o in opts)
    fitted = [o["option"] for o in opts if o["skipped"] is None]
    assert 1 in fitted, "option 1 both succeeds and fails from these states: it is refitted"
    labels = ["shipped"] + [str(k) for k in fitted] + (["all"] if len(fitted) >= 2 else [])
    rows = report["candidates"]
    assert [(r["label"], r["epsilon"]) for r in rows] == [(l, e) for e in EVAL_EPS for l in labels]
    n_tab = len(labels)
    for e in range(2):                                                        # "shipped" against itself: exact zeros
        assert all(v == ZERO for v in rows[e * n_tab]["paired"].values())
    for o in opts:
        if o["skipped"] is None:
            for who in ("shipped", "refitted"):
                st = o[who]
                assert st["tp"] + st["fp"] + st["fn"] + st["tn"] == 256 and np.isfinite(st["log_loss"]), (o["option"], who)
        else:
            assert o["skipped"] == "the fit half holds one class only" and "refitted" not in o
    for r in rows:
        assert {"entries", "steps_share", "successes", "mean_discounted_return"} <= set(r["summary"])
    # the refit, the tables and the evaluation by hand: the same trial launch, refit_quadratic on the even-indexed states
    xs, ys, vxs, vys = (dev(v) for v in states)
    K = 2
    res = a.option_trials(torch.tensor([1, 2], dtype=torch.int32).repeat_interleave(512), xs.repeat(K), ys.repeat(K), vxs.repeat(K),
                          vys.repeat(K), seed=5)
    ok = (res.outcome.cpu().numpy() == _lib.TRIAL_SUCCESS).reshape(K, 512)
    assert [int(v.sum()) for v in ok] == [o["successes"] for o in opts]
    new = {}
    for k in fitted:
        row0 = a.clf[k].clone()
        new[k] = initfit.refit_quadratic(a._trial_ctx, a.clf[k], torch.stack((xs[0::2], ys[0::2]), 1), torch.from_numpy(ok[k - 1][0::2].copy()),
                                         60, 2.0, 1e-4)
        assert torch.equal(a.clf[k], row0) and not torch.equal(new[k], row0)           # the input row is not written
        tc = a._trial_ctx
        z = tc.classifier_logits(xs[1::2].contiguous(), ys[1::2].contiguous(), new[k]).cpu().numpy()
        want = initfit.classification_stats(z > 0, ok[k - 1][1::2], z)
        got = opts[k - 1]["refitted"]
        assert {f: got[f] for f in ("tp", "fp", "fn", "tn")} == {f: want[f] for f in ("tp", "fp", "fn", "tn")}
        assert np.float64(got["log_loss"]).view(np.uint64) == np.float64(want["log_loss"]).view(np.uint64)
    tables = initfit.candidate_tables(a.clf, new)
    assert [l for l, _ in tables] == labels
    for e, eps in enumerate(EVAL_EPS):
        summaries, paired = a.evaluate_policies(a.W, eps, None, n_episodes=256, seed=5, clf=[t for _, t in tables])
        for j in range(n_tab):
            assert rows[e * n_tab + j]["summary"] == summaries[j] and rows[e * n_tab + j]["paired"] == paired[j], (eps, labels[j])
    # the fixed-point lines: the same states under the table of every refitted row, next to the shipped table's
    fp = report["fixed_point"]
    assert [f["option"] for f in fp] == [1, 2] and all(f["table"] == labels[-1] for f in fp)
    res2 = a.option_trials(res.option, xs.repeat(K), ys.repeat(K), vxs.repeat(K), vys.repeat(K), seed=5, clf=tables[-1][1])
    ok2 = (res2.outcome.cpu().numpy() == _lib.TRIAL_SUCCESS).reshape(K, 512)
    for i, f in enumerate(fp):
        assert f["shipped"]["success_rate"] == float(ok[i].mean()) and f["refitted"]["success_rate"] == float(ok2[i].mean())
        assert f["shipped"]["outcomes"] == opts[i]["outcomes"] and sum(f["refitted"]["outcomes"].values()) == 512
    print("fixed point:", [(f["option"], f["shipped"]["success_rate"], f["refitted"]["success_rate"]) for f in fp])
    _left_alone(a, before, clf0, [], "the checks by hand")
    # the chosen table's summary is evaluate() with that table in place: z = -inf applies whatever has the highest mean
    means = [r["summary"]["mean_discounted_return"] for r in rows[:n_tab]]
    best = max(range(n_tab), key=lambda j: (means[j], -j))
    report2, clf_chosen = a.improve_initiation(states=states, z=-float("inf"), apply=True, **STEP)
    assert report2["chosen"] == labels[best] and report2["accepted"] == (best != 0)
    assert np.array_equal(as_bytes(clf_chosen), as_bytes(tables[best][1])) and np.array_equal(as_bytes(a.clf), as_bytes(clf_chosen))
    want, _ = _evaluate_with(a, clf_chosen, n_episodes=256, epsilon=EVAL_EPS[0], seed=5)
    assert report2["candidates"][best]["summary"] == want
    a.clf.copy_(clf0)


def test_apply_writes_the_chosen_table_when_accepted_and_nothing_when_not(monkeypatch):
    a = P._agent()
    states = near_target_states(a.map, 512, 5)
    before, clf0 = P._before(a), a.clf.clone()
    report, kept = a.improve_initiation(states=states, z=1e30, apply=True, **STEP)       # not accepted: nothing is written
    assert report["accepted"] is False and torch.equal(kept, clf0)
    _left_alone(a, before, clf0, [], "improve_initiation(apply=True), not accepted")
    last = report["candidates"][len(report["candidates"]) // 2 - 1]["label"]
    assert last != "shipped"
    monkeypatch.setattr(initfit, "choose_table",                                         # the rule aside: the last candidate, accepted
                        lambda cands, criterion, z: {"index": len(cands) - 1, "label": cands[-1]["label"], "chosen": cands[-1]["label"], "accepted": True})
    report, chosen = a.improve_initiation(states=states, apply=False, **STEP)
    assert report["accepted"] is True and report["chosen"] == last and not torch.equal(chosen, clf0)
    _left_alone(a, before, clf0, [], "improve_initiation(apply=False), accepted")
    report, chosen2 = a.improve_initiation(states=states, apply=True, **STEP)
    assert torch.equal(chosen2, chosen) and np.array_equal(as_bytes(a.clf), as_bytes(chosen)) and chosen2.data_ptr() != a.clf.data_ptr()
    P._assert_left_alone(a, before, [], "improve_initiation(apply=True), accepted: all but clf")


def test_a_one_class_option_is_skipped_and_the_refusals():
    a = P._agent()
    tx, ty, _ = a.map.target
    pos = a.map.sample_free(2000, np.random.default_rng(3))
    far = pos[np.hypot(pos[:, 0] - tx, pos[:, 1] - ty) > 0.45][:128]                      # outside option 1's disc: every trial fails
    assert len(far) == 128
    clf0 = a.clf.clone()
    report, kept = a.improve_initiation(options=[1], states=(far[:, 0], far[:, 1]), n_eval=256, seed=5, apply=True)
    (o,) = report["options"]
    assert o["option"] == 1 and o["successes"] == 0 and o["skipped"] == "the fit half holds one class only"
    assert [r["label"] for r in report["candidates"]] == ["shipped"] and report["chosen"] == "shipped" and report["accepted"] is False
    assert report["fixed_point"] is None and torch.equal(kept, clf0) and torch.equal(a.clf, clf0)
    kw = dict(n_states=64, n_eval=64)
    for bad in (dict(options=[3]), dict(options=[0]), dict(options=[]), dict(criterion="length"), dict(eval_epsilons=()),
                dict(eval_epsilons=[0.0] * 17),                                            # 4 tables x 17 epsilons > 64 policies
                dict(options=[1], eval_epsilons=[0.0] * 33)):
        with pytest.raises(ValueError):
            a.improve_initiation(**kw, **bad)
    a.enabled_mask = 0b010
    with pytest.raises(ValueError):
        a.improve_initiation(options=[2], **kw)
    a.enabled_mask = 0b110
    a.group = object()
    with pytest.raises(ValueError, match="sharded"):
        a.improve_initiation(apply=True, **kw)
    assert torch.equal(a.clf, clf0)


def test_initiation_report_log_loss_is_the_logits():
    a = P._agent()
    states = near_target_states(a.map, 512, 5)
    rep = a.initiation_report(1, states)
    z = a._trial_ctx.classifier_logits(rep["states"][0], rep["states"][1], a.clf[1].contiguous()).cpu().numpy()
    ok = rep["trials"].outcome.cpu().numpy() == _lib.TRIAL_SUCCESS
    want = initfit.classification_stats(rep["predicted"].cpu().numpy(), ok, z)
    assert np.isfinite(rep["log_loss"]) and rep["log_loss"] == want["log_loss"]
    assert (rep["tp"], rep["fp"], rep["fn"], rep["tn"]) == tuple(want[f] for f in ("tp", "fp", "fn", "tn"))
    assert np.array_equal(z > 0, rep["predicted"].cpu().numpy() != 0)
    zz = z.astype(np.float64)
    assert rep["log_loss"] == float(np.mean(np.logaddexp(0.0, zz) - np.where(ok, zz, 0.0)))
