"""SkillChainingAgent.fit_values_to_branches(weighting=..., tau2=..., branches=...) (SPEC §22.3) on the rig's small trained agent, in
tests/test_gpu_branch_fit.py's style: without the argument nothing changes, by bits; with one replicate every weight is 1 and the
precision fit is the unweighted one, by bits; the kept operands reproduce A, B and Delta; `branches=` launches no rollout and
reproduces the returns; the report's statistics stay the unweighted ones; apply=False leaves the training run alone."""
import contextlib

import numpy as np
import pytest
import torch

from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.valuefit import (error_stats, greedy_table, normalise_weights, precision_weights, ridge_solve,
                                                     ridge_solve_shared, root_weights)
from bits import assert_bits_equal
from gpu_util import assert_same_bits, clone_state, crossing_agent, spy_calls

pytestmark = pytest.mark.gpu

MAX_EP = 24
KW = dict(n_states=48, n_held=16, replicates=2, n_episodes=64, epsilon=0.5, ridge=1e-3)
COUNTERS = ("t", "enabled_mask", "gest_mask")
FIT = (0, 2)                                                          # the value functions that run (option 1 is switched off)


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def fitted():
    """tests/test_gpu_branch_fit.py's agent; one kept unweighted fit, and from ITS branches the two precision fits, all under a spy
    on the training context; what the agent was before."""
    a = crossing_agent(n=256, n_opt=2)
    a.ctx.set_hparams(max_episode_steps=MAX_EP, reoffer_period=1, r_option_success=0.0)
    a.enable_option(1, False)
    before = dict(W=a.W.clone(), state=clone_state(a.state), counters={f: getattr(a, f) for f in COUNTERS})
    with spy_calls(a.ctx) as (calls, _):
        base, W_base = a.fit_values_to_branches(keep=True, seed=5, **KW)
        side_calls = []
        with contextlib.ExitStack() as spies:                         # the side contexts, from here on: a rollout would show
            for c in list(a._branch_ctx.values()) + list(a._eval_ctx.values()):
                spies.enter_context(spy_calls(c[0], side_calls))
            prec, W_prec = a.fit_values_to_branches(keep=True, seed=5, weighting="precision", branches=base, **KW)
            per, W_per = a.fit_values_to_branches(keep=True, seed=5, weighting="precision_per_action", tau2=50.0, branches=base, **KW)
    torch.cuda.synchronize()
    return dict(a=a, before=before, calls=list(calls), side_calls=side_calls, base=base, W_base=W_base, prec=prec, W_prec=W_prec,
                per=per, W_per=W_per)


def test_weighting_none_and_no_argument_give_the_same_bits(fitted):
    a = fitted["a"]
    rep, W = a.fit_values_to_branches(seed=5, weighting=None, tau2=None, branches=None, **KW)
    assert_bits_equal(host(W), host(fitted["W_base"]), msg="W_new with weighting=None against W_new without the argument:")
    assert rep["weighting"] is None and fitted["base"]["weighting"] is None and rep["tau2"] is None
    for k in FIT:
        assert "effective_n" not in rep["vf"][k] and "w" not in fitted["base"]["vf"][k]["operands"]
        assert {f: v for f, v in rep["vf"][k].items()} == {f: v for f, v in fitted["base"]["vf"][k].items() if f != "operands"}
    # and the unweighted fit from kept branches is the fit that made them
    rep2, W2 = a.fit_values_to_branches(seed=5, branches=fitted["base"], **KW)
    assert_bits_equal(host(W2), host(fitted["W_base"]), msg="W_new from the kept branches:")


def test_one_replicate_makes_every_weight_one_and_the_fit_the_unweighted_one(fitted):
    a = fitted["a"]
    kw = dict(KW, replicates=1)
    plain, W_plain = a.fit_values_to_branches(keep=True, seed=5, **kw)
    for weighting in ("precision", "precision_per_action"):
        rep, W = a.fit_values_to_branches(keep=True, seed=5, weighting=weighting, branches=plain, **kw)
        assert_bits_equal(host(W), host(W_plain), msg=f"{weighting} with one replicate against the unweighted W_new:")
        for k in FIT:
            op = rep["vf"][k]["operands"]
            assert not op["se2"].any() and np.all(op["w"] == 1.0) and np.all(host(op["rw"]) == 1.0) and rep["vf"][k]["tau2"] == 0.0
            n_eff = rep["vf"][k]["effective_n"]
            assert n_eff == ([float(op["n_fit"])] * 5 if weighting == "precision_per_action" else float(op["n_fit"]))
            assert not torch.equal(W[k], a.W[k])


def test_kept_operands_reproduce_A_B_and_delta(fitted):
    a = fitted["a"]
    for k in FIT:
        op = fitted["prec"]["vf"][k]["operands"]
        n_fit = op["n_fit"]
        w, tau2 = precision_weights(op["se2"][:n_fit])
        assert np.array_equal(op["w"], w) and fitted["prec"]["vf"][k]["tau2"] == tau2 and fitted["prec"]["tau2"] is None
        assert not np.all(w == 1.0)                                   # (two replicates: the weights have something to do)
        assert_bits_equal(host(op["rw"]), root_weights(w), msg=f"vf {k}: rw:")
        s = [t[:n_fit].contiguous() for t in op["states"]]
        D = torch.from_numpy(np.ascontiguousarray(op["D"][:, :n_fit])).to(a.W.device)
        A, B = a.ctx.feature_gram_weighted(s, [0, n_fit], op["rw"], D)
        assert op["A"].shape == (1, 1296, 1296) and op["B"].shape == (1, 5, 1296)
        assert_bits_equal(host(op["A"]), host(A), msg=f"vf {k}: A against feature_gram_weighted's:")
        assert_bits_equal(host(op["B"]), host(B), msg=f"vf {k}: B against feature_gram_weighted's:")
        delta = ridge_solve_shared(host(A)[0], host(B)[0], n_fit, KW["ridge"], a.ctx.scale)
        assert np.array_equal(delta.view(np.uint64), op["delta"].view(np.uint64))
        want = (host(fitted["before"]["W"][k]).astype(np.float64) + delta).astype(np.float32)
        assert_bits_equal(host(fitted["W_prec"][k]), want, msg=f"vf {k}: W_new:")
        assert not torch.equal(fitted["W_prec"][k], fitted["W_base"][k])
        sw, sw2 = np.cumsum(w)[-1], np.cumsum(w * w)[-1]
        assert fitted["prec"]["vf"][k]["effective_n"] == float(sw * sw / sw2) < n_fit

        op = fitted["per"]["vf"][k]["operands"]                        # per action: five segments of the same states, one target each
        w, tau2 = precision_weights(op["se2"][:n_fit], 50.0, per_action=True)
        assert tau2 == 50.0 == fitted["per"]["vf"][k]["tau2"] == fitted["per"]["tau2"] and np.array_equal(op["w"], w) and w.shape == (n_fit, 5)
        assert_bits_equal(host(op["rw"]), root_weights(w), msg=f"vf {k}: rw per action:")
        assert op["A"].shape == (5, 1296, 1296) and op["B"].shape == (5, 1, 1296)
        for act in range(5):
            A1, B1 = a.ctx.feature_gram_weighted(s, [0, n_fit], op["rw"][:, act].contiguous(), D[act:act + 1].contiguous())
            assert_bits_equal(host(op["A"][act]), host(A1)[0], msg=f"vf {k} action {act}: A:")
            assert_bits_equal(host(op["B"][act]), host(B1)[0], msg=f"vf {k} action {act}: B:")
        delta = ridge_solve(host(op["A"]), host(op["B"])[:, 0], [n_fit] * 5, KW["ridge"], a.ctx.scale)
        assert np.array_equal(delta.view(np.uint64), op["delta"].view(np.uint64))
        want = (host(fitted["before"]["W"][k]).astype(np.float64) + delta).astype(np.float32)
        assert_bits_equal(host(fitted["W_per"][k]), want, msg=f"vf {k}: W_new per action:")
        assert len(fitted["per"]["vf"][k]["effective_n"]) == 5


def test_branches_launch_no_rollout_and_reproduce_the_returns(fitted):
    assert fitted["side_calls"], "the weighted fits called nothing on the side contexts: the spy saw nothing"
    ran = set(fitted["side_calls"]) - {"scg_feature_gram_weighted", "scg_q_values"}     # the Gram and Q^new, nothing else: no rollout
    assert not ran, f"a fit from kept branches called {ran}"
    for rep in (fitted["prec"], fitted["per"]):
        assert rep["trajectory"] is fitted["base"]["trajectory"]
        for k in FIT:
            op, op0 = rep["vf"][k]["operands"], fitted["base"]["vf"][k]["operands"]
            assert op["result"] is op0["result"] and op["n_fit"] == op0["n_fit"]
            for f in ("gbar", "se2"):                                 # float64: word for word
                assert op[f].shape == op0[f].shape and np.array_equal(op[f].view(np.uint64), op0[f].view(np.uint64)), f"vf {k}: {f}"
            assert_bits_equal(op["D"], op0["D"], msg=f"vf {k}: D:")
            for i in (0, 1):
                assert np.array_equal(op["rows"][i], op0["rows"][i])
        assert rep["vf"][1]["n_fit"] == 0 and "fit" not in rep["vf"][1]


def test_the_yardstick_stays_unweighted(fitted):
    a = fitted["a"]
    for rep, W_new in ((fitted["prec"], fitted["W_prec"]), (fitted["per"], fitted["W_per"])):
        for k in FIT:
            r = rep["vf"][k]
            op = r["operands"]
            n_fit, gbar, se2, q_old = op["n_fit"], op["gbar"], op["se2"], op["q_old"]
            q_new = host(a.ctx.q_values(op["states"], W_new[k].contiguous().view(-1))).T
            assert_bits_equal(op["q_new"], q_new, msg=f"vf {k}: Q^new:")
            for name, sl in (("fit", slice(0, n_fit)), ("held_out", slice(n_fit, None))):
                h = r[name]
                assert h["old"] == error_stats(q_old[sl].reshape(-1), gbar[sl].reshape(-1))
                assert h["new"] == error_stats(q_new[sl].reshape(-1), gbar[sl].reshape(-1))
                e = (q_new[sl].astype(np.float64) - gbar[sl]).reshape(-1)
                assert h["new"]["n"] == 5 * len(gbar[sl]) and h["new"]["rmse"] == pytest.approx(float(np.sqrt(np.mean(e * e))), rel=1e-12)
                assert h["per_action"] == [{"old": error_stats(q_old[sl, c], gbar[sl, c]), "new": error_stats(q_new[sl, c], gbar[sl, c])}
                                           for c in range(5)]
                assert h["target_se"] == pytest.approx(float(np.sqrt(np.mean(se2[sl]))), rel=1e-12)
                assert h["greedy"] == greedy_table(gbar[sl], q_old[sl], q_new[sl])
            assert r["held_out"]["old"] == fitted["base"]["vf"][k]["held_out"]["old"]      # the same yardstick as the unweighted fit's


def test_given_weights_and_the_refusals(fitted):
    a, base = fitted["a"], fitted["base"]
    n_fit = base["vf"][0]["n_fit"]
    w = np.random.default_rng(3).uniform(0.5, 2.0, n_fit)
    rep, W = a.fit_values_to_branches(vfs=[0], keep=True, seed=5, weighting=w, branches=base, **KW)
    assert rep["weighting"] == "given" and np.array_equal(rep["vf"][0]["operands"]["w"], normalise_weights(w))
    rep1, W1 = a.fit_values_to_branches(vfs=[0], seed=5, weighting=np.ones(n_fit), branches=base, **KW)
    assert_bits_equal(host(W1[0]), host(fitted["W_base"][0]), msg="given unit weights against the unweighted W_new:")
    rep5, W5 = a.fit_values_to_branches(vfs=[0], seed=5, weighting=np.ones((n_fit, 5)) * 3.0, branches=base, **KW)
    assert_bits_equal(host(W5[0]), host(fitted["W_base"][0]), msg="given equal weights per action against the unweighted W_new:")
    for bad in (np.ones(n_fit + 1), np.ones((n_fit, 4)), -np.ones(n_fit), np.full(n_fit, np.nan), np.full(n_fit, np.inf)):
        with pytest.raises(ValueError):
            a.fit_values_to_branches(vfs=[0], seed=5, weighting=bad, branches=base, **KW)
    with pytest.raises(ValueError, match="weighting"):
        a.fit_values_to_branches(weighting="variance", **KW)
    for bad in ({}, {"trajectory": base["trajectory"], "vf": {}}, fitted["a"].fit_values_to_branches(vfs=[0], seed=5, branches=base, **KW)[0]):
        with pytest.raises(ValueError, match="branches"):
            a.fit_values_to_branches(vfs=[0], weighting="precision", branches=bad, **KW)
    with pytest.raises(ValueError):
        a.fit_values_to_branches(vfs=[0], weighting="precision", tau2=-1.0, branches=base, **KW)
    assert_bits_equal(host(a.W), host(fitted["before"]["W"]), msg="W after the refusals:")


def test_improve_policy_passes_the_weighting_through(fitted):
    a = fitted["a"]
    rep, W = a.improve_policy(lambdas=(1.0,), n_eval=64, seed=5, weighting="precision", **KW)
    assert rep["fit"]["weighting"] == "precision" and "effective_n" in rep["fit"]["vf"][0]
    assert_bits_equal(host(a.W), host(fitted["before"]["W"]), msg="W after improve_policy(apply=False):")


def test_apply_false_leaves_the_training_run_alone(fitted):
    """(after every other test of the module: none of them may have touched the training run)"""
    a, before = fitted["a"], fitted["before"]
    assert fitted["calls"] == [], f"the fits called into the training context: {fitted['calls']}"
    assert_bits_equal(host(a.W), host(before["W"]), msg="W:")
    assert_same_bits(a.state, before["state"], EnvState.FIELDS, msg="the training state")
    assert {f: getattr(a, f) for f in COUNTERS} == before["counters"]
