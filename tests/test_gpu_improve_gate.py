"""SPEC §25.3 on the GPU: fit_gate() and improve_gate() on tests/gpu_util.py's crossing_agent at the size of
tests/test_gpu_population.py's agent (256 envs, options 1 and 2 on the wide chain, 24-step episodes): the agent is left alone, the
"shipped" candidate is evaluate(), the candidates are evaluate_policies(gate=) by hand, ONE population launch evaluates them, and
apply=True makes evaluate() act under the chosen table until `gate` is None again. No test asserts that a fitted gate helps."""
import contextlib

import numpy as np
import pytest
import torch

import test_gpu_population as P
from skill_chaining_with_graphs_amd import _lib, gatefit
from skill_chaining_with_graphs_amd.core import EnvState, ScgContext
from skill_chaining_with_graphs_amd.evaluation import paired_differences
from gpu_util import as_bytes, assert_same_bits, clone_state, spy_calls

pytestmark = pytest.mark.gpu

N_EVAL = 256
ZERO = {"mean_diff": 0.0, "se": 0.0, "n": N_EVAL}
EVAL_EPS = (0.1, 0.0)       # the decision is taken at 0.1: at 0 every episode of this one-start map is the same one, and se = 0
FIT = dict(n_record=64, n_states=256, replicates=2, epsilon=0.3, min_offers=8, seed=5)


@contextlib.contextmanager
def _count_calls():
    """Every library call of every context inside the body, by name (the training context's go to spy_calls as well)."""
    names, orig = [], ScgContext._call

    def call(self, name, *args):
        names.append(name)
        return orig(self, name, *args)

    ScgContext._call = call
    try:
        yield names
    finally:
        ScgContext._call = orig


def _left_alone(a, before, state0, calls, msg):
    P._assert_left_alone(a, before, calls, msg)
    assert_same_bits(a.state, state0, EnvState.FIELDS, msg)
    assert a.gate is None, msg


def test_fit_gate_and_improve_gate_leave_the_agent_alone():
    a = P._agent()
    before, state0 = P._before(a), clone_state(a.state)
    with spy_calls(a.ctx) as (calls, _):
        fit_report, u = a.fit_gate(**FIT)
        with _count_calls() as names:
            report, kept = a.improve_gate(eval_epsilons=EVAL_EPS, z=1e30, n_eval=N_EVAL, **FIT)
    _left_alone(a, before, state0, calls, "fit_gate / improve_gate(apply=False)")
    assert names.count("scg_rollout_population_gate") == 1, "the candidates are evaluated in ONE population launch"
    # the fit's report
    rows = fit_report["options"]
    print("fit:", [{f: r[f] for f in ("option", "n", "n_fit", "n_held", "fitted", "rmse", "agreement_fitted", "agreement_shipped")} for r in rows])
    assert 0 < fit_report["n_states"] <= 256 and fit_report["replicates"] == 2 and rows and sorted(u) == [r["option"] for r in rows if r["fitted"]]
    assert u, "no option has min_offers fit states: the fit is not exercised"
    for r in rows:
        assert r["n_fit"] + r["n_held"] == r["n"] and r["fitted"] == (r["n_fit"] >= 8)
        if r["fitted"] and r["n_held"]:
            assert np.isfinite(r["rmse"]) and 0.0 <= r["agreement_fitted"] <= 1.0 and 0.0 <= r["agreement_shipped"] <= 1.0
    assert all(v.shape == (1296,) and v.dtype == np.float64 and np.isfinite(v).all() for v in u.values())
    # the targets by hand: the recorded offer states, gate_audit per replicate with its own seed
    traj, _ = a.record_episodes(64, epsilon=0.3, seed=5)
    states = traj.offer_states(256)
    assert len(states[0]) == fit_report["n_states"]
    audits = [a.gate_audit(states=states, epsilon=0.3, seed=5 + r)["per_state"] for r in range(2)]
    assert not np.array_equal(audits[0]["g_enter"], audits[1]["g_enter"])               # the replicates have their own draws
    delta = (sum(p["g_enter"].astype(np.float64) for p in audits) - sum(p["g_decline"].astype(np.float64) for p in audits)) / 2
    opt, odd = audits[0]["option"], np.arange(len(delta)) % 2 == 1
    for r in rows:
        assert r["n"] == int((opt == r["option"]).sum()) and r["n_held"] == int((odd & (opt == r["option"])).sum())
        if r["n_held"]:
            assert r["mean_delta"] == float(np.mean(delta[odd & (opt == r["option"])]))
    # the same fit again inside improve_gate
    assert str(report["fit"]["options"]) == str(rows)                                    # (str: an unfitted row holds NaNs)
    # the step's report
    assert report["accepted"] is False and report["chosen"] == "shipped" and report["criterion"] == "discounted" and report["z"] == 1e30
    assert np.array_equal(as_bytes(kept), as_bytes(gatefit.shipped_gate(a.W)))
    labels = ["shipped", "always", "never"] + [str(k) for k in sorted(u)] + (["all"] if len(u) >= 2 else [])
    cands = report["candidates"]
    n_tab = len(labels)
    assert [(c["label"], c["epsilon"]) for c in cands] == [(l, e) for e in EVAL_EPS for l in labels]
    tables = gatefit.candidate_gates(a.W, u)
    for e, eps in enumerate(EVAL_EPS):
        ship = cands[e * n_tab]
        assert ship["summary"] == a.evaluate(n_episodes=N_EVAL, epsilon=eps, seed=5, discounted=True), f"shipped at {eps}"
        assert all(v == ZERO for v in ship["paired"].values())
        always, never = cands[e * n_tab + 1]["summary"], cands[e * n_tab + 2]["summary"]
        assert sum(always["declines"]) == 0 and sum(always["entries"]) > 0 and sum(never["entries"]) == 0 and sum(never["declines"]) > 0
        summaries, paired, envs = a.evaluate_policies(a.W, eps, None, n_episodes=N_EVAL, seed=5, per_env=True, gate=[t for _, t in tables])
        for j in range(n_tab):
            assert cands[e * n_tab + j]["summary"] == summaries[j] and cands[e * n_tab + j]["paired"] == paired[j], (eps, labels[j])
            assert paired[j] == paired_differences(envs[j], envs[0])
            assert {"entries", "declines", "steps_share", "mean_discounted_return"} <= set(summaries[j])
    assert len({str(c["summary"]) for c in cands[:n_tab]}) >= 3                          # the tables reached the kernel
    _left_alone(a, before, state0, [], "the checks by hand")
    for bad in (dict(criterion="length"), dict(eval_epsilons=())):
        with pytest.raises(ValueError):
            a.improve_gate(n_eval=N_EVAL, **dict(FIT, **bad))
    with pytest.raises(ValueError):
        a.improve_gate(eval_epsilons=tuple(0.01 * i for i in range(13)), n_eval=N_EVAL, **FIT)      # 13 x 6 > SCG_POP_MAX, before any launch


def test_apply_stores_the_gate_that_evaluate_then_acts_under():
    a = P._agent()
    before, state0 = P._before(a), clone_state(a.state)
    kw = dict(n_episodes=N_EVAL, epsilon=EVAL_EPS[0], seed=5, discounted=True)
    shipped = a.evaluate(**kw)
    with spy_calls(a.ctx) as (calls, _):
        report, chosen = a.improve_gate(eval_epsilons=EVAL_EPS, z=-float("inf"), n_eval=N_EVAL, apply=True, **FIT)
    P._assert_left_alone(a, before, calls, "improve_gate(apply=True)")
    assert_same_bits(a.state, state0, EnvState.FIELDS, "improve_gate(apply=True)")
    cands = {c["label"]: c for c in report["candidates"] if c["epsilon"] == EVAL_EPS[0]}
    means = [c["summary"]["mean_discounted_return"] for c in cands.values()]
    best = list(cands)[max(range(len(means)), key=lambda j: (means[j], -j))]
    print("chosen:", report["chosen"], "accepted:", report["accepted"], "means:", dict(zip(cands, means)))
    assert report["chosen"] == (best if report["accepted"] else "shipped") and (best != "shipped" or not report["accepted"])
    assert cands["shipped"]["summary"] == shipped
    assert a.gate is not None and np.array_equal(as_bytes(a.gate), as_bytes(chosen))
    if report["chosen"] in ("shipped", "always", "never"):
        assert np.array_equal(as_bytes(chosen), as_bytes(dict(gatefit.candidate_gates(a.W, {}))[report["chosen"]]))
    assert a.evaluate(**kw) == cands[report["chosen"]]["summary"]                        # evaluate() acts under the stored table
    assert a.evaluate_policies(a.W, EVAL_EPS[0], None, n_episodes=N_EVAL, seed=5)[0][0] == cands[report["chosen"]]["summary"]
    # an explicit table, whatever is stored; and None for SPEC §4.2's own comparison
    assert a.evaluate(gate=gatefit.never_enter(a.n_vf), **kw) == cands["never"]["summary"]
    assert a.evaluate(gate=gatefit.always_enter(a.n_vf), **kw) == cands["always"]["summary"]
    assert a.evaluate(gate=None, **kw) == shipped
    assert cands["never"]["summary"] != shipped and cands["always"]["summary"] != shipped
    for rule in (dict(interrupt=True), dict(choose="value")):
        with pytest.raises(_lib.ScgError):
            a.evaluate(gate=gatefit.never_enter(a.n_vf), **dict(kw, **rule))
    for bad in (torch.zeros(3, 5, 1296), "shipped", [gatefit.never_enter(a.n_vf)] * 2):
        with pytest.raises(ValueError):
            a.evaluate(gate=bad, **kw)
    # without the stored table evaluate() is the shipped evaluation again; the learner never read it
    a.gate = None
    assert a.evaluate(**kw) == shipped
    P._assert_left_alone(a, before, [], "the evaluations")
