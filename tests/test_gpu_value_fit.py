"""SkillChainingAgent.fit_values_to_returns (SPEC §16) on a 256-env agent with one enabled option on the rig's dense map:
its targets against the scalar model of §16.2 (also with an option step limit of 3, where option 2 times out inside its initiation
set and is entered again: several executions in one run of a vf), each (A, b) it formed against the host model of §16.1, its weights against the
normal equations, the objective's inequality, rows without samples, apply=False / apply=True, and the report tool at toy size."""
import numpy as np
import pytest
import torch

import gram_model as GM
from bits import assert_bits_equal
from gpu_util import crossing_agent, dev, gestating_agent, spy_calls
from skill_chaining_with_graphs_amd.agent import SkillChainingAgent
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd import ScgError, _lib
from test_gpu_tools import tool
from test_gram_host import RESIDUAL_RATIO_BOUND
from util import HP, SCALE, dense_map, disc_weights, make_oracle

pytestmark = pytest.mark.gpu

NF = 1296
N_EPISODES, RIDGE, EPS = 256, 1e-3, 0.5
RUN, IDLE = (0, 2), 1            # the value functions that run in the record, and the one that never does
IDX = GM.index_set(_lib.GRAM_MACRO_TILE)


def fit_agent(**hp):
    """The agent and one fit with everything kept. Option 2 (enabled) is offered everywhere outside its target, option 1's set:
    everything but a small disc round the start, so it is offered at the start and succeeds when the ball leaves the disc.
    Option 1 gestates (known, never selected): value function 1 never runs. W is random at a scale that has nothing to do
    with the returns; half the actions are random (every episode has the one start)."""
    m = dense_map()
    ag = SkillChainingAgent(m, 256, 2, seed=5, block_envs=256, **dict(HP, max_episode_steps=63, **hp))
    ag.init_weights(std=0.05, seed=3)
    sx, sy = (float(v) for v in m.starts[0])
    clf = np.zeros((3, 8), np.float32)
    clf[1], clf[2] = -disc_weights(sx, sy, 0.04), disc_weights(0.5, 0.5, 1.5)
    ag.clf.copy_(dev(clf))
    ag.enable_option(2)
    ag.gest_mask = 0b010
    ag.gest_counts = ag.ctx.set_gestation(ag.gest_mask)
    W0 = ag.W.clone()
    report, W_new = ag.fit_values_to_returns(n_episodes=N_EPISODES, epsilon=EPS, seed=9, ridge=RIDGE, keep=True)
    torch.cuda.synchronize()
    orc, _ = make_oracle("pinball_simple")
    return dict(ag=ag, W0=W0, report=report, W_new=W_new, orc=orc)


@pytest.fixture(scope="module")
def fitted():
    f = fit_agent()
    yield f
    f["ag"].ctx.close()


SHORT_OPTION_STEPS = 3           # option 2 needs more steps than this to leave the start's disc: it times out inside its own initiation set


@pytest.fixture(scope="module")
def fitted_short():
    """The same agent with max_option_steps = 3: option 2 ends by TIMEOUT while the ball is still inside its initiation set, is the
    candidate again on the next step (SPEC §4.2) and is entered again: several executions in one run of vf = 2."""
    f = fit_agent(max_option_steps=SHORT_OPTION_STEPS)
    yield f
    f["ag"].ctx.close()


def test_the_record_is_what_the_test_needs(fitted):
    rep = fitted["report"]
    flat = rep["trajectory"].to_numpy()
    rows = np.diff(flat["offsets"])
    assert rows.max() <= 64 and rows.mean() > 16
    assert sum(rep["vf"][0]["n"]) > 1000 and sum(rep["vf"][2]["n"]) > 300, "both value functions must run"
    assert rep["vf"][IDLE]["n"] == [0] * 5
    assert torch.equal(fitted["ag"].W, fitted["W0"])


def test_targets_equal_the_scalar_model(fitted):
    rep, ag = fitted["report"], fitted["ag"]
    flat, tg = rep["trajectory"].to_numpy(), rep["targets"]
    off = flat["offsets"]
    bonus = 0
    for e in range(N_EPISODES):
        sl = slice(off[e], off[e + 1])
        g, y = GM.scalar_targets(flat["reward"][sl], flat["vf"][sl], flat["term"][sl], float(ag.ctx.cfg.gamma), float(ag.ctx.cfg.r_option_success))
        assert np.allclose(tg["g"][sl], g, rtol=1e-13, atol=0) and np.allclose(tg["y"][sl], y, rtol=1e-13, atol=0), e
        bonus += int(np.sum(np.asarray(y) != np.asarray(g)))
    assert bonus > 0, "no option run of the record ended in SUCCESS: the pseudo-reward is not exercised"
    for k in RUN:                                                    # ... and they are the targets of the samples, in (env, row) order per action
        op = rep["vf"][k]["operands"]
        assert np.array_equal(op["y"], tg["y"][op["rows"]]) and np.all(flat["vf"][op["rows"]] == k)
        fit = op["rows"][: op["n_fit"]]
        env = np.searchsorted(off, fit, side="right") - 1
        assert np.all(env % 2 == 0) and np.all((np.searchsorted(off, op["rows"][op["n_fit"]:], side="right") - 1) % 2 == 1)
        for a in range(5):
            seg = fit[op["offsets"][a]: op["offsets"][a + 1]]
            assert np.all(flat["action"][seg] == a) and np.all(np.diff(seg) > 0)


def test_targets_follow_executions_when_an_option_times_out_and_is_entered_again(fitted_short):
    """SPEC §16.2's tau on a record in which one run of vf = 2 holds several executions: targets["y"] against the scalar model
    bit for bit, and the rows that carry a bonus are exactly the rows of Trajectory.segments' runs of an option that end in SUCCESS."""
    rep, ag = fitted_short["report"], fitted_short["ag"]
    traj, tg = rep["trajectory"], rep["targets"]
    flat = traj.to_numpy()
    off, vf, term = flat["offsets"], flat["vf"], flat["term"]
    gamma, r_succ = float(ag.ctx.cfg.gamma), float(ag.ctx.cfg.r_option_success)
    assert ag.ctx.cfg.max_option_steps == SHORT_OPTION_STEPS and r_succ == 100.0
    reentered = then_success = 0
    for e in range(N_EPISODES):
        sl = slice(off[e], off[e + 1])
        v, t = vf[sl], term[sl]
        for j in range(len(v) - 1):
            if t[j] == _lib.TRIAL_TIMEOUT and v[j + 1] == v[j]:
                reentered += 1
                k = j + 1
                while k + 1 < len(v) and v[k + 1] == v[j] and t[k] != _lib.TRIAL_SUCCESS:
                    k += 1
                then_success += int(t[k] == _lib.TRIAL_SUCCESS)
        g, y = GM.scalar_targets(flat["reward"][sl], v, t, gamma, r_succ)
        assert np.array_equal(tg["g"][sl], g) and np.array_equal(tg["y"][sl], y), e
        paid = np.zeros(len(v), bool)                                # ... and by the record's own segments
        for s in traj.segments(e):
            if s["vf"] >= 1 and s["term"] == _lib.TRIAL_SUCCESS:
                paid[max(s["start"], 1): s["end"] + 1] = True
                rows = np.arange(max(s["start"], 1), s["end"] + 1)
                want = tg["g"][sl][rows] + np.array([gamma ** int(s["end"] - j) * r_succ for j in rows])
                assert np.array_equal(tg["y"][sl][rows], want), (e, s)
        assert np.array_equal(tg["y"][sl] != tg["g"][sl], paid), e
    print(f"TIMEOUT rows followed by the same vf: {reentered}, of them followed by a SUCCESS in the same vf run: {then_success}")
    assert reentered >= 50 and then_success >= 20


@pytest.mark.parametrize("k", RUN)
def test_operands_equal_the_host_model(fitted, k):
    op, ag = fitted["report"]["vf"][k]["operands"], fitted["ag"]
    s = [t.cpu().numpy() for t in op["states"]]
    phi = fitted["orc"].features(*s)
    q = fitted["orc"].q_values(*s, fitted["W0"][k].cpu().numpy())
    d = (op["y"] - q[op["action"], np.arange(len(op["y"]))].astype(np.float64)).astype(np.float32)
    assert_bits_equal(op["d"], d, msg=f"vf {k}: residuals:")
    A, b = op["A"].cpu().numpy(), op["b"].cpu().numpy()
    assert_bits_equal(A[np.ix_(range(5), IDX, IDX)], GM.gram(phi, op["offsets"], IDX, IDX), msg=f"vf {k}: A on the index set:")
    assert_bits_equal(b, GM.rhs(phi, d, op["offsets"]), msg=f"vf {k}: b:")


@pytest.mark.parametrize("k", RUN)
def test_weights_satisfy_the_normal_equations_and_lower_the_fit_error(fitted, k):
    """The matrix is the kernel's A (tied to the model by test_operands_equal_the_host_model and tests/test_gpu_gram.py: the full
    model matrix would cost minutes); the residual bound is test_gram_host's."""
    rep = fitted["report"]["vf"][k]
    op = rep["operands"]
    A, b = op["A"].cpu().numpy().astype(np.float64), op["b"].cpu().numpy().astype(np.float64)
    w_old = fitted["W0"][k].cpu().numpy()
    for a in range(5):
        n = rep["n"][a]
        M = A[a] + np.diag(RIDGE * max(n, 1) / SCALE.astype(np.float64) ** 2)
        res = np.linalg.norm(M @ op["delta"][a] - b[a])
        scale = np.finfo(np.float64).eps * NF * (np.linalg.norm(M) * np.linalg.norm(op["delta"][a]) + np.linalg.norm(b[a]))
        print(f"vf {k} action {a}: n {n} residual ratio {res / scale:.3g}")
        assert res <= RESIDUAL_RATIO_BOUND * scale
    assert_bits_equal(fitted["W_new"][k].cpu().numpy(), (w_old.astype(np.float64) + op["delta"]).astype(np.float32), msg="W_new:")
    # the objective sum (y - Q)^2 + penalty is minimised with the penalty centred on W_old: the fit half's SSE cannot rise
    old, new = rep["fit"]["old"], rep["fit"]["new"]
    sse = lambda e: e["rmse"] ** 2 * e["n"]
    print(f"vf {k}: fit rmse {old['rmse']:.2f} -> {new['rmse']:.2f}, held-out {rep['held_out']['old']['rmse']:.2f} -> {rep['held_out']['new']['rmse']:.2f}")
    assert sse(new) <= sse(old) and sse(new) < 0.5 * sse(old), "the seeded case must make the inequality strict by a wide margin"
    # ... nor exceed the objective at any other point, e.g. at the best constant per action (feature 0 alone, scale 1): J = sum (d - c)^2 + ridge n c^2
    j_const = 0.0
    for a in range(5):
        da = op["d"][op["offsets"][a]: op["offsets"][a + 1]].astype(np.float64)
        if len(da):
            c = da.sum() / (len(da) * (1 + RIDGE))
            j_const += float(np.sum((da - c) ** 2) + RIDGE * len(da) * c * c)
    print(f"vf {k}: SSE old {sse(old):.6g}, at the best constants {j_const:.6g}, new {sse(new):.6g}")
    assert sse(new) <= j_const * (1 + 1e-3) and j_const < sse(old)
    assert rep["delta_norm"] > 0 and old["n"] == sum(rep["n"]) and rep["held_out"]["old"]["n"] > 0


def test_rows_without_samples_keep_their_bits(fitted):
    assert torch.equal(fitted["W_new"][IDLE], fitted["W0"][IDLE])
    assert fitted["report"]["vf"][IDLE]["delta_norm"] == 0.0
    assert all(not torch.equal(fitted["W_new"][k], fitted["W0"][k]) for k in RUN)


@pytest.mark.parametrize("make", [crossing_agent, gestating_agent])
def test_apply_false_leaves_the_training_run_alone(make):
    a = make(n=512)
    a.enable_tracing(16)
    for _ in range(3):
        a.step_batch()
    W0, t0 = a.W.clone(), a.t
    st0 = {f: getattr(a.state, f).clone() for f in EnvState.FIELDS}
    ring0 = [t.clone() for t in a.trace] if isinstance(a.trace, (list, tuple)) else None
    gest0 = a.gest_counts.clone() if hasattr(a, "gest_counts") else None
    with spy_calls(a.ctx) as (calls, _):
        report, W_new = a.fit_values_to_returns(n_episodes=64, seed=2)
    torch.cuda.synchronize()
    assert calls == [], f"fit_values_to_returns called into the training context: {calls}"
    assert torch.equal(a.W, W0) and a.t == t0 and not torch.equal(W_new, W0)
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(a.state, f), st0[f]), f
    if ring0 is not None:
        assert all(torch.equal(x, y) for x, y in zip(a.trace, ring0))
    if gest0 is not None:
        assert torch.equal(a.gest_counts, gest0)
    a.step_batch()                                                   # ... and the run goes on
    assert a.t == t0 + 1


def test_apply_true_changes_exactly_the_listed_rows(fitted):
    ag, W0 = fitted["ag"], fitted["W0"]
    try:
        report, W_new = ag.fit_values_to_returns(n_episodes=N_EPISODES, epsilon=EPS, seed=9, ridge=RIDGE, vfs=[2], apply=True)
        assert set(report["vf"]) == {2}
        assert torch.equal(ag.W[0], W0[0]) and torch.equal(ag.W[1], W0[1])
        assert torch.equal(ag.W[2], fitted["W_new"][2]) and torch.equal(W_new[2], ag.W[2]) and torch.equal(W_new[0], W0[0])
        with pytest.raises(ValueError):
            ag.fit_values_to_returns(n_episodes=N_EPISODES, vfs=[3])
        ag.group = object()                                          # shared weights: refused before anything runs
        with pytest.raises(ScgError, match="shared weights"):
            ag.fit_values_to_returns(n_episodes=N_EPISODES, apply=True)
    finally:
        ag.group = None
        ag.W.copy_(W0)


def test_value_fit_report_runs_end_to_end_at_toy_size(tmp_path):
    out = tool("value_fit_report.py", "--maps", "pinball_simple", "--seeds", 1, "--envs", 256, "--warm", 40, "--after", 8,
               "--steps-per-option", 16, "--min-examples", 64, "--states", 128, "--episodes", 128, "--options", 2, "--record-envs", 16, "--out-dir", tmp_path).splitlines()
    assert out[0].startswith("# value_fit_report map pinball_simple envs 256 ")
    assert out[1].startswith("seed 1: ")
    assert (tmp_path / "r22_value_fit_pinball_simple.txt").read_text().splitlines() == out
    assert sum(ln.startswith("  fit round ") for ln in out) == 2
    assert any(ln.startswith("  before      success ") for ln in out) and any(ln.startswith("  after       success ") for ln in out)
    rows = [ln.split() for ln in out if ln.startswith("    vf ") and ln.split()[1].isdigit()]
    assert rows and all(len(r) == 11 for r in rows)
