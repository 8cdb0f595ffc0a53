"""SPEC §29.2 on the device, on the small agent of tests/test_gpu_lambda_returns.py (64 recorded episodes at epsilon = 0.5, a few
thousand step rows): valuefit.double_targets against valuefit.trace_targets where the two tables are one and against
tests/double_model.py where they are not, and fit_values_to_returns(double=True) end to end — the optimism of the first and second
sweep, the mean table, fold A's table against a direct Gram and ridge solve, the agent left alone, the single path untouched, the
refusals."""
import numpy as np
import pytest
import torch

import double_model as DM
from skill_chaining_with_graphs_amd import ScgError
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.valuefit import (double_targets, fold_of, lambda_targets, mean_table, ridge_solve,
                                                     trace_targets)
from gpu_util import dev, spy_calls
from test_gpu_lambda_returns import small_agent  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

LAM, RIDGE = 0.9, 1e-3


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same32(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def parts(small_agent):
    ag, report, W_mc = small_agent
    traj = report["trajectory"]
    c = ag.ctx.cfg
    return ag, traj, traj.to_numpy(), ag._eval_ctx[64][0], W_mc, float(c.gamma), float(c.r_option_success)


def q_all(ctx, states, Wk):
    """[5][n] by ScgContext.q_values in chunks of the context's envs"""
    n = len(states[0])
    out = np.zeros((5, n), np.float32)
    for i in range(0, n, ctx.n_envs):
        sl = slice(i, i + ctx.n_envs)
        out[:, sl] = ctx.q_values([dev(np.ascontiguousarray(s[sl])) for s in states], dev(np.ascontiguousarray(Wk)).view(-1)).cpu().numpy()
    return out


def direct_refit(ectx, flat, y, rows, Wk, scale):
    """SPEC §16.3 on the step rows `rows` against the targets y: sorted by action, Q^old by q_values, the residual rounded once,
    feature_gram with the action as segment, ridge_solve, float32(W + Delta); an action without samples keeps its row."""
    rows = rows[np.argsort(flat["action"][rows], kind="stable")]
    act = flat["action"][rows].astype(np.int64)
    st = [np.ascontiguousarray(flat[f][rows - 1]) for f in ("x", "y", "vx", "vy")]
    w_old = Wk.cpu().numpy()
    q_old = q_all(ectx, st, w_old)[act, np.arange(len(act))]
    d = (y[rows] - q_old.astype(np.float64)).astype(np.float32)
    n_a = np.bincount(act, minlength=5).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(n_a)]).astype(np.int64)
    A, b = ectx.feature_gram([dev(s) for s in st], offsets, dev(d))
    delta = ridge_solve(A.cpu().numpy(), b.cpu().numpy(), n_a, RIDGE, scale)
    w_new = (w_old.astype(np.float64) + delta).astype(np.float32)
    w_new[n_a == 0] = w_old[n_a == 0]
    return w_new, n_a


@pytest.mark.parametrize("cut", [False, True])
def test_double_targets_of_one_table_are_trace_targets_by_bits(small_agent, cut):
    ag, traj, flat, ectx, W_mc, gamma, R = parts(small_agent)
    for lam in (LAM, [0.9, 0.3, 1.0]):
        tt = trace_targets(ectx, flat, ag.W, gamma, lam, R, cut=cut)
        dt = double_targets(ectx, flat, ag.W, ag.W.clone(), gamma, lam, R, cut=cut)
        for f in ("y0", "yk", "h", "ag", "y", "v0", "vk", "c", "cut", "sample"):
            assert bits_equal(dt[f], tt[f]), (f, lam)
        assert bits_equal(dt["vs0"], dt["v0"]) and bits_equal(dt["vsk"], dt["vk"])
    assert tt["sample"].sum() > 1000 and (tt["v0"] != 0).sum() > 1000 and (tt["vk"] != 0).sum() > 20 and tt["cut"].any()


@pytest.mark.parametrize("cut", [False, True])
def test_double_targets_of_two_tables_equal_the_model_by_bits(small_agent, cut):
    ag, traj, flat, ectx, W_mc, gamma, R = parts(small_agent)
    assert not torch.equal(W_mc, ag.W)
    q_values = lambda st, Wk: q_all(ag.ctx, st, Wk)
    lam = [0.9, 0.3, 1.0]
    dt = double_targets(ectx, flat, ag.W, W_mc, gamma, lam, R, cut=cut)
    want = DM.double_targets(q_values, flat, ag.W.cpu().numpy(), W_mc.cpu().numpy(), gamma, lam, R, cut)
    for f in ("v0", "vk", "vs0", "vsk", "ag", "y0", "yk", "h"):
        assert bits_equal(dt[f], want[f]), f
    tt = trace_targets(ectx, flat, ag.W, gamma, lam, R, cut=cut)
    assert bits_equal(dt["ag"], tt["ag"]) and bits_equal(dt["vs0"], tt["v0"]) and bits_equal(dt["vsk"], tt["vk"])     # the selecting side is W's
    assert not bits_equal(dt["y0"], tt["y0"]) and (dt["v0"] != dt["vs0"]).sum() > 1000
    with pytest.raises(ScgError, match="one shape"):
        double_targets(ectx, flat, ag.W, W_mc[:2], gamma, LAM, R)
    with pytest.raises(ScgError, match="double_targets: gamma and lam"):
        double_targets(ectx, flat, ag.W, W_mc, gamma, 1.5, R)


@pytest.fixture(scope="module")
def double_fit(small_agent):
    ag, traj, flat, ectx, W_mc, gamma, R = parts(small_agent)
    W0, t0 = ag.W.clone(), ag.t
    st0 = {f: getattr(ag.state, f).clone() for f in EnvState.FIELDS}
    gest0 = ag.gest_counts.clone()
    with spy_calls(ag.ctx) as (train_calls, _), spy_calls(ectx) as (eval_calls, _):
        report, W_new = ag.fit_values_to_returns(trajectory=traj, epsilon=0.5, seed=9, lam=LAM, sweeps=2, double=True, keep=True, ridge=RIDGE)
    torch.cuda.synchronize()
    return dict(report=report, W_new=W_new, W0=W0, t0=t0, st0=st0, gest0=gest0, train_calls=train_calls, eval_calls=eval_calls)


def test_optimism_is_zero_in_the_first_sweep_and_not_in_the_second(small_agent, double_fit):
    rep = double_fit["report"]
    assert len(rep["sweeps"]) == 2 and rep["lam"] == LAM and rep["trace"] == "peng" and rep["vf"] is rep["sweeps"][1]["vf"]
    for k in (0, 2):                                           # the value functions that run in the record
        first, second = rep["sweeps"][0]["vf"][k], rep["sweeps"][1]["vf"][k]
        assert first["optimism_n"] == second["optimism_n"] > 20
        assert first["optimism"] == 0.0, (k, first["optimism"])               # W_A = W_B: vs and v are one value, by bits
        assert second["optimism"] != 0.0 and np.isfinite(second["optimism"]), (k, second["optimism"])
        for s in (first, second):
            assert set(s) >= {"n", "delta_norm", "fit", "held_out", "mc", "folds", "optimism", "cut_share", "off_greedy", "horizon"}
            assert set(s["folds"]) == {"a", "b"} and s["held_out"]["new"]["n"] > 0 and s["mc"]["held_out"]["new"]["n"] == s["held_out"]["new"]["n"]
            assert s["n"] == [x + y for x, y in zip(s["folds"]["a"]["n"], s["folds"]["b"]["n"])]
            for fr in s["folds"].values():
                assert fr["fit"]["new"]["rmse"] < fr["fit"]["old"]["rmse"]     # a least-squares refit lowers its own fit error


def test_w_new_is_the_mean_table_of_the_reported_pair(small_agent, double_fit):
    rep, W_new = double_fit["report"], double_fit["W_new"]
    W_a, W_b = rep["double"]["W_a"], rep["double"]["W_b"]
    assert not torch.equal(W_a, W_b) and not torch.equal(W_a, double_fit["W0"])
    assert same32(W_new, mean_table(W_a, W_b))
    want = ((W_a.cpu().numpy().astype(np.float64) + W_b.cpu().numpy().astype(np.float64)) / 2).astype(np.float32)
    assert bits_equal(W_new.cpu().numpy(), want)
    for s in rep["sweeps"]:
        assert same32(s["W"], mean_table(s["W_a"], s["W_b"]))
    assert same32(rep["sweeps"][1]["W_a"], W_a) and same32(rep["sweeps"][1]["W"], W_new)
    assert same32(W_new[1], double_fit["W0"][1])               # value function 1 never runs: its rows keep their bits through the mean


def test_fold_a_is_a_direct_gram_and_ridge_solve_on_its_rows_and_the_ab_targets(small_agent, double_fit):
    ag, traj, flat, ectx, W_mc, gamma, R = parts(small_agent)
    rep = double_fit["report"]
    W = double_fit["W0"]
    ab = double_targets(ectx, flat, W, W.clone(), gamma, LAM, R, cut=False)       # sweep 1: both tables are W
    off = flat["offsets"]
    env = np.repeat(np.arange(len(off) - 1), np.diff(off))
    smp = np.nonzero(ab["sample"])[0]
    first = rep["sweeps"][0]
    for k in (0, 2):
        rows = smp[(flat["vf"][smp] == k) & (fold_of(env[smp]) == 0)]
        assert len(rows) > 10 and np.all(env[rows] % 4 == 0)
        w_new, n_a = direct_refit(ectx, flat, ab["y"], rows, W[k], ag.ctx.scale)
        assert first["vf"][k]["folds"]["a"]["n"] == [int(v) for v in n_a]
        assert bits_equal(first["W_a"][k].cpu().numpy(), w_new), k
        rows_b = smp[(flat["vf"][smp] == k) & (fold_of(env[smp]) == 1)]
        w_b, _ = direct_refit(ectx, flat, ab["y"], rows_b, W[k], ag.ctx.scale)   # (sweep 1: BA's targets are AB's)
        assert bits_equal(first["W_b"][k].cpu().numpy(), w_b) and not bits_equal(w_b, w_new), k
    # sweep 2's fold A against the kept AB targets of that sweep (W_A selects, W_B values)
    lt = rep["double_targets"]
    ab2 = double_targets(ectx, flat, first["W_a"], first["W_b"], gamma, LAM, R, cut=False)
    assert bits_equal(lt["AB"]["y"], ab2["y"]) and not bits_equal(lt["AB"]["y"], lt["BA"]["y"])
    rows = smp[(flat["vf"][smp] == 0) & (fold_of(env[smp]) == 0)]
    w_new, _ = direct_refit(ectx, flat, ab2["y"], rows, first["W_a"][0], ag.ctx.scale)
    assert bits_equal(rep["double"]["W_a"][0].cpu().numpy(), w_new)


def test_the_agent_is_left_as_evaluate_leaves_it(small_agent, double_fit):
    ag = small_agent[0]
    assert double_fit["train_calls"] == [], f"the double fit called into the training context: {double_fit['train_calls']}"
    assert torch.equal(ag.W, double_fit["W0"]) and ag.t == double_fit["t0"] and torch.equal(ag.gest_counts, double_fit["gest0"])
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(ag.state, f), double_fit["st0"][f]), f
    calls = double_fit["eval_calls"]
    assert "scg_row_values_cross" in calls and "scg_trace_returns" in calls and "scg_q_values" not in calls


def test_double_false_is_the_single_fit_and_the_refusals(small_agent):
    ag, traj, flat, ectx, W_mc, gamma, R = parts(small_agent)
    kw = dict(trajectory=traj, epsilon=0.5, seed=9, lam=LAM, ridge=RIDGE)
    with spy_calls(ectx) as (calls, _):
        rep, W_single = ag.fit_values_to_returns(double=False, **kw)
    _, W_default = ag.fit_values_to_returns(**kw)
    assert same32(W_single, W_default) and "double" not in rep and "scg_row_values_cross" not in calls
    # the single path as SPEC §27.3 states it, recomputed: lambda_targets under W, the even envs' rows, one refit per value function
    lt = lambda_targets(ectx, flat, ag.W, gamma, LAM, R)
    off = flat["offsets"]
    env = np.repeat(np.arange(len(off) - 1), np.diff(off))
    smp = np.nonzero(lt["sample"])[0]
    for k in (0, 1, 2):
        rows = smp[(flat["vf"][smp] == k) & (env[smp] % 2 == 0)]
        w_new, _ = direct_refit(ectx, flat, lt["y"], rows, ag.W[k], ag.ctx.scale)
        assert bits_equal(W_single[k].cpu().numpy(), w_new), k
    assert not torch.equal(W_single, ag.W)
    with pytest.raises(ScgError, match="double=True needs lam"):
        ag.fit_values_to_returns(trajectory=traj, double=True)
    with pytest.raises(ScgError, match="double=True needs lam"):
        ag.fit_values_to_returns(trajectory=traj, double=True, order=3)
    with pytest.raises(ScgError):
        ag.fit_values_to_returns(trajectory=traj, double=True, lam=LAM, order=3)
    rep_w, W_w = ag.fit_values_to_returns(double=True, trace="watkins", sweeps=2, **kw)      # both traces
    assert rep_w["trace"] == "watkins" and 0.0 < rep_w["vf"][0]["cut_share"] < 1.0 and rep_w["sweeps"][0]["vf"][0]["optimism"] == 0.0
    assert same32(W_w, mean_table(rep_w["double"]["W_a"], rep_w["double"]["W_b"])) and torch.equal(ag.W, small_agent[0].W)


def test_double_fit_report_runs_end_to_end_at_toy_size(tmp_path):
    from test_gpu_tools import tool
    out = tool("double_fit_report.py", "--maps", "pinball_simple", "--seeds", 1, "--envs", 256, "--warm", 40, "--after", 8, "--steps-per-option", 16,
               "--min-examples", 64, "--episodes", 64, "--options", 2, "--lambdas", 0.9, "--sweeps", 2, "--eval-episodes", 64,
               "--out-dir", tmp_path, "--check-dir", tmp_path).splitlines()
    assert out[0].startswith("# double_fit_report map pinball_simple envs 256 ")
    assert (tmp_path / "r35_double_fit_pinball_simple.txt").read_text().splitlines() == out
    rows = [ln.split() for ln in out if ln.startswith("    ") and ln.split()[0] in ("single", "double") and len(ln.split()) == 13]
    assert len(rows) == 2 * 2 * 2 * 3                          # two arms, two traces, two sweeps, three value functions
    assert all(r[11] == r[12] == "-" for r in rows if r[0] == "single") and all(int(r[12]) >= 0 for r in rows if r[0] == "double")
    first = [r for r in rows if r[0] == "double" and r[3] == "1" and int(r[5]) > 0]
    assert first and all(float(r[11]) == 0.0 for r in first)   # optimism of sweep 1: exactly 0
    assert any("drift check: no r34_trace_fit report" in ln for ln in out)
    pol = [ln.split() for ln in out if "+-" in ln and " table " not in ln]
    assert len(pol) == 2 * (1 + 2 * 2) * 2 and pol[0][0] == "W" and pol[-1][0] == "double/watkins/0.90/2"
    assert len([ln for ln in out if ln.startswith("  descent ")]) == 2 * 2 * 2
