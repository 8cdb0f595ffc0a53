"""SPEC §31.3: fit_values_to_returns(solver="device") — the refit's normal equations solved by scg_ridge_solve, A and b left on the
device — equals, by bits in W_new and every sweep's W, the host path with tests/ridge_model.py in the place of valuefit.ridge_solve:
under both pipelines, under fresh=True and at a basis order. solver="host" is the path without the keyword; another name is refused;
apply=False leaves the agent alone."""
import hashlib

import numpy as np
import pytest
import torch

import ridge_model as R
from skill_chaining_with_graphs_amd import ScgError, valuefit
from gpu_util import assert_same_bits, clone_state, spy_calls
from test_gpu_fit_pipeline import bits, numbers
from test_gpu_lambda_returns import small_agent          # noqa: F401  (the fixture: 64 episodes at epsilon = 0.5, seed 9)

pytestmark = pytest.mark.gpu

KEPT = dict(epsilon=0.5, seed=9)
FIT = dict(lam=0.9, sweeps=2)
_solved = {}


def model_ridge_solve(A, b, n, ridge, scale, device=None):
    """valuefit.ridge_solve's signature on the model (tensors are downloaded); a system met before — the two pipelines form the
    same ones — is not solved again."""
    A, b = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (A, b))
    key = hashlib.sha1(A.tobytes() + b.tobytes() + np.asarray(n, np.int64).tobytes() + np.float64(ridge).tobytes()).hexdigest()
    if key not in _solved:
        _solved[key] = R.ridge_solve_like_valuefit(A, b, n, ridge, scale)
    return _solved[key].copy()


def restated(ag, monkeypatch, **kw):
    """The host path with the model in the place of valuefit.ridge_solve."""
    with monkeypatch.context() as mp:
        mp.setattr(valuefit, "ridge_solve", model_ridge_solve)
        return ag.fit_values_to_returns(solver="host", **kw)


def assert_same_fit(got, want):
    (rep_g, W_g), (rep_w, W_w) = got, want
    assert torch.equal(bits(W_g), bits(W_w))
    assert len(rep_g["sweeps"]) == len(rep_w["sweeps"])
    for s_g, s_w in zip(rep_g["sweeps"], rep_w["sweeps"]):
        assert torch.equal(bits(s_g["W"]), bits(s_w["W"]))
        assert numbers(s_g["vf"]) == numbers(s_w["vf"])


@pytest.mark.parametrize("pipeline", ["host", "device"])
def test_device_solver_equals_the_model_in_the_host_path(small_agent, monkeypatch, pipeline):
    ag, report, _ = small_agent
    traj = report["trajectory"]
    W0, t0, st0 = ag.W.clone(), ag.t, clone_state(ag.state)
    ectx = ag._eval_context(traj.n, 0.5, 9, None)[0]
    with spy_calls(ectx) as (calls, _):
        got = ag.fit_values_to_returns(trajectory=traj, pipeline=pipeline, solver="device", apply=False, **FIT, **KEPT)
    torch.cuda.synchronize()
    assert calls.count("scg_ridge_solve") == 2 * ag.n_vf, "one batched solve per sweep and table"
    assert torch.equal(ag.W, W0) and ag.t == t0, "apply=False must leave the agent's tables and step counter alone"
    assert_same_bits(ag.state, st0, msg="apply=False: training state")
    assert not torch.equal(got[1][0], W0[0]) and not torch.equal(got[1][2], W0[2])
    assert sum(got[0]["vf"][0]["n"]) > 100 and sum(got[0]["vf"][2]["n"]) > 20, "both value functions must run"
    assert_same_fit(got, restated(ag, monkeypatch, trajectory=traj, pipeline=pipeline, **FIT, **KEPT))
    for k, rep_k in got[0]["sweeps"][0]["vf"].items():         # an action without samples keeps its row bit for bit
        for a, n_a in enumerate(rep_k["n"]):
            if n_a == 0:
                assert torch.equal(bits(got[0]["sweeps"][0]["W"][k][a]), bits(W0[k][a])), (k, a)


def test_device_solver_under_fresh_records(small_agent, monkeypatch):
    ag, report, _ = small_agent
    traj = report["trajectory"]
    kw = dict(trajectory=traj, n_episodes=64, fresh=True, trace="watkins", **FIT, **KEPT)
    got = ag.fit_values_to_returns(solver="device", **kw)
    assert_same_fit(got, restated(ag, monkeypatch, **kw))
    assert got[0]["sweeps"][1]["episodes"]["episodes"] == 64


def test_device_solver_at_a_basis_order(small_agent, monkeypatch):
    ag, report, _ = small_agent
    traj = report["trajectory"]
    ectx = ag._eval_context(traj.n, 0.5, 9, None)[0]
    with spy_calls(ectx) as (calls, _):
        rep_d, W_d = ag.fit_values_to_returns(trajectory=traj, order=3, solver="device", **KEPT)
    assert calls.count("scg_ridge_solve") == len(rep_d["vf"])
    rep_m, W_m = restated(ag, monkeypatch, trajectory=traj, order=3, **KEPT)
    assert numbers(rep_d["vf"]) == numbers(rep_m["vf"]) and torch.equal(bits(W_d), bits(W_m))
    for k in rep_m["vf"]:
        d, m = rep_d["vf"][k]["delta"], rep_m["vf"][k]["delta"]
        assert d.shape == (5, 256) and np.array_equal(d.view(np.uint8), m.view(np.uint8)), k
    assert any(np.abs(rep_d["vf"][k]["delta"]).max() > 0 for k in rep_d["vf"])


def test_host_solver_is_the_path_without_the_keyword(small_agent):
    ag, report, _ = small_agent
    traj = report["trajectory"]
    ectx = ag._eval_context(traj.n, 0.5, 9, None)[0]
    kw = dict(trajectory=traj, lam=0.9, sweeps=2, **KEPT)
    rep_0, W_0 = ag.fit_values_to_returns(**kw)
    with spy_calls(ectx) as (calls, _):
        rep_h, W_h = ag.fit_values_to_returns(solver="host", **kw)
    assert "scg_ridge_solve" not in calls
    assert_same_fit((rep_h, W_h), (rep_0, W_0))
    # LAPACK's order is not the pinned one: close, not equal. Both solutions of a system of condition <= 1e6 (SPEC §31.4: 1e3 - 1e5)
    # with backward errors of 1e-16 lie within 1e-9 |Delta| of each other, so a first sweep's rows differ by that and one rounding
    # to binary32 of the row's entry.
    rep_d, _ = ag.fit_values_to_returns(solver="device", **kw)
    W1_d, W1_h = rep_d["sweeps"][0]["W"].double(), rep_h["sweeps"][0]["W"].double()
    slack = 2.0 ** -23 * W1_h.abs().max().item() + 1e-9 * (W1_h - ag.W.double()).abs().max().item()
    assert (W1_d - W1_h).abs().max().item() <= slack and len(rep_d["sweeps"]) == 2


def test_an_unknown_solver_is_refused(small_agent):
    ag, report, _ = small_agent
    for name in ("gpu", "torch", None, ""):
        with pytest.raises(ScgError, match="solver must be 'host' or 'device'"):
            ag.fit_values_to_returns(trajectory=report["trajectory"], lam=0.9, solver=name, **KEPT)
