"""SkillChainingAgent.fit_values_lstdq (SPEC §17) on tests/test_gpu_value_fit.py's 256-env agent with one enabled option on the rig's
dense map: its items, greedy next actions and TD residuals against the scalar model of §17.2, each (A, b, C) it formed against the
host models of §16.1 / §17.1, its weights against the block system reassembled in float64, rounds, gamma = 0, rows without
samples, apply=False / apply=True, and the report tool at toy size."""
import gc

import numpy as np
import pytest
import torch

import cross_gram_model as CM
import gram_model as GM
from bits import assert_bits_equal
from gpu_util import crossing_agent, dev, gestating_agent, spy_calls
from skill_chaining_with_graphs_amd.agent import SkillChainingAgent
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd import ScgError, _lib, valuefit
from test_gpu_tools import tool
from test_gram_host import RESIDUAL_RATIO_BOUND
from util import HP, SCALE, dense_map, disc_weights, make_oracle

pytestmark = pytest.mark.gpu

NF, NA = 1296, 5
N_EPISODES, RIDGE, EPS = 256, 1e-3, 0.5
RUN, IDLE = (0, 2), 1            # the value functions that run in the record, and the one that never does
IDX = GM.index_set(_lib.CROSS_GRAM_MACRO_TILE)
assert _lib.CROSS_GRAM_MACRO_TILE == _lib.GRAM_MACRO_TILE          # (one index set serves A and C)


@pytest.fixture(scope="module", autouse=True)
def cached_blocks_go_back():
    """Later modules find torch's allocator as they would without this one (tests/test_gpu_robustness.py counts on a 64 MiB request
    getting a segment of its own). A device torch.linalg.solve leaves torch's BLAS workspace behind, a live 128 MiB block in a
    208 MiB segment whose free rest would serve that request: it is released when the module is done, and so are the cached
    blocks (every fit's C is 168 MB)."""
    yield
    torch._C._cuda_clearCublasWorkspaces()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def fitted():
    """test_gpu_value_fit.py's agent (option 2 enabled and offered at the start, succeeding when the ball leaves a small disc
    round it; option 1 gestating, so value function 1 never runs; random W; half the actions random) and one two-round fit with
    everything kept."""
    m = dense_map()
    ag = SkillChainingAgent(m, 256, 2, seed=5, block_envs=256, **dict(HP, max_episode_steps=63))
    ag.init_weights(std=0.05, seed=3)
    sx, sy = (float(v) for v in m.starts[0])
    clf = np.zeros((3, 8), np.float32)
    clf[1], clf[2] = -disc_weights(sx, sy, 0.04), disc_weights(0.5, 0.5, 1.5)
    ag.clf.copy_(dev(clf))
    ag.enable_option(2)
    ag.gest_mask = 0b010
    ag.gest_counts = ag.ctx.set_gestation(ag.gest_mask)
    W0 = ag.W.clone()
    report, W_new = ag.fit_values_lstdq(n_episodes=N_EPISODES, epsilon=EPS, seed=9, ridge=RIDGE, rounds=2, keep=True)
    torch.cuda.synchronize()
    orc, _ = make_oracle("pinball_simple")
    yield dict(ag=ag, W0=W0, report=report, W_new=W_new, orc=orc, gamma=float(ag.ctx.cfg.gamma), r_succ=float(ag.ctx.cfg.r_option_success))
    ag.ctx.close()


def ops(fitted, k, rnd=0):
    return fitted["report"]["rounds"][rnd]["vf"][k]["operands"]


def test_the_record_exercises_every_kind(fitted):
    rep = fitted["report"]
    rows = np.diff(rep["trajectory"].to_numpy()["offsets"])
    assert rows.max() <= 64 and rows.mean() > 16
    kinds = {k: rep["rounds"][0]["vf"][k]["kinds"] for k in (0, 1, 2)}
    print(f"kinds per value function: {kinds}; solve seconds {[round(t, 2) for t in rep['solve_seconds']]}")
    assert kinds[0]["CONT"] > 1000 and kinds[0]["END"] == N_EPISODES and kinds[0]["BOOT"] == 0      # every episode ends once; the root never boots
    assert kinds[2]["CONT"] > 300 and kinds[2]["BOOT"] > 100, "option 2 must run and end while the episode goes on"
    assert kinds[IDLE] == {"CONT": 0, "BOOT": 0, "END": 0}
    assert torch.equal(fitted["ag"].W, fitted["W0"]) and len(rep["rounds"]) == 2


@pytest.mark.parametrize("k", RUN)
def test_items_next_actions_and_residuals_equal_the_scalar_model(fitted, k):
    op, flat = ops(fitted, k), fitted["report"]["trajectory"].to_numpy()
    off = flat["offsets"]
    want = {}
    for e in range(N_EPISODES):
        sl = slice(off[e], off[e + 1])
        for j, kind, r in CM.scalar_items(flat["reward"][sl], flat["done"][sl], flat["vf"][sl], flat["term"][sl], k, fitted["r_succ"]):
            want[int(off[e]) + j] = (e, kind, r)
    rows, n_fit = op["rows"], op["n_fit"]
    assert sorted(rows.tolist()) == sorted(want) and len(set(rows.tolist())) == len(rows)
    assert [want[i][1] for i in rows.tolist()] == op["kind"].tolist() and [want[i][2] for i in rows.tolist()] == op["r"].tolist()
    env = np.array([want[i][0] for i in rows.tolist()])
    assert np.all(env[:n_fit] % 2 == 0) and np.all(env[n_fit:] % 2 == 1) and np.all(np.diff(rows[n_fit:]) > 0)
    assert np.array_equal(op["action"], flat["action"][rows])
    for a in range(NA):                                              # the fit samples by action, (env, row) order within one
        seg = rows[op["offsets"][a]: op["offsets"][a + 1]]
        assert np.all(flat["action"][seg] == a) and np.all(np.diff(seg) > 0)
    for f, t, t2 in zip(("x", "y", "vx", "vy"), op["states"], op["next_states"]):
        assert np.array_equal(t.cpu().numpy(), flat[f][rows - 1]) and np.array_equal(t2.cpu().numpy(), flat[f][rows])
    # a' and delta, with the oracle's Q
    s, s2 = ([t.cpu().numpy() for t in op[name]] for name in ("states", "next_states"))
    W0 = fitted["W0"].cpu().numpy()
    q, qn, q0 = fitted["orc"].q_values(*s, W0[k]), fitted["orc"].q_values(*s2, W0[k]), fitted["orc"].q_values(*s2, W0[0])
    model = [CM.scalar_residual(op["r"][i], op["kind"][i], fitted["gamma"], q[op["action"][i], i], qn[:, i], q0[:, i]) for i in range(len(rows))]
    assert op["a2"].tolist() == [v[0] for v in model]
    assert_bits_equal(op["delta"], np.array([v[1] for v in model], np.float32), msg=f"vf {k}: delta:")
    # the CONT fit samples by (a, a'), (env, row) order within a pair
    cont = [i for i in range(n_fit) if op["kind"][i] == CM.CONT]
    assert op["c_index"].tolist() == sorted(cont, key=lambda i: (op["action"][i], op["a2"][i], rows[i]))
    sizes = np.bincount(NA * op["action"][cont] + op["a2"][cont], minlength=NA * NA)
    assert np.array_equal(op["c_offsets"], np.concatenate([[0], np.cumsum(sizes)]))
    print(f"vf {k}: (a, a') segment sizes {sizes.tolist()}")


@pytest.mark.parametrize("k", RUN)
def test_operands_equal_the_host_models(fitted, k):
    op = ops(fitted, k)
    phi, phi2 = (fitted["orc"].features(*[t.cpu().numpy() for t in op[name]]) for name in ("states", "next_states"))
    A, b, Cm = op["A"].cpu().numpy(), op["b"].cpu().numpy(), op["C"].cpu().numpy()
    assert_bits_equal(A[np.ix_(range(NA), IDX, IDX)], GM.gram(phi, op["offsets"], IDX, IDX), msg=f"vf {k}: A on the index set:")
    assert_bits_equal(b, GM.rhs(phi, op["delta"], op["offsets"]), msg=f"vf {k}: b:")
    ci = op["c_index"]
    assert Cm.shape == (NA * NA, NF, NF)
    assert_bits_equal(Cm[np.ix_(range(NA * NA), IDX, IDX)], CM.cross(phi[ci], phi2[ci], op["c_offsets"], IDX, IDX), msg=f"vf {k}: C on the index set:")


def system(op, n, gamma, ridge):
    """SPEC §17.3's M and right-hand side over the actions with samples, reassembled in float64 from the kept operands."""
    A, Cm = op["A"].cpu().numpy(), op["C"].cpu().numpy().reshape(NA, NA, NF, NF)
    act = [a for a in range(NA) if n[a] > 0]
    M = np.zeros((len(act) * NF, len(act) * NF))
    for i, a in enumerate(act):
        for j, a2 in enumerate(act):
            M[i * NF:(i + 1) * NF, j * NF:(j + 1) * NF] = -gamma * Cm[a, a2].astype(np.float64)
        M[i * NF:(i + 1) * NF, i * NF:(i + 1) * NF] += A[a].astype(np.float64) + np.diag(ridge * max(n[a], 1) / SCALE.astype(np.float64) ** 2)
    return M, np.concatenate([op["b"].cpu().numpy()[a].astype(np.float64) for a in act]), act


@pytest.mark.parametrize("k", RUN)
def test_weights_satisfy_the_block_system(fitted, k):
    """The blocks are the kernels' A and C (tied to the models by test_operands_equal_the_host_models); the residual bound is
    test_gram_host's ratio on eps 6480 (||M|| ||Delta|| + ||b||): partial-pivoting LU is backward stable like the Cholesky that
    ratio was first measured on."""
    rep = fitted["report"]["rounds"][0]["vf"][k]
    op = rep["operands"]
    M, rhs, act = system(op, rep["n"], fitted["gamma"], RIDGE)
    x = np.concatenate([op["Delta"][a] for a in act])
    res = np.linalg.norm(M @ x - rhs)
    scale = np.finfo(np.float64).eps * NA * NF * (np.linalg.norm(M) * np.linalg.norm(x) + np.linalg.norm(rhs))
    print(f"vf {k}: actions {act} residual ratio {res / scale:.3g} (bound {RESIDUAL_RATIO_BOUND:.3g}), reported {rep['solve_residual']:.3g}")
    assert res <= RESIDUAL_RATIO_BOUND * scale
    assert rep["solve_residual"] == pytest.approx(res / (np.linalg.norm(M) * np.linalg.norm(x) + np.linalg.norm(rhs)), rel=1e-6)
    w_old = fitted["W0"][k].cpu().numpy()
    W1 = fitted["report"]["rounds"][0]["W"]
    assert_bits_equal(W1[k].cpu().numpy(), (w_old.astype(np.float64) + op["Delta"]).astype(np.float32), msg="W after round 0:")
    assert rep["delta_norm"] > 0 and rep["fit"]["td"]["old"]["n"] == sum(rep["n"]) and rep["held_out"]["td"]["old"]["n"] > 0
    assert rep["a_changed"] is None and 0.0 <= fitted["report"]["rounds"][1]["vf"][k]["a_changed"] <= 1.0
    td, mc = rep["held_out"]["td"], rep["held_out"]["mc"]
    print(f"vf {k}: held-out TD rms {td['old']['rmse']:.2f} -> {td['new']['rmse']:.2f}, MC rmse {mc['old']['rmse']:.2f} -> {mc['new']['rmse']:.2f}")


def test_rows_without_samples_keep_their_bits(fitted):
    for rnd in fitted["report"]["rounds"]:
        assert torch.equal(rnd["W"][IDLE], fitted["W0"][IDLE]) and rnd["vf"][IDLE]["delta_norm"] == 0.0
    assert torch.equal(fitted["W_new"], fitted["report"]["rounds"][1]["W"])
    assert all(not torch.equal(fitted["W_new"][k], fitted["W0"][k]) for k in RUN)


def test_two_rounds_equal_two_calls_chained_by_hand(fitted):
    ag, rep = fitted["ag"], fitted["report"]
    r2, W2 = ag.fit_values_lstdq(epsilon=EPS, seed=9, ridge=RIDGE, rounds=1, keep=True, trajectory=rep["trajectory"], weights=rep["rounds"][0]["W"])
    assert torch.equal(W2, fitted["W_new"]) and torch.equal(ag.W, fitted["W0"])
    for k in RUN:
        a, b = r2["rounds"][0]["vf"][k]["operands"], ops(fitted, k, 1)
        assert np.array_equal(a["a2"], b["a2"]) and np.array_equal(a["c_index"], b["c_index"])
        assert_bits_equal(a["delta"], b["delta"], msg=f"vf {k}: delta of the second round:")
        assert torch.equal(a["A"], b["A"]) and torch.equal(a["A"], ops(fitted, k, 0)["A"]) and torch.equal(a["b"], b["b"]) and torch.equal(a["C"], b["C"])
        assert not np.array_equal(b["delta"], ops(fitted, k, 0)["delta"])       # (the second round is another system)


def test_gamma_zero_is_the_ridge_fit_on_the_one_step_rewards(fitted):
    """gamma = 0 through the hyper-parameters: delta = r - Q(s, a), C drops out, and Delta is §16.3's solve of (A, b). LU and
    Cholesky are backward stable: each is within c F eps cond of the exact solution (c = 8 taken for each; cond computed)."""
    ag, k = fitted["ag"], 2
    try:
        ag.ctx.set_hparams(gamma=0.0)
        rep, W_new = ag.fit_values_lstdq(epsilon=EPS, seed=9, ridge=RIDGE, vfs=[k], keep=True, trajectory=fitted["report"]["trajectory"])
    finally:
        ag.ctx.set_hparams(gamma=HP["gamma"])
    op, n = rep["rounds"][0]["vf"][k]["operands"], rep["rounds"][0]["vf"][k]["n"]
    assert rep["gamma"] == 0.0
    s = [t.cpu().numpy() for t in op["states"]]
    q = fitted["orc"].q_values(*s, fitted["W0"][k].cpu().numpy())
    assert_bits_equal(op["delta"], (op["r"] - q[op["action"], np.arange(len(s[0]))].astype(np.float64)).astype(np.float32), msg="delta at gamma = 0:")
    assert torch.equal(op["A"], ops(fitted, k)["A"])
    A, b = op["A"].cpu().numpy(), op["b"].cpu().numpy()
    want = valuefit.ridge_solve(A, b, n, RIDGE, SCALE)
    for a in range(NA):
        if n[a]:
            cond = np.linalg.cond(A[a].astype(np.float64) + np.diag(RIDGE * n[a] / SCALE.astype(np.float64) ** 2))
            err = np.linalg.norm(op["Delta"][a] - want[a]) / np.linalg.norm(want[a])
            print(f"action {a}: n {n[a]} cond {cond:.3g} relative difference {err:.3g}")
            assert err <= 16 * NF * np.finfo(np.float64).eps * cond
    assert torch.equal(W_new[0], fitted["W0"][0]) and not torch.equal(W_new[k], fitted["W0"][k])


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
        report, W_new = a.fit_values_lstdq(n_episodes=64, seed=2)
    torch.cuda.synchronize()
    assert calls == [], f"fit_values_lstdq called into the training context: {calls}"
    assert torch.equal(a.W, W0) and a.t == t0 and not torch.equal(W_new, W0)
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(a.state, f), st0[f]), f
    if ring0 is not None:
        assert all(torch.equal(x, y) for x, y in zip(a.trace, ring0))
    if gest0 is not None:
        assert torch.equal(a.gest_counts, gest0)
    a.step_batch()                                                   # ... and the run goes on
    assert a.t == t0 + 1


def test_apply_true_changes_exactly_the_listed_rows_and_refusals(fitted):
    ag, W0 = fitted["ag"], fitted["W0"]
    try:
        report, W_new = ag.fit_values_lstdq(epsilon=EPS, seed=9, ridge=RIDGE, vfs=[2], apply=True, trajectory=fitted["report"]["trajectory"])
        assert set(report["rounds"][0]["vf"]) == {2}
        assert torch.equal(ag.W[0], W0[0]) and torch.equal(ag.W[1], W0[1])
        assert torch.equal(ag.W[2], fitted["report"]["rounds"][0]["W"][2]) and torch.equal(W_new[2], ag.W[2]) and torch.equal(W_new[0], W0[0])
        ag.W.copy_(W0)
        with pytest.raises(ValueError):
            ag.fit_values_lstdq(n_episodes=N_EPISODES, vfs=[3])
        with pytest.raises(ValueError):
            ag.fit_values_lstdq(n_episodes=N_EPISODES, rounds=0)
        bad = W0.clone()
        bad[0].view(-1)[7] = float("inf")
        with pytest.raises(ScgError, match="non-finite"):              # W^o_0 is every option's BOOT row: refused for vfs=[2] too
            ag.fit_values_lstdq(vfs=[2], trajectory=fitted["report"]["trajectory"], weights=bad, apply=True)
        assert torch.equal(ag.W, W0)
        ag.group = object()                                          # shared weights: refused before anything runs
        with pytest.raises(ScgError, match="shared weights"):
            ag.fit_values_lstdq(n_episodes=N_EPISODES, apply=True)
    finally:
        ag.group = None
        ag.W.copy_(W0)


def test_lstdq_report_runs_end_to_end_at_toy_size(tmp_path):
    out = tool("lstdq_report.py", "--maps", "pinball_simple", "--seeds", 1, "--envs", 256, "--warm", 40, "--after", 8,
               "--steps-per-option", 16, "--min-examples", 64, "--states", 128, "--episodes", 128, "--options", 2, "--record-envs", 16,
               "--rounds", 1, "--out-dir", tmp_path).splitlines()
    assert out[0].startswith("# lstdq_report map pinball_simple envs 256 ")
    assert out[1].startswith("seed 1: ")
    assert (tmp_path / "r23_lstdq_pinball_simple.txt").read_text().splitlines() == out
    assert sum(ln.startswith("  lstdq round ") for ln in out) == 1 and sum(ln.startswith("  mc fit: ") for ln in out) == 1
    for name in ("before", "lstdq 1", "mc fit"):
        assert any(ln.startswith(f"  {name:<11s} success ") for ln in out), name
    rows = [ln.split() for ln in out if ln.startswith("    vf ") and ln.split()[1].isdigit()]
    assert len(rows) == 6 and sorted(len(r) for r in rows) == [11] * 3 + [16] * 3
