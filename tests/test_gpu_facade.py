"""The north_star façade (PinballDomain.step, FourierBasis.features, Option.{policy, beta, in_initiation_set,
initiation_classifier}, SkillChainingAgent.q_update) called the way a user of the package would, every result checked
against the CPU oracle — bit for bit (floats included)."""
import numpy as np
import pytest
import torch

import option_rules as rules
import sc_oracle
from util import HP, SCALE, chain_classifiers, random_states, random_weights

pytestmark = pytest.mark.gpu
N, NOPT, MASK = 700, 2, 0b110


@pytest.fixture(scope="module")
def agent():
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    ag = SkillChainingAgent("pinball_simple", N, NOPT, seed=3, **HP)
    ag.clf.copy_(torch.as_tensor(chain_classifiers(ag.map, NOPT), device="cuda:0"))
    ag.enabled_mask = MASK
    ag.W.copy_(torch.as_tensor(random_weights(NOPT + 1, 8, std=0.1), device="cuda:0"))
    return ag


@pytest.fixture(scope="module")
def orc(agent):
    return sc_oracle.Oracle(agent.map, SCALE, n_envs=N, n_options=NOPT, seed=3, enabled_mask=MASK, **HP)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def test_pinball_domain_step(agent, orc):
    x, y, vx, vy = random_states(agent.map, N, 41, vmax=2.0)
    act = np.random.default_rng(42).integers(0, 5, N).astype(np.uint8)
    st = agent.state
    for name, v in (("x", x), ("y", y), ("vx", vx), ("vy", vy)):
        getattr(st, name).copy_(_dev(v))
    reward, goal = agent.domain.step(_dev(act))
    r_o, g_o = orc.pinball_step(x, y, vx, vy, act)                   # in place on the numpy arrays
    assert np.array_equal(reward.cpu().numpy(), r_o) and np.array_equal(goal.cpu().numpy(), g_o)
    for name, v in (("x", x), ("y", y), ("vx", vx), ("vy", vy)):
        assert np.array_equal(getattr(st, name).cpu().numpy(), v), name


def test_fourier_basis_features(agent, orc):
    from skill_chaining_with_graphs_amd import FourierBasis
    fb = FourierBasis(agent.ctx)
    x, y, vx, vy = random_states(agent.map, 64, 43, vmax=2.0)
    phi = fb.features(tuple(_dev(v) for v in (x, y, vx, vy)))
    assert fb.num_features == 1296 and tuple(phi.shape) == (64, 1296)
    assert np.array_equal(phi.cpu().numpy(), orc.features(x, y, vx, vy))
    assert fb.coefficients[1295].tolist() == [5, 5, 5, 5] and fb.coefficients[37].tolist() == [0, 1, 0, 1]


def test_option_policy_and_q_values(agent, orc):
    x, y, vx, vy = random_states(agent.map, N, 44, vmax=2.0)
    s = tuple(_dev(v) for v in (x, y, vx, vy))
    W = agent.W.cpu().numpy()
    for k in range(NOPT + 1):
        q_o = orc.q_values(x, y, vx, vy, W[k])
        assert np.array_equal(agent.options[k].q_values(s).cpu().numpy(), q_o)
        assert np.array_equal(agent.options[k].policy(s).cpu().numpy(), np.argmax(q_o, axis=0).astype(np.uint8))


def test_option_initiation_set_and_beta(agent, orc):
    rng = np.random.default_rng(45)
    x, y = rng.random(N).astype(np.float32), rng.random(N).astype(np.float32)
    goal = (rng.random(N) < 0.1).astype(np.uint8)
    done = np.where(goal == 1, 1, np.where(rng.random(N) < 0.05, 2, 0)).astype(np.uint8)
    steps = rng.integers(0, HP["max_option_steps"] + 2, N).astype(np.int32)
    clf = agent.clf.cpu().numpy()
    inset = rules.membership(lambda px, py, k: orc.classifier_predict(px, py, clf[k]), x, y, NOPT + 1, MASK)
    xd, yd = _dev(x), _dev(y)
    assert np.array_equal(agent.options[0].in_initiation_set(xd, yd).cpu().numpy(), np.ones(N, np.uint8))
    for k in (1, 2):
        assert np.array_equal(agent.options[k].in_initiation_set(xd, yd).cpu().numpy().astype(bool), inset[k])
        # SPEC §4.2 on the oracle's classifier outputs (the chain's parents: k -> k - 1)
        want = rules.option_end(inset, goal, done, np.full(N, k), steps, [0, 0, 1], MASK, HP["max_option_steps"])["term"]
        got = agent.options[k].beta(xd, yd, goal=_dev(goal), done=_dev(done), opt_steps=_dev(steps))
        assert np.array_equal(got.cpu().numpy().astype(bool), want), k
    got0 = agent.options[0].beta(xd, yd, goal=_dev(goal), done=_dev(done))
    assert np.array_equal(got0.cpu().numpy().astype(bool), (done != 0) | goal.astype(bool))


def test_beta_agrees_with_the_fused_step(agent, orc):
    """Option.beta on the fused step's own outputs must reproduce the step's keep/terminate decision: an env that ran
    option k keeps running it (option_id stays k and opt_steps advances) iff beta == 0."""
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    ag = SkillChainingAgent("pinball_simple", 2048, NOPT, seed=11, **HP)
    ag.clf.copy_(agent.clf); ag.enabled_mask = MASK
    ag.W.copy_(agent.W)
    ag.domain.reset_random(seed=5, v_max=1.0)
    seen = 0
    for _ in range(30):
        st = ag.state
        o_before, steps_before = st.option_id.clone(), st.opt_steps.clone()
        ep_before = st.ep_steps.clone()
        ag.step_batch()
        # post-physics state s': equals the committed state except for envs that were reset (done != 0)
        live = st.done == 0
        for k in (1, 2):
            ran = (o_before == k) & live
            if int(ran.sum()) == 0:
                continue
            b = ag.options[k].beta(st.x, st.y, goal=(st.done == 1).to(torch.uint8), done=st.done, opt_steps=steps_before)
            kept = (st.option_id == k) & (st.opt_steps == steps_before + 1)
            assert torch.equal(kept[ran], b[ran] == 0), k
            seen += int(ran.sum())
        assert torch.equal(st.ep_steps[live], ep_before[live] + 1)
    assert seen > 100


def test_agent_q_update(agent, orc):
    x, y, vx, vy = random_states(agent.map, N, 46, vmax=2.0)
    xn, yn, vxn, vyn = random_states(agent.map, N, 47, vmax=2.0)
    rng = np.random.default_rng(48)
    act = rng.integers(0, 5, N).astype(np.uint8)
    r = rng.normal(size=N).astype(np.float32)
    cont = np.where(rng.random(N) < 0.2, 0.0, HP["gamma"]).astype(np.float32)
    W0 = agent.W.clone()
    W = W0.cpu().numpy().copy()
    G, cnt = orc.q_update_grad((x, y, vx, vy), act, r, cont, (xn, yn, vxn, vyn), W[1])
    Gk = np.zeros_like(W); Gk[1] = G
    nk = np.zeros(NOPT + 1, np.int32); nk[1] = cnt
    orc.apply(W, Gk, nk)
    agent.q_update(1, tuple(_dev(v) for v in (x, y, vx, vy)), _dev(act), _dev(r), _dev(cont),
                   tuple(_dev(v) for v in (xn, yn, vxn, vyn)))
    assert cnt == N and np.array_equal(agent.W.cpu().numpy(), W)
    agent.W.copy_(W0)
