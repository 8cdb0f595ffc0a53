"""SPEC §11 / §12 option interruption on the HIP path against the float64 model (tests/ref64.py): the interrupting learner over the
sweep of tests/test_ref64_interrupt.py on every block build, at the headline shape and past 256 workgroups, and at the named
edges of the rule; learning steps chained on one device state (the prepared and folded next env orders), interrupting and plain;
and one-step acting rollouts of SPEC §8 and §11 with their counters and record rows. The bit-exact tests tie the kernels to
emulators written from the same reading of the SPEC; these tie them to the SPEC."""
import numpy as np
import pytest
import torch

from gpu_util import block_build, block_envs, dev, host_state, state_to_device       # noqa: F401  (block_envs: the fixture)
from ref64 import U32, compare, env_order_layout
from skill_chaining_with_graphs_amd.core import EnvState, ScgContext
from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
from skill_chaining_with_graphs_amd.trajectory import Trajectory
from test_gpu_ref64 import GpuRunner
from test_ref64_interrupt import EDGES, INT_SWEEP, MAX_EP, MAX_OPT, case_ids, interrupt_sweep_case, seat_running_envs
from test_ref64_oracle import OracleRunner, assert_rarely_ambiguous, check_step, pre_state
from util import HP, chain_classifiers, crossing_weights, random_weights, wide_chain

pytestmark = pytest.mark.gpu


class IntGpuRunner(GpuRunner):
    """ScgContext.step(learn=True, apply=True, interrupt=True) from a pre-state copied to the device."""

    interrupt = True


GPU_CASES = [(c, b) for b in (256, 128, 64) for c in INT_SWEEP if b == 256 or c[1] <= 1000]


@pytest.mark.parametrize("cfg,block_envs", GPU_CASES, indirect=["block_envs"], ids=case_ids(GPU_CASES))
def test_hip_interrupting_step_matches_the_float64_model(cfg, block_envs):
    interrupt_sweep_case(IntGpuRunner, cfg, block_envs)


@pytest.mark.parametrize("n,steps", [(65536, 3), (70000, 1)])
@pytest.mark.parametrize("block_envs", [256], indirect=True)
def test_hip_interrupting_step_big_shapes(n, steps, block_envs):
    """The headline shape (65 536 envs, 5 options, 3 step-batches) and 70 000 envs: 274 workgroups, more than the CUs, the last
    one partial. Single-item resolution is lost at this size: exact n_k and exact discrete fields carry the per-item check."""
    nopt = 5
    r = IntGpuRunner("pinball_simple", n, nopt, seed=2024, env_id_base=0)
    clf = chain_classifiers(r.map, nopt)
    rng = np.random.default_rng(n)
    W = random_weights(nopt + 1, 77, std=1e-3)
    n_amb = n_int = 0
    for t in range(steps):
        pre = pre_state(r.map, n, nopt, rng, max_ep=MAX_EP, max_opt=MAX_OPT)
        seat_running_envs(r.map, pre, clf, r.model.parents, rng)
        out, _, a = check_step(r, pre, W, clf, t, 0b111110, msg=f"n={n} t={t}")
        n_amb += a
        n_int += int(out["interrupted"].sum())
    print(f"\n[big n={n}] {n_int} interrupted, {n_amb} ambiguous in {steps * n} env-steps")
    assert_rarely_ambiguous(n_amb, steps * n)
    assert n_int >= steps * n // 100
    if n == 70000:
        assert -(-n // block_envs) > 256 and n % block_envs != 0


@pytest.mark.parametrize("edge", EDGES, ids=[e.__name__[5:] for e in EDGES])
@pytest.mark.parametrize("block_envs", [256, 64], indirect=True)
def test_hip_interrupt_edge_case(edge, block_envs):
    edge(IntGpuRunner)


# ---------------------------------------------------------------------------------------------------- chained steps

CHAINS = [
    # map, envs, options, block, distribution of the ids, layout of the first pre-state
    ("pinball_simple", 4096, 5, 256, "uniform", "chunked"),
    ("pinball_simple", 300, 5, 64, "heavy", "padded"),
]


@pytest.mark.parametrize("interrupt", [True, False], ids=["interrupting", "plain"])
@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: f"n{c[1]}-b{c[3]}-{c[5]}")
def test_chained_steps_on_one_device_state(chain, interrupt):
    """Six learning step-batches on one EnvState and one W on the device. Each is checked against the model from the SUT's own
    post-state and W of the step before, read back: from the second step on, the kernel runs in the env order that the step before
    prepared (with interruption: the order it folded)."""
    name, n, nopt, block, dist, layout = chain
    with block_build(block):
        r = GpuRunner(name, n, nopt, seed=31, env_id_base=5, reoffer_period=4)
        clf = chain_classifiers(r.map, nopt)
        rng = np.random.default_rng(n + nopt)
        pre = pre_state(r.map, n, nopt, rng, max_ep=MAX_EP, max_opt=MAX_OPT, dist=dist)
        seat_running_envs(r.map, pre, clf, r.model.parents, rng, share=0.8)
        enabled = 0b111110
        st = state_to_device({k: pre[k] for k in EnvState.FIELDS}, r.ctx)
        W_d = dev(crossing_weights(nopt + 1, 31))
        Wv, cv = W_d.view(-1), dev(clf).view(-1)
        n_amb = n_int = n_keep = 0
        layouts = []
        for t in range(50, 56):
            pre, W = host_state(st), W_d.cpu().numpy()
            layouts.append(env_order_layout(pre["option_id"], nopt + 1, block))
            r.ctx.step(st, Wv, cv, enabled, t, learn=True, apply=True, interrupt=interrupt)
            torch.cuda.synchronize()
            got, ev, ev_len = host_state(st), r.trace[2].cpu().numpy(), r.trace[3].cpu().numpy()
            out = r.model.step(pre, W, clf, t, enabled, 0, sut=dict(got, events=ev), interrupt=interrupt)
            n_amb += compare(out, got, r.G.cpu().numpy(), r.n_k.cpu().numpy(), W_d.cpu().numpy(), events=ev, ev_len=ev_len,
                             msg=f"t={t}")
            n_int += int(out["interrupted"].sum())
            n_keep += int(out["keep"].sum())
    print(f"\n[chain n={n} B={block} interrupt={interrupt}] layouts {layouts}, {n_keep} kept, {n_int} interrupted, {n_amb} ambiguous")
    assert_rarely_ambiguous(n_amb, 6 * n)
    assert layouts[0] == layout
    assert n_keep >= 6 * n // 20
    assert n_int >= 6 * n // 100 if interrupt else n_int == 0


# ---------------------------------------------------------------------------------------------------- acting rollouts

def _onehot(idx, on, n_vf):
    z = np.zeros((n_vf, len(idx)), np.int64)
    z[np.clip(idx, 0, n_vf - 1), np.arange(len(idx))] += np.asarray(on, np.int64)
    return z


def _check_counters(out, s0, s1, ok, msg):
    """SPEC §8's counters of one step: the integer ones exactly, ep_return / ret_sum to the rounding of the binary32 sum."""
    n_vf = s0["vf_steps"].shape[0]
    o, cand = out["vf"], out["cand"]
    want = dict(vf_steps=_onehot(o, np.ones(len(o), bool), n_vf),
                entries=_onehot(cand, out["entering"] & ~out["declined"], n_vf),
                declines=_onehot(cand, out["declined"], n_vf),
                successes=_onehot(o, (o >= 1) & out["succ_o"], n_vf))
    for f, w in want.items():
        bad = ok & ((s1[f].astype(np.int64) - s0[f]) != w).any(0)
        assert not bad.any(), f"{msg} {f}: {bad.sum()} envs differ, first {np.nonzero(bad)[0][:5].tolist()}"
    done = out["done"] != 0
    for f, w in (("episodes", done), ("goals", out["done"] == 1), ("len_sum", np.where(done, out["ev_len"], 0))):
        bad = ok & ((s1[f].astype(np.int64) - s0[f]) != w)
        assert not bad.any(), f"{msg} {f}: {bad.sum()} envs differ"
    bad = ok & (s1["finished"] != (s0["finished"].astype(bool) | done))
    assert not bad.any(), f"{msg} finished: {bad.sum()} envs differ"
    r = s0["ep_return"].astype(np.float64) + out["reward"]
    tol = U32 * np.abs(r)
    got = s1["ep_return"].astype(np.float64)
    bad = ok & np.where(done, got != 0.0, np.abs(got - r) > tol)
    assert not bad.any(), f"{msg} ep_return: {bad.sum()} envs differ"
    d = s1["ret_sum"] - s0["ret_sum"] - np.where(done, r, 0.0)
    bad = ok & (np.abs(d) > tol + 2.0 ** -52 * np.abs(s1["ret_sum"]))
    assert not bad.any(), f"{msg} ret_sum: {bad.sum()} envs differ"


def _check_record(out, tr, ok, msg):
    """SPEC §10's one-row record: s' (before the reset), the action, reward, done, the VF that ran the step, the id written and
    the term code (5 exactly on the interrupted envs)."""
    assert (tr.len.cpu().numpy() == 1).all(), f"{msg} record len"
    want = dict(x=out["sp"][0], y=out["sp"][1], vx=out["sp"][2], vy=out["sp"][3], action=out["action"], reward=out["reward"],
                done=out["done"], vf=out["vf"], option_id=out["option_id"], term=out["term"])
    for f, w in want.items():
        got = getattr(tr, f)[0].cpu().numpy().astype(np.float64)
        bad = ok & (got != np.asarray(w, np.float64))
        assert not bad.any(), f"{msg} record {f}: {bad.sum()} envs differ, first {np.nonzero(bad)[0][:5].tolist()}"


@pytest.mark.parametrize("interrupt", [False, True], ids=["s8", "s11"])
@pytest.mark.parametrize("block,epw", [(256, 2), (256, 32), (64, 2), (64, 32)])
def test_one_step_rollouts_match_the_float64_model(block, epw, interrupt, monkeypatch):
    """One-step rollouts chained over several t on one state, under two pinned launch geometries and two block builds: the acting
    outputs, interrupts[o][e], SPEC §8's counters and the record rows against the model with learn=False."""
    monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
    n, nopt, gest, enabled = 3000, 4, 0b10000, 0b01110
    hp = dict(HP, reoffer_period=4)
    r = OracleRunner("pinball_simple", n, nopt, seed=41, env_id_base=9, gest=gest, **hp)   # the model and its borrowed physics
    ctx = ScgContext(n, nopt, r.map, device=0, seed=41, env_id_base=9, block_envs=block, **hp)
    ctx.set_gestation(gest)
    clf = wide_chain(r.map, nopt)
    rng = np.random.default_rng(block + epw)
    pre = pre_state(r.map, n, nopt, rng, max_ep=MAX_EP, max_opt=MAX_OPT)
    seat_running_envs(r.map, pre, clf, r.model.parents, rng, share=0.7)
    W = crossing_weights(nopt + 1, 41)
    st = state_to_device({k: pre[k] for k in EnvState.FIELDS}, ctx)
    Wv, cv = dev(W).view(-1), dev(clf).view(-1)
    stats = EpisodeStats(nopt + 1, n, ctx.device)
    intr = torch.zeros((nopt + 1, n), dtype=torch.int32, device=ctx.device) if interrupt else None
    n_amb = n_int = n_keep = n_ent = 0
    for t in range(700, 706):
        msg = f"block {block} epw {epw} t {t}:"
        pre = host_state(st)
        s0 = {f: getattr(stats, f).cpu().numpy().copy() for f in EpisodeStats.FIELDS}
        i0 = intr.cpu().numpy().copy() if interrupt else None
        tr = Trajectory(n, 1, 0, ctx.device)
        ctx.rollout(st, Wv, cv, enabled, t, 1, stats, record=tr, interrupt=interrupt, interrupts=intr)
        torch.cuda.synchronize()
        got = host_state(st)
        out = r.model.step(pre, W, clf, t, enabled, gest, sut=got, learn=False, interrupt=interrupt)
        n_amb += compare(out, got, None, None, None, msg=msg)
        ok = np.ones(n, bool)
        ok[out["ambiguous"]] = False
        _check_counters(out, s0, {f: getattr(stats, f).cpu().numpy() for f in EpisodeStats.FIELDS}, ok, msg)
        _check_record(out, tr, ok, msg)
        if interrupt:
            d = intr.cpu().numpy().astype(np.int64) - i0
            bad = ok & (d != _onehot(out["vf"], out["interrupted"], nopt + 1)).any(0)
            assert not bad.any(), f"{msg} interrupts: {bad.sum()} envs differ"
        n_int += int(out["interrupted"].sum())
        n_keep += int(out["keep"].sum())
        n_ent += int((out["entering"] & ~out["declined"]).sum())
    print(f"\n[rollout B={block} epw={epw} interrupt={interrupt}] {n_keep} kept, {n_int} interrupted, {n_ent} entries, "
          f"{n_amb} ambiguous")
    assert_rarely_ambiguous(n_amb, 6 * n)
    assert n_keep >= 6 * n // 20 and n_ent >= 50
    assert n_int >= 6 * n // 100 if interrupt else n_int == 0
