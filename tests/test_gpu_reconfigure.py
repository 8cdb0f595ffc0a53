"""A context that is reconfigured while it is live equals a fresh one, bit for bit.

`scg_set_hparams`, `scg_set_map`, `scg_set_option_parents` and `scg_set_gestation` may be called between steps. A context that has
stepped carries an env order prepared by its last learning step, warm histogram buffers, cached step arguments on the Python side,
edge rows beyond a smaller map's edge count, a re-allocated start list and a rewritten cell-mask table. Here context A runs two
learning steps under settings S1, is reconfigured to S2 and goes on ON ITS OWN STATE (so that the prepared order and the cached
arguments are in use); context B is created with S2 and gets clones of A's state, weights, trace buffers and gestation counts.
The next steps of both must agree in every array: the state, qcache, action / reward / done, G, n_k, W, the ring, events / ev_len
and the gestation counts. Two contexts can be wrong in the same way, so every step of A is also held to the float64 model
(tests/ref64.py) built with S2. The same for the rollout and trial launches, which take their parameters the same way."""
import numpy as np
import pytest
import torch

import sc_oracle
import skill_chaining_with_graphs_amd as scg
from gpu_util import dev
from ref64 import StepModel, compare
from skill_chaining_with_graphs_amd.core import EnvState, ScgContext
from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
from skill_chaining_with_graphs_amd.trajectory import Trajectory
from skill_chaining_with_graphs_amd.trials import TrialResult
from test_ref64_interrupt import seat_running_envs
from test_ref64_oracle import assert_rarely_ambiguous, pre_state
from util import HP, SCALE, chain_classifiers, random_states, random_weights

pytestmark = pytest.mark.gpu

N, NOPT, SEED, BASE = 700, 3, 77, 5
S1 = dict(HP, update_count_floor=0, reoffer_period=4)
# every field changed, to values of tests/test_ref64_hparams.py's edge list: the re-offer period 4 -> 0, and the option limit
# 25 -> 2, which leaves envs mid-option beyond the new limit
S2 = dict(gamma=1.0, alpha=1.0, epsilon=0.0, r_option_success=-50.0, max_episode_steps=2, max_option_steps=2,
          update_count_floor=257, reoffer_period=0)
CHAIN, TREE3 = [0, 0, 1, 2], [0, 0, 0, 1]          # 3 -> 2 -> 1 -> goal;  1 -> goal, 2 -> goal, 3 -> 1
BLOCKS = pytest.mark.parametrize("block", [256, 64])


class Rig:
    """A context with every buffer a step writes attached, its env state, weights and classifiers on the device."""

    def __init__(self, block, map_name, hp, parents=CHAIN, gest=0, like=None):
        self.map = scg.load_map(map_name)
        self.ctx = ScgContext(N, NOPT, self.map, device=0, seed=SEED, env_id_base=BASE, block_envs=block, **hp)
        self.ctx.set_option_parents(parents)
        self.gs = self.ctx.set_gestation(gest)
        self.ring_x, self.ring_y, self.events, self.ev_len = self.ctx.set_trace_buffers(8)
        self.G, self.n_k = self.ctx.grad_buffers()
        self.st = EnvState(N, self.ctx.device, self.map)
        self.W = torch.zeros((NOPT + 1, 5, 1296), dtype=torch.float32, device=self.ctx.device)
        self.clf = dev(chain_classifiers(self.map, NOPT))
        self.Wv, self.cv = self.W.view(-1), self.clf.view(-1)          # the same objects every step: core.py's cached arguments
        if like is not None:                   # clones of the other rig's device data (never its tensors)
            for k, v in like.tensors().items():
                self.tensors()[k].copy_(v)

    def tensors(self):
        d = {k: getattr(self.st, k) for k in EnvState.FIELDS}
        d.update(W=self.W, clf=self.clf, G=self.G, n_k=self.n_k, ring_x=self.ring_x, ring_y=self.ring_y, events=self.events,
                 ev_len=self.ev_len, gest_succ=self.gs)
        return d

    def host(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in self.tensors().items()}

    def step(self, t, enabled=0b1110, interrupt=False):
        self.ctx.step(self.st, self.Wv, self.cv, enabled, t, interrupt=interrupt)


def warm(block, map_name="pinball_maze", hp=S1):
    """A context that has run two learning steps (t = 0, 1) on its state under `hp`: a prepared env order, warm histograms."""
    a = Rig(block, map_name, hp)
    rng = np.random.default_rng(N + block)
    clf = chain_classifiers(a.map, NOPT)
    pre = pre_state(a.map, N, NOPT, rng, max_ep=hp["max_episode_steps"], max_opt=hp["max_option_steps"])
    pre["opt_steps"][:] = np.minimum(pre["opt_steps"], 20)          # (the options stay clear of S1's limit during the warm-up)
    seat_running_envs(a.map, pre, clf, CHAIN, rng, share=0.8)
    for k in EnvState.FIELDS:
        getattr(a.st, k).copy_(dev(pre[k]))
    a.W.copy_(dev(random_weights(NOPT + 1, 3, std=1e-3)))
    for t in (0, 1):
        a.step(t)
    return a


def model_of(map_name, hp, parents=CHAIN):
    m = scg.load_map(map_name)
    orc = sc_oracle.Oracle(m, SCALE, n_envs=N, n_options=NOPT, seed=SEED, env_id_base=BASE, n_threads=8, **hp)
    return StepModel(orc, m, NOPT, seed=SEED, env_id_base=BASE, parents=parents, scale=SCALE, **hp)


def assert_same(a, b, msg, names=None):
    ta, tb = a.tensors(), b.tensors()
    for k in names or ta:
        assert torch.equal(ta[k], tb[k]), f"{msg}: {k} differs in {int((ta[k] != tb[k]).sum())} of {ta[k].numel()} elements"


def run_both(a, b, ts, model, enabled=0b1110, gest=0, interrupt=False, msg=""):
    """Steps `ts` on the reconfigured context `a` and the fresh one `b`: equal after every step, and `a` within the model."""
    n_amb = n_dealt = 0
    for t in ts:
        pre = a.host()
        a.step(t, enabled, interrupt)
        b.step(t, enabled, interrupt)
        got = a.host()
        assert_same(a, b, f"{msg} t={t}")
        out = model.step(pre, pre["W"], pre["clf"], t, enabled, gest, sut=dict(got), interrupt=interrupt)
        n_amb += compare(out, got, got["G"], got["n_k"], got["W"], events=got["events"], ev_len=got["ev_len"],
                         gest_succ=got["gest_succ"] - pre["gest_succ"], msg=f"{msg} t={t} model:")
        n_dealt += int((got["done"] == 2).sum())
    assert_rarely_ambiguous(n_amb, len(ts) * N, msg)
    return n_dealt                             # envs that ran into the episode limit and were dealt a start position


def move_to_map(rig, seed):
    """A state that is valid for the rig's (new) map, written in place: positions and velocities of random_states, a tenth of
    the envs one step before the episode limit, so that the new start list is drawn from. The option ids stay as they are (the
    prepared env order goes with them)."""
    x, y, vx, vy = random_states(rig.map, N, seed)
    rng = np.random.default_rng(seed)
    ep = np.where(rng.random(N) < 0.1, rig.ctx.cfg.max_episode_steps - 1, rng.integers(0, 30, N)).astype(np.int32)
    for k, v in dict(x=x, y=y, vx=vx, vy=vy, ep_steps=ep).items():
        getattr(rig.st, k).copy_(dev(v))
    rig.clf.copy_(dev(chain_classifiers(rig.map, NOPT)))


@BLOCKS
def test_set_hparams_changing_every_field(block):
    a = warm(block)
    pre = a.host()
    assert ((pre["option_id"] > 0) & (pre["opt_steps"] >= S2["max_option_steps"])).sum() >= 20     # mid-option, beyond the new limit
    a.ctx.set_hparams(**S2)
    b = Rig(block, "pinball_maze", S2, like=a)
    run_both(a, b, (2, 3), model_of("pinball_maze", S2), msg="S1 -> S2")


@BLOCKS
def test_set_map_to_fewer_edges_and_back(block):
    maze, simple = scg.load_map("pinball_maze"), scg.load_map("pinball_simple")
    assert maze.n_edges > simple.n_edges and len(maze.starts) > len(simple.starts)
    a = warm(block)
    a.ctx.set_map(simple)
    a.map = simple
    assert a.ctx.map is simple
    move_to_map(a, 1)
    b = Rig(block, "pinball_simple", S1, like=a)
    assert run_both(a, b, (2, 3), model_of("pinball_simple", S1), msg="maze -> simple") >= 20
    a.ctx.set_map(maze)
    a.map = maze
    move_to_map(a, 2)
    c = Rig(block, "pinball_maze", S1, like=a)
    assert run_both(a, c, (4, 5), model_of("pinball_maze", S1), msg="simple -> maze") >= 20


@BLOCKS
def test_set_option_parents_and_gestation(block):
    a = warm(block)
    a.ctx.set_option_parents(TREE3)
    a.ctx.set_gestation(0b100)
    b = Rig(block, "pinball_maze", S1, parents=TREE3, gest=0b100, like=a)
    run_both(a, b, (2, 3), model_of("pinball_maze", S1, TREE3), enabled=0b1010, gest=0b100, msg="chain -> tree, gestation on")
    a.ctx.set_gestation(0)
    c = Rig(block, "pinball_maze", S1, parents=TREE3, like=a)
    run_both(a, c, (4, 5), model_of("pinball_maze", S1, TREE3), msg="gestation off")


@BLOCKS
def test_everything_at_once(block):
    a = warm(block)
    simple = scg.load_map("pinball_simple")
    a.ctx.set_hparams(**S2)
    a.ctx.set_map(simple)
    a.map = simple
    a.ctx.set_option_parents(TREE3)
    a.ctx.set_gestation(0b100)
    move_to_map(a, 3)
    b = Rig(block, "pinball_simple", S2, parents=TREE3, gest=0b100, like=a)
    run_both(a, b, (2, 3), model_of("pinball_simple", S2, TREE3), enabled=0b1010, gest=0b100, interrupt=True, msg="all at once")


@BLOCKS
def test_there_and_back_leaves_nothing_behind(block):
    """S1 -> S2 -> S1 (settings, map, parents, gestation) equals a context that never left S1: first without a step under S2
    (against a twin that ran the same warm-up), then with two steps under S2 in between (against a fresh S1 context)."""
    a, twin = warm(block), warm(block)
    assert_same(a, twin, "the warm-up is deterministic")

    def there(r):
        r.ctx.set_hparams(**S2)
        r.ctx.set_map(scg.load_map("pinball_simple"))
        r.ctx.set_option_parents(TREE3)
        r.ctx.set_gestation(0b100)

    def back(r):
        r.ctx.set_hparams(**S1)
        r.ctx.set_map(scg.load_map("pinball_maze"))
        r.ctx.set_option_parents(CHAIN)
        r.ctx.set_gestation(0)

    there(a)
    back(a)
    assert bytes(a.ctx.cfg) == bytes(twin.ctx.cfg)
    run_both(a, twin, (2, 3), model_of("pinball_maze", S1), msg="S1 -> S2 -> S1, no step between")
    there(a)
    a.map = a.ctx.map
    move_to_map(a, 4)
    for t in (4, 5):
        a.step(t, 0b1010)
    back(a)
    a.map = a.ctx.map
    move_to_map(a, 5)
    b = Rig(block, "pinball_maze", S1, like=a)
    run_both(a, b, (6, 7), model_of("pinball_maze", S1), msg="S1 -> S2 (two steps) -> S1")


# ---------------------------------------------------------------------------------------------------- the other launches

def _rollout(r, kind):
    """Eight acting steps with BEGIN from the rig's state; returns every output of the launch."""
    stats = EpisodeStats(NOPT + 1, N, r.ctx.device)
    out = {}
    if kind == "trials":
        opt = torch.as_tensor(1 + np.arange(N) % NOPT, dtype=torch.int32)
        res = TrialResult(N, opt, r.ctx.device)
        rec = Trajectory(N, 8, 0, r.ctx.device)
        r.ctx.option_trials(r.st.x, r.st.y, r.st.vx, r.st.vy, res.option, r.W.view(-1), r.clf.view(-1), 0b1110, 9, res)
        r.ctx.option_trials(r.st.x, r.st.y, r.st.vx, r.st.vy, res.option, r.W.view(-1), r.clf.view(-1), 0b1110, 9,
                            TrialResult(N, opt, r.ctx.device), record=rec)
        out.update({f: getattr(res, f) for f in TrialResult.FIELDS})
        out.update({"rec_" + f: getattr(rec, f) for f in rec.fields}, rec_len=rec.len)
        return out
    rec = Trajectory(N, 9, 0, r.ctx.device) if kind == "record" else None
    r.ctx.rollout(r.st, r.W.view(-1), r.clf.view(-1), 0b1110, 9, 8, stats, begin=True, record=rec, interrupt=kind == "interrupt")
    out.update({f: getattr(stats, f) for f in EpisodeStats.FIELDS}, interrupts=stats.interrupts)
    if rec is not None:
        out.update({"rec_" + f: getattr(rec, f) for f in rec.fields}, rec_len=rec.len)
    return out


@pytest.mark.parametrize("kind", ["rollout", "interrupt", "record", "trials"])
@BLOCKS
def test_rollouts_and_trials_after_set_hparams(block, kind):
    """scg_rollout, scg_rollout_interrupt, scg_rollout_record and scg_option_trials take the context's settings the same way the
    step does: after S1 -> S2 each equals the same launch of a fresh S2 context (SCG_ROLLOUT_EPW left alone)."""
    hp2 = dict(S2, max_episode_steps=5, epsilon=0.1)       # (episodes that end inside the eight steps, and some that do not)
    a = warm(block)
    a.W.copy_(dev(random_weights(NOPT + 1, 4, std=0.05)))
    a.ctx.set_hparams(**hp2)
    b = Rig(block, "pinball_maze", hp2, like=a)
    ra, rb = _rollout(a, kind), _rollout(b, kind)
    torch.cuda.synchronize()
    for k in ra:
        assert torch.equal(ra[k], rb[k]), f"{kind}: {k} differs"
    assert_same(a, b, kind, names=EnvState.FIELDS)
    if kind == "trials":
        assert (ra["outcome"] != 0).all() and int(ra["steps"].max()) <= hp2["max_option_steps"]
    else:
        assert int(ra["episodes"].sum()) >= N              # max_episode_steps = 5 took hold: every env finished an episode
