"""The CPU oracle against the independent float64 model of one step-batch (tests/ref64.py, SPEC §2, §4-§7).

Parity tests show that the oracle and the HIP path agree; these show that the oracle does what the SPEC says: which env is an
update item of which value function, with which target, the value gate, the re-offer stagger, the env order (an env dropped
or counted twice in a chunk), n_k, the count floor, gest_succ and the events. Every step starts from a pre-state made here, so
that errors do not pile up. Discrete fields are exact; qcache, G and W are within per-element tolerances; where N <= ~2000
the tolerance is below the single-item resolution, so a dropped, duplicated or misrouted update item fails."""
import numpy as np
import pytest

import sc_oracle
import skill_chaining_with_graphs_amd as scg
from ref64 import StepModel, compare, env_order_layout, philox4x32_10
from util import HP, SCALE, chain_classifiers, disc_weights, oracle_block, random_states, random_weights

TREE = [0, 0, 0, 1, 2, 4]                 # 1 -> goal, 2 -> goal, 3 -> 1, 4 -> 2, 5 -> 4


def test_vectorised_philox_published_vectors():
    from test_oracle_primitives import PHILOX_KAT
    for ctr, key, want in PHILOX_KAT:
        got = philox4x32_10(*[np.array([c], np.uint64) for c in ctr], *key)
        assert tuple(int(v[0]) for v in got) == want


class OracleRunner:
    """The system under test on the CPU: the oracle, with trace buffers and gestation counters attached."""

    def __init__(self, map_name, n, n_options, *, seed=0, env_id_base=0, parents=None, gest=0, **hp):
        m = scg.load_map(map_name) if isinstance(map_name, str) else map_name
        kw = dict(HP)
        kw.update(hp)
        self.orc = sc_oracle.Oracle(m, SCALE, n_envs=n, n_options=n_options, seed=seed, env_id_base=env_id_base,
                                    n_threads=8, **kw)
        if parents is not None:
            self.orc.set_parents(parents)
        self.orc.set_gestation(gest)
        self.orc.set_trace(8)
        self.gest, self.map = gest, m
        self.model = StepModel(self.orc, m, n_options, seed=seed, env_id_base=env_id_base, parents=parents, scale=SCALE, **kw)

    def step(self, pre, W, clf, t, enabled):
        st = {k: v.copy() for k, v in pre.items()}
        gs0 = self.orc.gest_succ.copy()
        G, n_k = self.orc.step(st, W, clf, t, enabled_mask=enabled)
        Wn = W.copy()
        self.orc.apply(Wn, G, n_k)
        return dict(st=st, G=G, n_k=n_k, W=Wn, events=self.orc.events.copy(), ev_len=self.orc.ev_len.copy(),
                    gest_succ=self.orc.gest_succ - gs0)


def check_step(runner, pre, W, clf, t, enabled, check_resolution=False, msg=""):
    """One step of the system under test from `pre` against the model: (model output, SUT output, ambiguous env count).
    A runner whose `interrupt` is set steps with SPEC §12's interruption, and so does the model."""
    got = runner.step(pre, W, clf, t, enabled)
    out = runner.model.step(pre, W, clf, t, enabled, runner.gest, sut=dict(got["st"], events=got["events"]),
                            interrupt=getattr(runner, "interrupt", False))
    n_amb = compare(out, got["st"], got["G"], got["n_k"], got["W"], events=got["events"], ev_len=got["ev_len"],
                    gest_succ=got["gest_succ"], check_resolution=check_resolution, msg=msg)
    return out, got, n_amb


def tree_classifiers(m):
    tx, ty, _ = m.target
    clf = np.zeros((6, 8), np.float32)
    for k, (cx, cy, r) in enumerate([(tx, ty, 0.15), (tx - 0.25, ty + 0.1, 0.15), (tx, ty + 0.3, 0.2),
                                     (tx - 0.45, ty + 0.3, 0.2), (tx - 0.6, ty + 0.55, 0.25)], start=1):
        clf[k] = disc_weights(cx, cy, r)
    return clf


def pre_state(m, n, n_options, rng, *, max_ep, max_opt, dist="uniform", n_vf=None, wild_ids=False):
    """A pre-step state with every case the step has to handle: option ids k and -k (staying out), envs about to time out
    of their option and of their episode, envs about to reach the goal, random qcache (random greedy actions)."""
    n_vf = n_options + 1 if n_vf is None else n_vf
    st = sc_oracle.new_state(n, m)
    x, y, vx, vy = random_states(m, n, int(rng.integers(1 << 30)), vmax=2.0)
    if n >= 8:
        vx[:n // 16] = np.where(rng.random(n // 16) < 0.5, -2.0, 2.0)            # |v| = 2: s^ = 0 or 1 after the clip
    tx, ty, tr = m.target
    near = np.zeros(n, bool)                                                    # about to hit the goal (a few: a goal item's
    near[rng.choice(n, max(1, min(n // 25, 4)), replace=False)] = True          #  delta of 1e4 dominates its action's tolerance)
    x[near] = tx - tr - 0.01; y[near] = ty; vx[near] = 1.0; vy[near] = 0.0
    st["x"][:], st["y"][:], st["vx"][:], st["vy"][:] = x, y, vx, vy
    if n_options:
        if dist == "heavy":
            opt = np.where(rng.random(n) < 0.9, rng.integers(1, n_options + 1, n), 0)
        else:
            opt = rng.integers(-n_options, n_options + 1, n)
        if wild_ids:
            w = rng.random(n) < 0.1
            opt[w] = rng.choice([33, 257, n_vf, -n_vf, -40], int(w.sum()))
        st["option_id"][:] = opt
    st["opt_steps"][:] = np.where(rng.random(n) < 0.2, max_opt - 1, rng.integers(0, max_opt, n))
    st["ep_steps"][:] = np.where(rng.random(n) < 0.1, max_ep - 1, rng.integers(0, max_ep, n))
    st["qcache"][:] = rng.standard_normal((5, n)).astype(np.float32)
    return st


# (map, N, options, parents, gest, reoffer, floor, epsilon, env_id_base, dist)
SWEEP = [
    ("pinball_empty", 1, 0, None, 0, 4, 0, 0.1, 0, "uniform"),
    ("pinball_simple", 63, 2, None, 0b100, 4, 64, 1.0, 5, "uniform"),
    ("pinball_simple", 257, 5, TREE, 0, 4, 0, 0.1, 3, "uniform"),
    ("pinball_maze", 257, 3, None, 0b1000, 1, 64, 0.0, 0, "uniform"),
    ("pinball_simple", 1000, 5, None, 0b100000, 4, 64, 0.1, 1001, "uniform"),
    ("pinball_simple", 1000, 4, TREE, 0, 4, 0, 0.1, 7, "heavy"),
    ("pinball_maze", 1000, 1, None, 0, 1, 0, 0.0, 0, "uniform"),
    ("pinball_simple", 4100, 5, None, 0b1000, 4, 64, 0.1, 123, "uniform"),
    ("pinball_empty", 4100, 5, TREE, 0b10000, 4, 0, 1.0, 2, "heavy"),
]


# every configuration on the default build of the oracle, those up to 1000 envs on the 64- and 128-env builds too
CASES = [(c, b) for b in (256, 128, 64) for c in SWEEP if b == 256 or c[1] <= 1000]


def assert_rarely_ambiguous(n_amb, n_env_steps, msg=""):
    assert n_amb <= max(2, n_env_steps // 200), f"{msg}: {n_amb} ambiguous envs in {n_env_steps} env-steps"


@pytest.mark.parametrize("cfg,block_envs", CASES, ids=[f"b{b}-{c[0]}-{c[1]}-{c[2]}opt-{c[9]}" for c, b in CASES])
def sweep_case(make, cfg, block_envs, steps=(0, 1, 2), seed=None):
    """One configuration of the sweep: fresh pre-states every step (errors do not pile up), both env-order layouts where
    the option mix calls for them. `steps` and `seed` (default 11 + N) may be any 64-bit values (test_wide_identity.py)."""
    map_name, n, nopt, parents, gest, period, floor, eps, base, dist = cfg
    runner = make(map_name, n, nopt, seed=11 + n if seed is None else seed, env_id_base=base, parents=parents, gest=gest,
                  reoffer_period=period, update_count_floor=floor, epsilon=eps)
    enabled = ((1 << (nopt + 1)) - 2) & ~gest
    clf = tree_classifiers(runner.map)[:nopt + 1] if parents is not None else chain_classifiers(runner.map, nopt)
    rng = np.random.default_rng(n * 7 + nopt)
    W = random_weights(nopt + 1, n + 1, std=1e-3)
    n_amb, layouts = 0, set()
    for t in steps:
        pre = pre_state(runner.map, n, nopt, rng, max_ep=HP["max_episode_steps"], max_opt=HP["max_option_steps"], dist=dist)
        layouts.add(env_order_layout(pre["option_id"], nopt + 1, block_envs))
        n_amb += check_step(runner, pre, W, clf, t, enabled, check_resolution=n <= 2000, msg=f"t={t}")[2]
    assert_rarely_ambiguous(n_amb, len(steps) * n)
    return layouts


@pytest.mark.parametrize("cfg,block_envs", CASES, ids=[f"b{b}-{c[0]}-{c[1]}-{c[2]}opt-{c[9]}" for c, b in CASES])
def test_oracle_step_matches_the_float64_model(cfg, block_envs):
    with oracle_block(block_envs):
        sweep_case(OracleRunner, cfg, block_envs)


def test_sweep_covers_both_env_order_layouts():
    """The sweep's option mixes put SPEC §5's chunked AND padded layouts in front of the model (an env dropped or counted
    twice by either one would show up as a wrong n_k, a wrong G and an unchanged state)."""
    seen = set()
    for cfg, b in CASES:
        if cfg[2]:
            rng = np.random.default_rng(cfg[1] * 7 + cfg[2])
            pre = pre_state(scg.load_map(cfg[0]), cfg[1], cfg[2], rng, max_ep=60, max_opt=25, dist=cfg[9])
            seen.add(env_order_layout(pre["option_id"], cfg[2] + 1, b))
    assert seen == {"chunked", "padded"}


# ---------------------------------------------------------------------------------------------------- named edge cases
# Each takes `make` (the runner class of the system under test: OracleRunner here, the HIP path in test_gpu_ref64.py).

def _inside(m, n, rng, cx, cy, r):
    """n free positions inside the disc (cx, cy, r), clear of the goal disc."""
    out = []
    while len(out) < n:
        p = m.sample_free(4 * n, rng, margin=1.5)
        d = np.hypot(p[:, 0] - cx, p[:, 1] - cy)
        g = np.hypot(p[:, 0] - m.target[0], p[:, 1] - m.target[1])
        out.extend(p[(d < r) & (g > m.target[2] + 0.05)].tolist())
    return np.asarray(out[:n], np.float32)


def edge_new_option_copy_of_root_enters(make, n=512):
    """A new option starts as a copy of the root (W_k = W_0): the tie V_k = V_0 is exact and every candidate enters."""
    r = make("pinball_simple", n, 3, seed=3, epsilon=0.0)
    clf = chain_classifiers(r.map, 3)
    rng = np.random.default_rng(1)
    pre = pre_state(r.map, n, 3, rng, max_ep=60, max_opt=25)
    pre["option_id"][:] = 0
    W = random_weights(4, 2, std=0.05)
    W[1:] = W[0]
    out, got, n_amb = check_step(r, pre, W, clf, 0, 0b1110)
    assert n_amb == 0
    ent = out["entering"]
    assert ent.sum() > 20 and not out["declined"].any()
    assert np.array_equal(got["st"]["option_id"][ent], out["cand"][ent]) and (got["st"]["option_id"][ent] > 0).all()


def edge_nan_weights_decline(make, n=512):
    """NaN in W_k (every action): every candidate of option k declines (a NaN never compares >=), its qcache holds the
    root's values, and the other value functions are unaffected. NaN in ONE action of W_k: the max passes over it (IEEE
    maxNum), and the gate compares the other four."""
    r = make("pinball_simple", n, 3, seed=4, epsilon=0.0)
    clf = chain_classifiers(r.map, 3)
    rng = np.random.default_rng(2)
    pre = pre_state(r.map, n, 3, rng, max_ep=60, max_opt=25)
    pre["option_id"][:] = np.where(np.abs(pre["option_id"]) == 2, 0, pre["option_id"])     # nobody runs option 2 yet
    W = random_weights(4, 3, std=0.05)
    W[2, :, 100] = np.nan
    out, got, _ = check_step(r, pre, W, clf, 0, 0b1110)
    c2 = out["entering"] & (out["cand"] == 2)
    assert c2.sum() > 5 and out["declined"][c2].all()
    st = got["st"]
    assert (st["option_id"][c2] == -2).all()
    assert np.isfinite(st["qcache"][:, c2]).all()
    assert np.isfinite(got["W"][[0, 1, 3]]).all() and got["n_k"][2] == 0
    W = random_weights(4, 3, std=0.05)
    W[2, 3, 100] = np.nan
    out, got, _ = check_step(r, pre, W, clf, 1, 0b1110)
    c2 = out["entering"] & (out["cand"] == 2)
    assert c2.sum() > 5 and out["declined"][c2].any() and not out["declined"][c2].all()


def edge_exit_rule(make, n=512):
    """SPEC §5 exit rule: an option that ends while the episode goes on — on success (reaching its parent's set) and on
    failure (leaving its own) — bootstraps from the ROOT's value m_0 of s_next."""
    r = make("pinball_simple", n, 3, seed=5, epsilon=1.0, max_option_steps=1000)
    clf = chain_classifiers(r.map, 3)
    rng = np.random.default_rng(3)
    pre = pre_state(r.map, n, 3, rng, max_ep=1000, max_opt=1000)
    pre["ep_steps"][:] = 0; pre["opt_steps"][:] = 0
    tx, ty, _ = r.map.target
    ring = _inside(r.map, n, rng, tx, ty, 0.40)            # around the rim of I_1 (0.18) and I_2 (0.35)
    pre["x"][:], pre["y"][:] = ring[:, 0], ring[:, 1]
    pre["vx"][:] = rng.uniform(-2, 2, n); pre["vy"][:] = rng.uniform(-2, 2, n)
    pre["option_id"][:] = rng.integers(1, 4, n)
    W = random_weights(4, 4, std=0.05)
    out, got, _ = check_step(r, pre, W, clf, 0, 0b1110)
    o, done = pre["option_id"], out["done"]
    term = (out["opt_steps"] == 0) & (done == 0)
    from ref64 import clf_model
    in_par = np.zeros(n, bool)                             # s' (= s_next: no reset) inside the parent's set (option 1's parent is the goal)
    for k in (2, 3):
        in_par |= (o == k) & (clf_model(clf[k - 1], out["x"], out["y"])[0] > 0)
    assert (term & in_par).sum() >= 3 and (term & ~in_par).sum() >= 3       # both kinds of exit happened


def edge_gestation_has_no_timeout(make, n=512):
    """A gestating option's off-policy items never time out: an env at its option step limit still bootstraps from m_k."""
    r = make("pinball_simple", n, 2, seed=6, gest=0b100, epsilon=1.0, max_option_steps=5)
    clf = chain_classifiers(r.map, 2)
    rng = np.random.default_rng(4)
    pre = pre_state(r.map, n, 2, rng, max_ep=60, max_opt=5)
    tx, ty, _ = r.map.target
    pos = _inside(r.map, n, rng, tx, ty, 0.33)             # inside I_2
    pre["x"][:], pre["y"][:] = pos[:, 0], pos[:, 1]
    pre["vx"][:] = 0.0; pre["vy"][:] = 0.0
    pre["opt_steps"][:] = 4; pre["ep_steps"][:] = 0
    W = random_weights(3, 5, std=0.05)
    out, got, _ = check_step(r, pre, W, clf, 0, 0b010)
    assert out["n_k"][2] > 50


def edge_reoffer_stagger_uses_global_id(make, n=256, seed=7, env_id_base=4097, period=4, steps=(0, 1)):
    """An env staying out of option k (option_id = -k) is offered k again when (t + global env id) mod reoffer_period == 0
    (the sum taken mod 2^64: test_wide_identity.py passes counters and ids round 2^32 and 2^64)."""
    r = make("pinball_simple", n, 1, seed=seed, env_id_base=env_id_base, epsilon=0.0, reoffer_period=period)
    clf = chain_classifiers(r.map, 1)
    rng = np.random.default_rng(5)
    pre = pre_state(r.map, n, 1, rng, max_ep=60, max_opt=25)
    tx, ty, _ = r.map.target
    pos = _inside(r.map, n, rng, tx, ty, 0.15)
    pre["x"][:], pre["y"][:] = pos[:, 0], pos[:, 1]
    pre["vx"][:] = 0.0; pre["vy"][:] = 0.0; pre["ep_steps"][:] = 0
    pre["option_id"][:] = -1
    W = random_weights(2, 6, std=0.05)
    for t in steps:
        out, got, _ = check_step(r, pre, W, clf, t, 0b10)
        stays = out["stay"]
        assert (1 - 1 / period - 0.15) * n < stays.sum() < (1 - 1 / period + 0.15) * n
        offered = np.array([(t + env_id_base + e) % 2 ** 64 % period == 0 for e in range(n)])
        assert not stays[offered].any()


def edge_out_of_range_ids(make, n=512):
    """Caller-written ids outside (-n_vf, n_vf) (33, 257, n_vf, -n_vf, -40) name no option: the env runs the root — no
    termination test, no update item of any option — and is selected afresh."""
    nopt = 2
    r = make("pinball_simple", n, nopt, seed=8, epsilon=0.1)
    clf = chain_classifiers(r.map, nopt)
    rng = np.random.default_rng(6)
    pre = pre_state(r.map, n, nopt, rng, max_ep=60, max_opt=25)
    tx, ty, _ = r.map.target
    half = n // 2
    pos = _inside(r.map, half, rng, tx, ty, 0.17)          # half of them inside I_1 (and I_2)
    pre["x"][:half], pre["y"][:half] = pos[:, 0], pos[:, 1]
    pre["vx"][:half] = 0.0; pre["vy"][:half] = 0.0
    wild = np.array([33, 257, nopt + 1, -(nopt + 1), -40])
    pre["option_id"][:] = np.where(np.arange(n) % 3 == 0, wild[np.arange(n) % 5], pre["option_id"])
    pre["opt_steps"][:] = 3; pre["ep_steps"][:] = 0
    W = random_weights(nopt + 1, 7, std=0.05)
    out, got, _ = check_step(r, pre, W, clf, 0, 0b110)
    w = np.isin(pre["option_id"], wild)
    assert (got["st"]["opt_steps"][w] == 0).all()
    assert (np.abs(got["st"]["option_id"][w]) <= nopt).all()


EDGES = [edge_new_option_copy_of_root_enters, edge_nan_weights_decline, edge_exit_rule, edge_gestation_has_no_timeout,
         edge_reoffer_stagger_uses_global_id, edge_out_of_range_ids]


@pytest.mark.parametrize("edge", EDGES, ids=[e.__name__[5:] for e in EDGES])
def test_oracle_edge_case(edge):
    edge(OracleRunner)
