"""SPEC §11 / §12 option interruption in the float64 model (tests/ref64.py), on the CPU: the model against the oracle-built
emulator of the interrupting learner (tests/interrupt_learning_model.py) over tests/test_ref64_oracle.py's sweep and at the named
edges of the rule, and six wrong answers that compare() must refuse.

The model's rule is written from the SPEC alone; the emulator was written together with the kernel. Agreement here says that the
two readings of §12 agree and that the model can judge the HIP path (tests/test_gpu_ref64_interrupt.py runs the same sweep and
edges there)."""
from types import SimpleNamespace

import numpy as np
import pytest

import interrupt_learning_model as ilm
import skill_chaining_with_graphs_amd as scg
from ref64 import clf_model, compare, env_order_layout
from test_ref64_oracle import SWEEP, OracleRunner, assert_rarely_ambiguous, check_step, pre_state, tree_classifiers
from util import HP, chain_classifiers, crossing_weights, disc_weights, oracle_block, random_weights

MAX_EP, MAX_OPT = HP["max_episode_steps"], HP["max_option_steps"]


class EmulatorRunner(OracleRunner):
    """SPEC §12 on the CPU: interrupt_learning_model.step on the oracle (post-state, G, n_k), then its apply."""

    interrupt = True

    def step(self, pre, W, clf, t, enabled):
        gs0 = self.orc.gest_succ.copy()
        post, G, n_k, _ = ilm.step(self.orc, pre, W, clf, t, enabled, gest=self.gest, interrupt=self.interrupt)
        return dict(st=post, G=G, n_k=n_k, W=ilm.apply(self.orc, W, G, n_k), events=self.orc.events.copy(),
                    ev_len=self.orc.ev_len.copy(), gest_succ=self.orc.gest_succ - gs0)


def seat_running_envs(m, st, clf, parents, rng, share=0.6, vmax=0.3):
    """Move a share of the envs that run an option k (option_id = k >= 1) to slow states well inside I_k and outside k's target
    region: their options can go on (SPEC §4.2's keep), so that the interruption rule has envs to decide on."""
    pool = m.sample_free(8192, rng, margin=1.5)
    px, py = pool[:, 0], pool[:, 1]
    z = [None] + [clf_model(clf[k], px, py)[0] for k in range(1, len(clf))]
    oid = st["option_id"]
    for k in range(1, len(clf)):
        inside = z[k] > 0.02
        if parents[k] != 0:
            inside &= z[parents[k]] < -0.02
        pts = np.nonzero(inside)[0]
        who = np.nonzero((oid == k) & (rng.random(len(oid)) < share))[0]
        if len(pts) and len(who):
            pick = rng.choice(pts, len(who))
            st["x"][who], st["y"][who] = px[pick], py[pick]
            st["vx"][who] = rng.uniform(-vmax, vmax, len(who)).astype(np.float32)
            st["vy"][who] = rng.uniform(-vmax, vmax, len(who)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the sweep

INT_SWEEP = [c for c in SWEEP if c[2] >= 1]           # (a configuration without options has nothing to interrupt)


def case_ids(cases):
    return [f"b{b}-{c[0]}-{c[1]}-{c[2]}opt-{c[9]}" for c, b in cases]


def interrupt_sweep_case(make, cfg, block_envs, steps=(0, 1, 2), seed=None):
    """One configuration of tests/test_ref64_oracle.py's sweep with interruption: fresh pre-states every step, a share of the option
    runners seated inside their sets. Asserts that the case is not vacuous; returns (layouts, interrupted, ambiguous)."""
    map_name, n, nopt, parents, gest, period, floor, eps, base, dist = cfg
    r = make(map_name, n, nopt, seed=11 + n if seed is None else seed, env_id_base=base, parents=parents, gest=gest, reoffer_period=period,
             update_count_floor=floor, epsilon=eps)
    enabled = ((1 << (nopt + 1)) - 2) & ~gest
    clf = tree_classifiers(r.map)[:nopt + 1] if parents is not None else chain_classifiers(r.map, nopt)
    rng = np.random.default_rng(n * 7 + nopt)
    W = random_weights(nopt + 1, n + 1, std=1e-3)
    n_amb = n_int = 0
    layouts = set()
    for t in steps:
        pre = pre_state(r.map, n, nopt, rng, max_ep=MAX_EP, max_opt=MAX_OPT, dist=dist)
        seat_running_envs(r.map, pre, clf, r.model.parents, rng)
        layouts.add(env_order_layout(pre["option_id"], nopt + 1, block_envs))
        out, _, a = check_step(r, pre, W, clf, t, enabled, check_resolution=n <= 2000, msg=f"t={t}")
        n_amb += a
        n_int += int(out["interrupted"].sum())
    print(f"\n[{map_name} n={n} opt={nopt} B={block_envs}] {n_int} interrupted, {n_amb} ambiguous in {len(steps) * n} env-steps")
    assert_rarely_ambiguous(n_amb, len(steps) * n)
    assert n_int >= max(3, len(steps) * n // 100), f"only {n_int} interrupted envs: the case is (nearly) vacuous"
    return layouts, n_int, n_amb


CPU_CASES = [(c, b) for b in (256, 64) for c in INT_SWEEP if b == 256 or c[1] <= 1000]


@pytest.mark.parametrize("cfg,block_envs", CPU_CASES, ids=case_ids(CPU_CASES))
def test_model_matches_the_interrupt_emulator(cfg, block_envs):
    with oracle_block(block_envs):
        interrupt_sweep_case(EmulatorRunner, cfg, block_envs)


def test_interrupt_sweep_covers_both_env_order_layouts():
    """The first pre-state of every case (the option ids do not depend on the seating) puts both of SPEC §5's layouts in front
    of the model, on the 256- and on the 64-env build."""
    seen = {256: set(), 64: set()}
    for cfg, b in CPU_CASES:
        pre = pre_state(scg.load_map(cfg[0]), cfg[1], cfg[2], np.random.default_rng(cfg[1] * 7 + cfg[2]), max_ep=MAX_EP,
                        max_opt=MAX_OPT, dist=cfg[9])
        seen[b].add(env_order_layout(pre["option_id"], cfg[2] + 1, b))
    assert seen == {256: {"chunked", "padded"}, 64: {"chunked", "padded"}}, seen


# ---------------------------------------------------------------------------------------------------- named edges
# Each takes `make` (the runner class of the system under test: EmulatorRunner here, the HIP path in test_gpu_ref64_interrupt.py),
# runs one interrupting step against the model and asserts that its edge occurred.

def _edge(make, n, nopt, seed, *, map_name="pinball_simple", clf=None, ids=None, share=1.0, **kw):
    """A runner and a pre-state at the start of the episode and of the options, the option runners seated inside their sets."""
    r = make(map_name, n, nopt, seed=seed, **kw)
    clf = chain_classifiers(r.map, nopt) if clf is None else clf
    rng = np.random.default_rng(seed)
    pre = pre_state(r.map, n, nopt, rng, max_ep=MAX_EP, max_opt=MAX_OPT)
    if ids is not None:
        pre["option_id"][:] = ids
    pre["ep_steps"][:] = 0
    pre["opt_steps"][:] = 0
    seat_running_envs(r.map, pre, clf, r.model.parents, rng, share=share)
    return r, clf, pre


def _check(r, pre, W, clf, enabled, n):
    out, got, n_amb = check_step(r, pre, W, clf, 0, enabled)
    assert_rarely_ambiguous(n_amb, n)
    ok = np.ones(n, bool)
    ok[out["ambiguous"]] = False
    return out, got, ok


def edge_ties_never_interrupt(make, n=512):
    """Every W_k == W_0: V_o and V_0 are the same sum in the same order, an exact tie, which keeps the option."""
    r, clf, pre = _edge(make, n, 3, 21)
    W = crossing_weights(4, 21)
    W[1:] = W[0]
    out, got, _ = _check(r, pre, W, clf, 0b1110, n)
    keep = out["keep"]
    assert keep.sum() >= 50 and not out["interrupted"].any()
    assert np.array_equal(got["st"]["option_id"][keep], pre["option_id"][keep])


def edge_nan_option_weights_interrupt(make, n=512):
    """NaN in all of W_2: V_2 is NaN, so every env whose option 2 goes on is interrupted and takes the root's finite values; the
    other options' kept envs are decided by value."""
    r, clf, pre = _edge(make, n, 3, 22)
    W = crossing_weights(4, 22)
    W[2] = np.nan
    out, got, _ = _check(r, pre, W, clf, 0b1110, n)
    k2 = out["keep"] & (out["vf"] == 2)
    assert k2.sum() >= 10 and out["interrupted"][k2].all()
    assert np.isfinite(got["st"]["qcache"][:, k2]).all()
    other = out["keep"] & (out["vf"] != 2)
    assert out["interrupted"][other].any() and not out["interrupted"][other].all()


def edge_nan_root_weights_interrupt(make, n=512):
    """NaN in all of W_0: V_0 is NaN, so every option that goes on is interrupted (its qcache: the root's NaN values)."""
    r, clf, pre = _edge(make, n, 3, 23)
    W = crossing_weights(4, 23)
    W[0] = np.nan
    out, got, _ = _check(r, pre, W, clf, 0b1110, n)
    keep = out["keep"]
    assert keep.sum() >= 30 and out["interrupted"][keep].all()
    assert np.isnan(got["st"]["qcache"][:, keep]).all()


def edge_nan_root_action_is_passed_over(make, n=512):
    """NaN in one action row of W_0: Q_0(., 3) is NaN everywhere and V_0 is the maxNum of the other four, so kept envs are still
    decided by value; an interrupted env's qcache holds the root's NaN for action 3 only."""
    r, clf, pre = _edge(make, n, 3, 24)
    W = crossing_weights(4, 24)
    W[0, 3, 100] = np.nan
    out, got, _ = _check(r, pre, W, clf, 0b1110, n)
    cut = out["interrupted"]
    assert cut.sum() >= 5 and (out["keep"] & ~cut).sum() >= 5
    q = got["st"]["qcache"][:, cut]
    assert np.isnan(q[3]).all() and np.isfinite(q[[0, 1, 2, 4]]).all()


def edge_candidate_kinds(make, n=768):
    """c is §4.2's candidate as if the option had ended: c == o (an env of option 1), c != o (option 2 inside I_1 too: the lower
    option wins) and c == 0 (option 3 gestating, outside every enabled option's set) in one batch. I_3 holds I_1 and I_2, so an env
    interrupted out of option 1 or 2 is also a gestation item of VF 3, whose target §12 leaves alone (r + γ m_3: the item
    neither succeeds nor fails)."""
    cx, cy = 0.35, 0.4                                     # pinball_empty: far from the goal disc at (0.8, 0.8)
    clf = np.zeros((4, 8), np.float32)
    clf[1] = disc_weights(cx - 0.08, cy, 0.15)
    clf[2] = disc_weights(cx + 0.08, cy, 0.15)
    clf[3] = disc_weights(cx, cy, 0.32)
    r, clf, pre = _edge(make, n, 3, 25, map_name="pinball_empty", clf=clf, ids=1 + np.arange(n) % 3, parents=[0, 0, 0, 0],
                        gest=0b1000)
    W = crossing_weights(4, 25)
    out, got, ok = _check(r, pre, W, clf, 0b0110, n)
    cut = out["interrupted"] & ok
    c, o = out["c"], out["vf"]
    kinds = [(cut & (c == o)).sum(), (cut & (c >= 1) & (c != o)).sum(), (cut & (c == 0)).sum()]
    assert min(kinds) >= 3, f"interrupted envs with c == o, c != o, c == 0: {kinds}"
    assert np.array_equal(got["st"]["option_id"][cut], -c[cut])
    assert (cut & (o <= 2)).sum() >= 3 and np.isin(out["items"][3], np.nonzero(cut & (o <= 2))[0]).sum() >= 3


def edge_option_time_limit(make, n=512):
    """opt_steps = max_option_steps - 1: the option times out (§4.2's otime), so it does not go on and is never interrupted; at
    max_option_steps - 2 it goes on and can be."""
    r, clf, pre = _edge(make, n, 3, 26)
    last = np.arange(n) % 2 == 0
    pre["opt_steps"][:] = np.where(last, MAX_OPT - 1, MAX_OPT - 2)
    W = crossing_weights(4, 26)
    out, got, _ = _check(r, pre, W, clf, 0b1110, n)
    cut, keep = out["interrupted"], out["keep"]
    assert (last & (out["vf"] >= 1)).sum() >= 30 and not keep[last].any() and not cut[last].any()
    assert cut[~last].sum() >= 5 and (keep & ~cut).sum() >= 5
    assert (got["st"]["opt_steps"][keep & ~cut] == MAX_OPT - 1).all()


def edge_disabled_and_gestating_ids(make, n=768):
    """An id naming a disabled option (3: neither enabled nor gestating) fails at once, its set being empty, and is never
    interrupted. An id naming a gestating option (2) can go on and be interrupted; its c never names 2 (a gestating option is not
    selected), so such envs write 0 or -1."""
    ids = np.array([1, 2, 3, -3, 0])[np.arange(n) % 5]
    r, clf, pre = _edge(make, n, 3, 27, ids=ids, gest=0b0100)
    W = crossing_weights(4, 27)
    out, got, _ = _check(r, pre, W, clf, 0b0010, n)
    cut, keep = out["interrupted"], out["keep"]
    o3, o2 = ids == 3, ids == 2
    assert not keep[o3].any() and not cut[o3].any() and (got["st"]["opt_steps"][o3] == 0).all()
    assert cut[o2].sum() >= 3 and (keep & ~cut)[o2].sum() >= 3
    assert (out["c"][o2 & cut] != 2).all()


def edge_out_of_range_ids_never_interrupt(make, n=768):
    """Ids outside (-n_vf, n_vf) name no option: the env runs the root, keeps nothing and is never interrupted, beside envs of
    the same batch whose options are interrupted."""
    nopt = 2
    wild = np.array([33, 257, nopt + 1, -(nopt + 1), -40])
    ids = np.where(np.arange(n) % 3 == 0, wild[np.arange(n) % 5], 1 + np.arange(n) % 2)
    r, clf, pre = _edge(make, n, nopt, 28, ids=ids)
    W = crossing_weights(nopt + 1, 28)
    out, got, _ = _check(r, pre, W, clf, 0b110, n)
    w = np.isin(ids, wild)
    assert not out["keep"][w].any() and not out["interrupted"][w].any() and (got["st"]["opt_steps"][w] == 0).all()
    assert out["interrupted"][~w].sum() >= 5


def edge_reoffer_every_step(make, n=512):
    """reoffer_period = 1: every step is a re-offer step and no env stays out, yet an interrupted env writes -c; the offer of c
    waits for its next step."""
    r, clf, pre = _edge(make, n, 3, 29, reoffer_period=1)
    W = crossing_weights(4, 29)
    out, got, ok = _check(r, pre, W, clf, 0b1110, n)
    cut = out["interrupted"] & ok & (out["c"] >= 1)
    assert cut.sum() >= 5 and not out["stay"].any()
    assert np.array_equal(got["st"]["option_id"][cut], -out["c"][cut])


EDGES = [edge_ties_never_interrupt, edge_nan_option_weights_interrupt, edge_nan_root_weights_interrupt,
         edge_nan_root_action_is_passed_over, edge_candidate_kinds, edge_option_time_limit, edge_disabled_and_gestating_ids,
         edge_out_of_range_ids_never_interrupt, edge_reoffer_every_step]


@pytest.mark.parametrize("edge", EDGES, ids=[e.__name__[5:] for e in EDGES])
def test_emulator_edge_case(edge):
    edge(EmulatorRunner)


# ---------------------------------------------------------------------------------------------------- mutations
# The emulator's correct outputs of one step, changed in one place each: compare() must refuse every one.

@pytest.fixture(scope="module")
def base():
    n, nopt = 1000, 5
    r = EmulatorRunner("pinball_simple", n, nopt, seed=17, env_id_base=7, reoffer_period=4)
    clf = chain_classifiers(r.map, nopt)
    rng = np.random.default_rng(17)
    pre = pre_state(r.map, n, nopt, rng, max_ep=MAX_EP, max_opt=MAX_OPT)
    seat_running_envs(r.map, pre, clf, r.model.parents, rng)
    W = random_weights(nopt + 1, 18, std=1e-3)
    enabled = 0b111110
    out, got, _ = check_step(r, pre, W, clf, 3, enabled, check_resolution=True)         # the outputs as they are pass
    plain, G_plain, _, _ = ilm.step(r.orc, pre, W, clf, 3, enabled, interrupt=False, recompute=True)
    ok = np.ones(n, bool)
    ok[out["ambiguous"]] = False
    cut = np.nonzero(out["interrupted"] & ok & (out["c"] >= 1))[0]
    assert len(cut) >= 10, len(cut)
    return SimpleNamespace(pre=pre, out=out, got=got, plain=plain, G_plain=G_plain, e=int(cut[0]))


def _refuse(b, st=None, G=None, n_k=None):
    g = b.got
    with pytest.raises(AssertionError):
        compare(b.out, g["st"] if st is None else st, g["G"] if G is None else G, g["n_k"] if n_k is None else n_k, g["W"],
                events=g["events"], ev_len=g["ev_len"], gest_succ=g["gest_succ"], check_resolution=True)


def _state(b):
    return {k: v.copy() for k, v in b.got["st"].items()}


def test_mutation_a_plain_G_with_interrupting_acting_outputs(base):
    _refuse(base, G=base.G_plain)


def test_mutation_b_no_id_where_c_names_an_option(base):
    st = _state(base)
    st["option_id"][base.e] = 0
    _refuse(base, st=st)


def test_mutation_c_qcache_of_the_interrupted_option(base):
    st = _state(base)
    st["qcache"][:, base.e] = base.plain["qcache"][:, base.e]              # the plain step's Q_o(s_next, .)
    _refuse(base, st=st)


def test_mutation_d_opt_steps_not_reset(base):
    st = _state(base)
    st["opt_steps"][base.e] = base.pre["opt_steps"][base.e] + 1
    _refuse(base, st=st)


def test_mutation_e_one_env_given_the_plain_step(base):
    st = _state(base)
    for f in scg.EnvState.FIELDS:
        st[f][..., base.e] = base.plain[f][..., base.e]
    _refuse(base, st=st)


def test_mutation_f_n_k_of_the_option_off_by_one(base):
    n_k = base.got["n_k"].copy()
    n_k[base.out["vf"][base.e]] += 1
    _refuse(base, n_k=n_k)
