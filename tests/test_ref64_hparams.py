"""The step-batch at the edges of its hyper-parameters against the float64 model (tests/ref64.py), on the CPU.

The sweeps of tests/test_ref64_oracle.py and tests/test_ref64_interrupt.py hold gamma, alpha, the success reward and both step
limits at tests/util.py's HP and the weights at std 1e-3. Here one setting per case goes to an end of its domain (include/scg_abi.h
names the domains) while the rest stays at HP: gamma 0 and 1, alpha 0 and 1, a zero, a negative and a huge success reward, step
limits of 1 and 2 (`opt_steps + 1 >= max_option_steps` and `ep_steps + 1 >= max_episode_steps` fire on the first step), re-offer
periods 0, 1, 2 and 2^20 at env id bases on both sides of a multiple of 2^20, count floors of 1, just above the env count and
2^30, and weights of trained size. Every case steps plain (the oracle) and interrupting (SPEC §12, the emulator of
tests/interrupt_learning_model.py) at t = 0, 1, 2 from fresh pre-states made with the case's OWN limits, so that the envs "about
to time out" sit at the real limits. Comparisons are ref64.compare's (discrete fields exact, floats within the model's bounds,
the tolerance below the single-item resolution); what an edge implies exactly is asserted exactly.

tests/test_gpu_ref64_hparams.py runs the same cases on the HIP path."""
import numpy as np
import pytest

from ref64 import clf_model, env_order_layout
from test_ref64_interrupt import EmulatorRunner, seat_running_envs
from test_ref64_oracle import TREE, OracleRunner, assert_rarely_ambiguous, check_step, pre_state, tree_classifiers
from util import HP, chain_classifiers, oracle_block, random_weights

WIDE = 1 << 20                                # the large re-offer period: its mask 2^20 - 1 opens for one env id in 2^20
BASES = (0, WIDE - 100)                       # env ids 0..256 (t + g = 0 at t = 0 only) and ids that cross 2^20 (one env per step)


def _case(name, *, std=1e-3, base=0, map_name="pinball_simple", n=257, nopt=3, parents=None, dist="uniform", **hp):
    return dict(name=name, std=std, base=base, map_name=map_name, n=n, nopt=nopt, parents=parents, dist=dist, hp=hp)


HP_CASES = (
    [_case(f"gamma{g:g}", gamma=g) for g in (0.0, 1.0)]
    + [_case(f"alpha{a:g}", alpha=a) for a in (0.0, 1.0)]                       # (alpha 1 with std 1e-3 weights only)
    + [_case(f"rsucc{r:g}", r_option_success=r) for r in (0.0, -50.0, 1e4)]
    + [_case(f"maxopt{k}", max_option_steps=k) for k in (1, 2)]
    + [_case(f"maxep{k}", max_episode_steps=k) for k in (1, 2)]
    + [_case(f"reoffer{p}-base{b}", base=b, reoffer_period=p) for p in (0, 1, 2, WIDE) for b in BASES]
    # one more base than the two above: with ids round 2^19, t + g passes a number whose low 19 bits are zero and whose bit 19 is
    # set. No env may be re-offered there; a gate that dropped the mask's top bit would open (neither base above can show that)
    + [_case(f"reoffer{WIDE}-base{WIDE // 2 - 100}", base=WIDE // 2 - 100, reoffer_period=WIDE)]
    + [_case(f"floor{f}", update_count_floor=f) for f in (1, 257, 1 << 30)]
    + [_case("eps0-maxopt1-maxep1", epsilon=0.0, max_option_steps=1, max_episode_steps=1)]
    # weights of trained size. These two cases alone are compared WITHOUT compare()'s check_resolution. That check is a property
    # of the inputs, not of the system under test: it asks that every update item's |delta| exceed the tolerance of its action's
    # sum. With std 1e-3 weights every ordinary delta is r = -1 to within 0.05; with values of order 1..30 the deltas r + gamma V'
    # - Q(s, a) of a thousand items spread over an interval of that width round zero, so some item always lies within the
    # tolerance (measured: std 0.05, tolerance 0.156 against a smallest |delta| of 0.011; std 1, 0.415 against 0.157). Such an
    # item contributes nothing to G whether it is there or not. The exact n_k and the exact discrete fields still place each item.
    + [_case(f"std{s:g}", std=s) for s in (0.05, 1.0)]
    # the padded env order (SPEC §5) on both block builds: 1000 envs, nine in ten running one of five options
    + [_case("maze1000-tree", map_name="pinball_maze", n=1000, nopt=5, parents=TREE, dist="heavy")]
)
for _i, _c in enumerate(HP_CASES):
    _c["rng"] = 4000 + _i
HP_CASES[-1]["rng"] = 4027                    # (a seed whose first option mix is padded on the 64-env build too, not only on 256)
CASE_IDS = [c["name"] for c in HP_CASES]


def case_classifiers(case, m):
    return tree_classifiers(m)[:case["nopt"] + 1] if case["parents"] is not None else chain_classifiers(m, case["nopt"])


def _seat_gate_probes(m, pre, clf, probes, rng):
    """Put the envs `probes` and their successors at rest well inside I_3 and outside I_2 (option 3's target region), at the start
    of an episode, staying out of option 3 (option_id = -3). These cases run with W_3 = W_0, an exact tie that the value gate
    accepts: an env that is offered option 3 enters it (an offer that the gate declines writes -3 again and could not be told
    from no offer), so whether its id becomes 3 is the re-offer gate's alone."""
    n = len(pre["x"])
    pool = m.sample_free(4096, rng, margin=2.0)
    z3, z2 = clf_model(clf[3], pool[:, 0], pool[:, 1])[0], clf_model(clf[2], pool[:, 0], pool[:, 1])[0]
    pts = pool[(z3 > 0.2) & (z2 < -0.2)]
    assert len(pts) >= 8
    who = sorted({e for p in probes for e in (p, p + 1) if e < n})
    for i, e in enumerate(who):
        pre["x"][e], pre["y"][e] = pts[i % len(pts)]
        pre["vx"][e] = pre["vy"][e] = 0.0
        pre["option_id"][e], pre["opt_steps"][e], pre["ep_steps"][e] = -3, 0, 0
    return who


def _edge_properties(case, hp, r, pre, W, out, got, msg):
    """What the case's edge implies exactly, beyond the model's comparison."""
    st = got["st"]
    if hp["gamma"] == 0.0:                     # the target is r alone, for continuing and ending items alike: no Q(s') in G
        for k in out["items"]:
            assert np.array_equal(out["item_targets"][k], out["item_rewards"][k]), f"{msg} VF {k}: a target depends on Q(s')"
    if hp["alpha"] == 0.0:                     # a step of size 0: W bit for bit as before, G and n_k checked as ever
        assert np.array_equal(got["W"].view(np.uint32), W.view(np.uint32)), f"{msg} alpha = 0 moved W"
        assert got["n_k"][0] == len(pre["x"]) and np.any(got["G"] != 0)
    if hp["max_option_steps"] == 1:            # every option step is a time-out: no option goes on
        assert not out["keep"].any() and not out["interrupted"].any()
        assert (st["opt_steps"] == 0).all(), f"{msg} opt_steps above 0 at max_option_steps = 1"
        assert (out["vf"] >= 1).sum() >= 20
    if hp["max_episode_steps"] == 1:           # every env ends its episode, by the goal (1) or by the limit (2), and is re-dealt
        assert (st["done"] != 0).all(), f"{msg} an env went on at max_episode_steps = 1"
        assert np.array_equal(st["done"] == 1, (out["events"] & 1) == 1)
        assert (st["ep_steps"] == 0).all() and (st["vx"] == 0).all() and (st["vy"] == 0).all()
        starts = {(float(a), float(b)) for a, b in np.asarray(r.map.starts, np.float32)}
        assert {(float(a), float(b)) for a, b in zip(st["x"], st["y"])} <= starts
        assert (st["done"] == 2).sum() >= len(pre["x"]) - 8


def hparam_case(make, case, block_envs, steps=(0, 1, 2)):
    """One case on the system under test `make` (a runner class; `interrupt` set on it steps SPEC §12's learner): three steps from
    fresh pre-states against the model, the case's exact properties, the ambiguity cap, and that the case is not vacuous."""
    hp = dict(HP, update_count_floor=0, reoffer_period=4)
    hp.update(case["hp"])
    n, nopt, base, period = case["n"], case["nopt"], case["base"], hp["reoffer_period"]
    r = make(case["map_name"], n, nopt, seed=11 + n, env_id_base=base, parents=case["parents"], **case["hp"])
    interrupt = getattr(r, "interrupt", False)
    clf = case_classifiers(case, r.map)
    enabled = (1 << (nopt + 1)) - 2
    rng = np.random.default_rng(case["rng"])
    W = random_weights(nopt + 1, n + 1, std=case["std"])
    if period == WIDE:
        W[3] = W[0]                            # (see _seat_gate_probes)
    n_amb = n_int = n_stay = n_reoffered = n_half = 0
    layouts = set()
    for t in steps:
        msg = f"{case['name']} t={t}:"
        pre = pre_state(r.map, n, nopt, rng, max_ep=hp["max_episode_steps"], max_opt=hp["max_option_steps"], dist=case["dist"])
        seat_running_envs(r.map, pre, clf, r.model.parents, rng)
        half = []
        if period == WIDE:                     # the envs whose t + g is a multiple of HALF the period: the one the gate opens for
            half = [e for e in range(n) if (t + base + e) % (period // 2) == 0]        # and the one only a narrower mask would
            _seat_gate_probes(r.map, pre, clf, half, rng)
        layouts.add(env_order_layout(pre["option_id"], nopt + 1, block_envs))
        out, got, a = check_step(r, pre, W, clf, t, enabled, check_resolution=case["std"] <= 1e-3, msg=msg)
        _edge_properties(case, hp, r, pre, W, out, got, msg)
        ok = np.ones(n, bool)
        ok[out["ambiguous"]] = False
        oid = pre["option_id"].astype(np.int64)
        n_amb += a
        n_int += int(out["interrupted"].sum())
        n_stay += int((out["stay"] & ok).sum())
        n_reoffered += int(((oid < 0) & (oid == -out["cand"]) & out["entering"] & (out["done"] == 0) & ok).sum())
        for e in half:
            assert e not in out["ambiguous"] and out["cand"][e] == 3 and not out["declined"][e], f"{msg} the probe env {e} is no probe"
            if (t + base + e) % period != 0:   # bit log2(period) - 1 alone is set: the gate stays shut
                assert out["stay"][e] and got["st"]["option_id"][e] == -3, f"{msg} env {e} was re-offered at half the period"
                n_half += 1
            else:                              # the gate opens: offered, and entered
                assert out["entering"][e] and got["st"]["option_id"][e] == 3, f"{msg} env {e} was not re-offered"
    print(f"\n[{case['name']} B={block_envs} interrupt={interrupt}] layouts {sorted(layouts)}, {n_int} interrupted, {n_stay} stayed out, "
          f"{n_reoffered} re-offered, {n_amb} ambiguous in {len(steps) * n} env-steps")
    assert_rarely_ambiguous(n_amb, len(steps) * n, case["name"])
    if "reoffer_period" not in case["hp"]:
        pass
    elif period <= 1:                          # every step is a re-offer step
        assert n_stay == 0 and n_reoffered >= 1
    elif base + n + max(steps) < period and base > 0:      # no multiple of the period in reach: the gate never opens
        assert n_reoffered == 0 and n_stay >= 1 and n_half >= 1
    else:                                      # a case that is silently all-or-nothing proves little
        assert n_reoffered >= 1 and n_stay >= 1, f"{n_reoffered} envs re-offered, {n_stay} stayed out"
    if interrupt and hp["max_option_steps"] >= 3 and hp["max_episode_steps"] >= 2:
        assert n_int >= 3, f"only {n_int} interrupted envs: the case is (nearly) vacuous"
    return layouts


RUNNERS = {"plain": OracleRunner, "interrupting": EmulatorRunner}


@pytest.mark.parametrize("mode", list(RUNNERS))
@pytest.mark.parametrize("case", HP_CASES, ids=CASE_IDS)
def test_oracle_at_hyperparameter_edges(case, mode):
    hparam_case(RUNNERS[mode], case, 256)


@pytest.mark.parametrize("mode", list(RUNNERS))
def test_oracle_at_hyperparameter_edges_on_the_64_env_build(mode):
    """The 1000-env case on the oracle's 64-env build (16 blocks, the last one partial)."""
    with oracle_block(64):
        hparam_case(RUNNERS[mode], HP_CASES[-1], 64)


def test_cases_change_one_setting_and_cover_the_padded_layout():
    """Every case but the combined one changes at most one setting of HP; the case list holds every edge named in the module's
    docstring; and the 1000-env case puts SPEC §5's padded layout in front of both block builds."""
    import skill_chaining_with_graphs_amd as scg
    for c in HP_CASES:
        assert len(c["hp"]) <= 1 or c["name"] == "eps0-maxopt1-maxep1", c["name"]
    assert len(CASE_IDS) == len(set(CASE_IDS))
    big = HP_CASES[-1]
    for b in (256, 64):
        rng = np.random.default_rng(big["rng"])
        pre = pre_state(scg.load_map(big["map_name"]), big["n"], big["nopt"], rng, max_ep=HP["max_episode_steps"],
                        max_opt=HP["max_option_steps"], dist=big["dist"])
        assert env_order_layout(pre["option_id"], big["nopt"] + 1, b) == "padded", b
