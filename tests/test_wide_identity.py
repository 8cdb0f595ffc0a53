"""SPEC §2's 64-bit run identity on the CPU: the seed, the step counter t and the global env id past 2^32.

Every random draw is keyed by three 64-bit quantities that are split into 32-bit words for Philox. These tests put non-zero
bits into every upper word: the draw model (tests/draw_model.py) is shown to tell a wide value from its truncation, the oracle
is held to the draw model over the wide grid, the oracle's step-batch to the float64 model (tests/ref64.py) at wide
identities, and the host side refuses values outside the 64-bit ranges before anything is launched. The HIP side of the same
checks is tests/test_gpu_wide_identity.py."""
import math

import numpy as np
import pytest

import sc_oracle
import skill_chaining_with_graphs_amd as scg
from draw_model import WIDE_SEED, WIDE_T, draws, draws_batch, grid, seven_start_map, wide_bases
from test_ref64_oracle import SWEEP, TREE, OracleRunner, edge_reoffer_stagger_uses_global_id, sweep_case
from util import HP, SCALE

N = 1000
W_SEED, W_T = 2 ** 63 + 3, 2 ** 32 + 5
W_BASE = 2 ** 32 - N // 2
WIDE_STEPS = (2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1)


def _id(v):
    """A readable test id of a 64-bit value: 2^k+d."""
    v = int(v)
    if abs(v) < 2 ** 20:
        return str(v)
    k = round(math.log2(abs(v)))
    d = abs(v) - 2 ** k
    return ("-" if v < 0 else "") + (f"2^{k}{d:+d}" if d else f"2^{k}")


def grid_id(c):
    return "seed" + _id(c[0]) + "-base" + _id(c[1]) + "-t" + _id(c[2])


# ---------------------------------------------------------------------------------------------------- the model discriminates
# Without these a test at a wide value proves nothing about the upper word: a wide value and its truncation to 32 bits must
# give different draws (a random action differs with probability 4/5, a start index of 7 with 6/7; at least half is asked).

@pytest.mark.parametrize("others", [(W_SEED, W_BASE), (3, 0)], ids=["wide", "small"])
@pytest.mark.parametrize("t", [v for v in WIDE_T if v >= 2 ** 32], ids=_id)
def test_model_tells_a_wide_t_from_its_truncation(t, others):
    seed, base = others
    _, a, s = draws_batch(base, N, seed, t, 7)
    _, a32, s32 = draws_batch(base, N, seed, t % 2 ** 32, 7)
    assert np.mean(a != a32) >= 0.5 and np.mean(s != s32) >= 0.5, (np.mean(a != a32), np.mean(s != s32))


@pytest.mark.parametrize("others", [(W_T, W_BASE), (5, 0)], ids=["wide", "small"])
@pytest.mark.parametrize("seed", [v for v in WIDE_SEED if v >= 2 ** 32], ids=_id)
def test_model_tells_a_wide_seed_from_its_truncation(seed, others):
    t, base = others
    _, a, s = draws_batch(base, N, seed, t, 7)
    _, a32, s32 = draws_batch(base, N, seed % 2 ** 32, t, 7)
    assert np.mean(a != a32) >= 0.5 and np.mean(s != s32) >= 0.5, (np.mean(a != a32), np.mean(s != s32))


@pytest.mark.parametrize("others", [(W_SEED, W_T), (3, 5)], ids=["wide", "small"])
@pytest.mark.parametrize("base", [2 ** 32 - N // 2, 2 ** 32, 2 ** 40 + 3, -5], ids=_id)
def test_global_ids_2_pow_32_apart_share_a_stream(base, others):
    """SPEC §2: c0 = g mod 2^32. The opposite contract to t and the seed: g and g + 2^32 (and g mod 2^32) draw the same."""
    seed, t = others
    ref = draws_batch(base, N, seed, t, 7)
    for other in (base + 2 ** 32, base % 2 ** 32):
        for a, b in zip(ref, draws_batch(other, N, seed, t, 7)):
            assert np.array_equal(a, b)
    u, a, s = ref                                              # ... and neighbouring ids do not
    assert np.mean(a[1:] != a[:-1]) >= 0.5 and np.mean(s[1:] != s[:-1]) >= 0.5


def test_the_grid_holds_every_value_of_every_axis():
    for n in (1, N):
        g = grid(n)
        assert {c[0] for c in g} == set(WIDE_SEED) and {c[2] for c in g} == set(WIDE_T) and {c[1] for c in g} == set(wide_bases(n))
    inside = [W_BASE + e for e in range(N)]
    assert inside[N // 2 - 1] == 2 ** 32 - 1 and inside[N // 2] == 2 ** 32        # the wrap lies inside the batch (and inside
    assert (N // 2) % 64 != 0                                                      # a block, a wave)


# ---------------------------------------------------------------------------------------------------- the oracle's draws

def draw_case_state(m, n):
    """Pre-state of the draw cases: envs at rest in the free middle of the 7-start map (no goal within one step)."""
    st = sc_oracle.new_state(n, m)
    rng = np.random.default_rng(n)
    st["x"][:] = rng.uniform(0.2, 0.6, n)
    st["y"][:] = rng.uniform(0.4, 0.7, n)
    return st


def assert_draws(m, st, n, seed, base, t, eps=1.0, greedy=None, msg=""):
    """After one step with max_episode_steps = 1 from draw_case_state: the action is the draw model's (a_rand under eps = 1,
    else where(explore_u < float32(eps), a_rand, greedy)) and every env was reset to starts[start], bit for bit."""
    u, a_rand, start = draws_batch(base, n, seed, t, len(m.starts))
    want = a_rand if greedy is None else np.where(u < float(np.float32(eps)), a_rand, greedy)
    bad = np.nonzero(np.asarray(st["action"]).astype(np.int64) != want)[0]
    assert len(bad) == 0, f"{msg} action: {len(bad)} of {n} envs differ from the draw model, first {bad[:5].tolist()}"
    assert np.all(np.asarray(st["done"]) == 2), f"{msg} an env did not time out"
    S = np.asarray(m.starts, np.float32)
    for k, col in (("x", 0), ("y", 1)):
        bad = np.nonzero(np.asarray(st[k]).view(np.uint32) != S[start, col].view(np.uint32))[0]
        assert len(bad) == 0, f"{msg} {k}: {len(bad)} of {n} envs not at starts[start], first {bad[:5].tolist()}"


def _oracle(m, n, seed, base, eps):
    return sc_oracle.Oracle(m, SCALE, n_envs=n, n_options=0, seed=seed, env_id_base=base, n_threads=4,
                            **dict(HP, epsilon=eps, max_episode_steps=1))


@pytest.mark.parametrize("n", [N, 1])
@pytest.mark.parametrize("cell", grid(N), ids=grid_id)
def test_oracle_draws_match_the_model_over_the_grid(cell, n):
    seed, base, t = cell
    if n == 1:                                                 # the single env's id: bit 31 alone, and all 32 bits
        base = {2 ** 31 - N // 2: 2 ** 31, 2 ** 32 - N // 2: 2 ** 32 - 1}.get(base, base)
    m = seven_start_map()
    st = draw_case_state(m, n)
    _oracle(m, n, seed, base, 1.0).step(st, np.zeros((1, 5, 1296), np.float32), np.zeros((1, 8), np.float32), t)
    assert_draws(m, st, n, seed, base, t, msg=grid_id(cell))


def greedy_qcache(n):
    """(qcache [5, n], its greedy action): one action stands out per env."""
    greedy = (np.arange(n) * 3 + 1) % 5
    q = np.zeros((5, n), np.float32)
    q[greedy, np.arange(n)] = 1.0
    return q, greedy


@pytest.mark.parametrize("eps", [0.2, 0.7])
@pytest.mark.parametrize("cell", [(W_SEED, W_BASE, 2 ** 32 - 1), (W_SEED, W_BASE, 2 ** 64 - 1), (2 ** 64 - 1, 2 ** 40 + 3, 2 ** 32),
                                  (3, 0, 5)], ids=grid_id)
def test_oracle_explore_comparison_at_wide_identities(cell, eps):
    seed, base, t = cell
    m = seven_start_map()
    st = draw_case_state(m, N)
    st["qcache"][:], greedy = greedy_qcache(N)
    _oracle(m, N, seed, base, eps).step(st, np.zeros((1, 5, 1296), np.float32), np.zeros((1, 8), np.float32), t)
    assert_draws(m, st, N, seed, base, t, eps=eps, greedy=greedy, msg=grid_id(cell))
    u = draws_batch(base, N, seed, t, 7)[0]
    assert 0.5 * eps < np.mean(u < eps) < 1.5 * eps            # both branches of the comparison are taken


# ---------------------------------------------------------------------------------------------------- the step-batch

def wide_cfg(cfg):
    """A configuration of test_ref64_oracle.SWEEP moved to a base whose ids cross the 2^32 wrap inside the batch."""
    return cfg[:8] + (2 ** 32 - cfg[1] // 2,) + cfg[9:]


# one chain, two trees, two with gestation; N in {257, 1000}
WIDE_SWEEP = [wide_cfg(c) for c in SWEEP if (c[1], c[2]) in ((257, 5), (257, 3), (1000, 5), (1000, 4))]
assert len(WIDE_SWEEP) == 4 and any(c[3] is TREE for c in WIDE_SWEEP) and any(c[3] is None for c in WIDE_SWEEP) \
    and any(c[4] for c in WIDE_SWEEP)
SWEEP_IDS = [f"{c[0]}-{c[1]}-{c[2]}opt-{c[9]}" for c in WIDE_SWEEP]


@pytest.mark.parametrize("cfg", WIDE_SWEEP, ids=SWEEP_IDS)
def test_oracle_step_matches_the_float64_model_at_wide_identities(cfg):
    sweep_case(OracleRunner, cfg, 256, steps=WIDE_STEPS, seed=W_SEED)


@pytest.mark.parametrize("period", [4, 8])
def test_oracle_reoffer_stagger_across_the_wrap(period):
    """(t + g) mod period with t at 2^32 - 1 and 2^32 and ids that cross 2^32 inside the batch."""
    edge_reoffer_stagger_uses_global_id(OracleRunner, seed=W_SEED, env_id_base=2 ** 32 - 128, period=period,
                                        steps=(2 ** 32 - 1, 2 ** 32))


def test_step_model_forms_the_stagger_mod_2_pow_64():
    """StepModel at t = 2^64 - 1 and a negative base: the stagger is ((t + g) mod 2^64) mod period, formed without int64 or
    float64 on the way (checked here against the oracle through the same edge)."""
    edge_reoffer_stagger_uses_global_id(OracleRunner, seed=W_SEED, env_id_base=-100, period=4, steps=(2 ** 64 - 1, 2 ** 63))


# ---------------------------------------------------------------------------------------------------- host-side refusals

@pytest.mark.parametrize("kw", [dict(seed=2 ** 64), dict(seed=-1), dict(env_id_base=2 ** 63), dict(env_id_base=-2 ** 63 - 1)],
                         ids=lambda kw: "-".join(f"{k}{_id(v)}" for k, v in kw.items()))
def test_context_refuses_an_identity_outside_64_bits_before_any_device_call(kw):
    """ctypes would mask these into range silently (seed = -1 becoming 2^64 - 1). The check precedes the look for a GPU and
    the library load: it raises on a host without either."""
    with pytest.raises(scg.ScgError, match="64-bit"):
        scg.ScgContext(4, 0, scg.load_map("pinball_empty"), **kw)


@pytest.mark.parametrize("t", [-1, 2 ** 64], ids=_id)
def test_step_refuses_a_counter_outside_64_bits_before_anything_else(t):
    """step(t = -1) would run as t = 2^64 - 1 and step(t = 2^64) as t = 0. The check comes first — before the operands are
    looked at and before the cached-argument fast path — so it can be shown on an object that has no context at all."""
    ctx = object.__new__(scg.ScgContext)
    with pytest.raises(scg.ScgError, match="step: t must be a 64-bit unsigned step counter"):
        ctx.step(None, None, None, 0, t)
