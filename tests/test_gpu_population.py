"""SPEC §21 population rollouts on the GPU (scg_rollout_population): every policy's env range equals by bits what scg_rollout_branch
writes on a context of n_per envs under that policy alone — the yardstick is always the existing entry point on the small context,
never the new one. Shapes, launch geometries, the four `rules`, BEGIN_AT with a force and a first action, a record window across a
policy boundary, the block builds; common random numbers; pop = NULL and C = 1; the refusals in their sequence; and the agent's
evaluate_policies() against evaluate() per policy, and improve_policy().

The map has eight starts on a ring just outside a large goal (and one far away), so that episodes of a dozen steps end at the goal;
options, parents and classifiers are tests/util.py's sibling tree on it, the weights crossing_weights plus seeded noise per policy."""
import ctypes as C

import numpy as np
import pytest
import torch

import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd._lib import Population, ScgError
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.evaluation import EpisodeStats, GateAudit, paired_differences
from skill_chaining_with_graphs_amd.trajectory import Trajectory
from skill_chaining_with_graphs_amd.valuefit import damped_tables
from gpu_util import (as_bytes, block_envs, clone_state, crossing_agent, current_block_envs, dev, make_context,  # noqa: F401
                      spy_calls, state_to_device)                                                            # (block_envs: the fixture)
from util import HP, crossing_weights, random_env_state, sibling_tree

pytestmark = pytest.mark.gpu

STATS = EpisodeStats.FIELDS
AUDIT = tuple(GateAudit.DTYPES)[1:]                    # the audit's outputs (every member but force)
INT, BEST = _lib.SELECT_INTERRUPT, _lib.SELECT_BEST
B, ONE, AT = _lib.ROLLOUT_BEGIN, _lib.ROLLOUT_ONE_EPISODE, _lib.ROLLOUT_BEGIN_AT
ALL_RULES = [0, INT, BEST, BEST | INT]
RULE_IDS = ["plain", "interrupt", "best", "best+interrupt"]
N_OPT, SEED, REOFFER, MAX_EP = 5, 3, 4, 12
K, T0 = 8, 40                                          # two launches of K steps end every episode (MAX_EP = 12)
MASK_ARG = 0b111110                                    # the call's own enabled_mask: no policy's, so a policy that read it shows
GUARD, G8 = -777.25, 77
EPS = (0.0, 0.1, 0.5)


def _map():
    ring = " ".join(f"{0.75 + 0.105 * np.cos(a):.4f} {0.75 + 0.105 * np.sin(a):.4f}" for a in np.arange(8) * np.pi / 4)
    return scg.parse_map("\n".join([
        "ball 0.02", "target 0.75 0.75 0.1", f"start 0.2 0.2 {ring}",
        "polygon 0.0 0.0 0.0 0.01 1.0 0.01 1.0 0.0", "polygon 0.0 0.0 0.01 0.0 0.01 1.0 0.0 1.0",
        "polygon 0.0 1.0 0.0 0.99 1.0 0.99 1.0 1.0", "polygon 1.0 1.0 0.99 1.0 0.99 0.0 1.0 0.0"]), "goal_ring")


def _context(m, parents, n, epsilon, block=None):
    return make_context(m, n, N_OPT, block, parents, 0, SEED, reoffer_period=REOFFER,
                        **dict(HP, max_episode_steps=MAX_EP, epsilon=epsilon))


def _policies(n_pol, same=False):
    """(W [C][6][5][1296], epsilon [C], enabled [C]) on the host: root + options 1 and 2 enabled, the last of two or more policies
    with option 2 disabled; distinct tables (seeded noise) unless `same`."""
    W0 = crossing_weights(N_OPT + 1, 6)
    W = np.stack([W0 if same or c == 0 else
                  W0 + (np.random.default_rng(100 + c).standard_normal(W0.shape) * 0.05).astype(np.float32) for c in range(n_pol)])
    enabled = np.full(n_pol, 0b110, np.int32)
    if n_pol >= 2 and not same:
        enabled[-1] = 0b010
    eps = np.full(n_pol, 0.1, np.float32) if same else np.asarray(EPS[:n_pol], np.float32)
    return W.astype(np.float32), eps, enabled


class Run:
    """A context's env state and everything a launch can write besides it, the audit's outputs prefilled with guards."""

    def __init__(self, ctx, st_np, rows=2 * K + 1, window=None, force=None):
        n = ctx.n_envs
        self.ctx, self.n = ctx, n
        self.st = state_to_device(st_np, ctx)
        self.stats = EpisodeStats(ctx.n_vf, n, ctx.device)
        self.window = (0, n) if window is None else window           # (first, count); count 0: no record
        self.rec = Trajectory(self.window[1], rows, self.window[0], ctx.device, n_vf=ctx.n_vf) if self.window[1] else None
        self.interrupts = torch.zeros((ctx.n_vf, n), dtype=torch.int32, device=ctx.device)
        self.overrides = torch.zeros((ctx.n_vf, n), dtype=torch.int32, device=ctx.device)
        self.audit = GateAudit(n, ctx.device, force=force)
        self.audit.applied.fill_(G8)
        self.audit.cand.fill_(G8)
        for f in ("v_root", "v_cand", "disc_final"):
            getattr(self.audit, f).fill_(GUARD)

    def args(self, W, clf, mask, t0, n_steps, flags, rules, first):
        cs, au = self.stats.c_struct(), self.audit.c_struct()
        rc = None if self.rec is None else self.rec.c_struct()
        keep = (cs, rc, au)
        p = lambda t: C.c_void_p(t.data_ptr())
        return keep, [p(getattr(self.st, f)) for f in EnvState.FIELDS] + [
            p(W), p(clf), C.c_uint32(mask), C.c_uint64(t0), C.c_int32(n_steps), C.c_uint32(flags), C.byref(cs),
            p(self.interrupts), p(self.overrides), None if rc is None else C.byref(rc), C.c_uint32(rules), C.byref(au),
            None if first is None else p(first), self.ctx._stream()]

    def branch(self, W, clf, mask, t0, n_steps, flags, rules, first=None):
        """The yardstick: scg_rollout_branch."""
        keep, a = self.args(W, clf, mask, t0, n_steps, flags, rules, first)
        self.ctx._call("scg_rollout_branch", *a)

    def population(self, W, clf, mask, t0, n_steps, flags, rules, pop, first=None):
        keep, a = self.args(W, clf, mask, t0, n_steps, flags, rules, first)
        self.ctx._call("scg_rollout_population", *a, None if pop is None else C.byref(pop))

    def outputs(self):
        """Every output as host arrays whose last axis is the env (the record's: its window's column)."""
        torch.cuda.synchronize()
        out = {f: getattr(self.st, f).cpu().numpy().reshape(-1, self.n) for f in EnvState.FIELDS}
        out.update({"stats." + f: getattr(self.stats, f).cpu().numpy().reshape(-1, self.n) for f in STATS})
        out["interrupts"], out["overrides"] = self.interrupts.cpu().numpy(), self.overrides.cpu().numpy()
        out.update({"audit." + f: getattr(self.audit, f).cpu().numpy().reshape(1, self.n) for f in AUDIT})
        rec = {}
        if self.rec is not None:
            rec = {f: getattr(self.rec, f).cpu().numpy() for f in self.rec.fields}
            rec["len"] = self.rec.len.cpu().numpy().reshape(1, -1)
        return out, rec


def _pop_struct(n_pol, n_per, eps, enabled):
    return Population(n_pol, n_per, None if eps is None else C.c_void_p(eps.data_ptr()),
                      None if enabled is None else C.c_void_p(enabled.data_ptr()))


def _clip(window, lo, hi):
    """The part of a record window (first, count) inside the envs lo .. hi - 1, relative to lo."""
    a, b = max(window[0], lo), min(window[0] + window[1], hi)
    return (a - lo, max(b - a, 0))


def _slice_state(st_np, lo, hi):
    return {f: np.ascontiguousarray(v[..., lo:hi]) for f, v in st_np.items()}


def _assert_slice(got, want, lo, hi, window, msg):
    """Policy range lo .. hi - 1 of the population's outputs `got` against the single run's `want`, by bits."""
    (g, g_rec), (w, w_rec) = got, want
    for f in w:
        assert np.array_equal(as_bytes(np.ascontiguousarray(g[f][:, lo:hi])), as_bytes(w[f])), f"{msg}: {f} differs"
    first, cnt = _clip(window, lo, hi)
    assert bool(w_rec) == (cnt > 0)
    at = first + lo - window[0]
    for f in w_rec:
        assert np.array_equal(as_bytes(np.ascontiguousarray(g_rec[f][:, at:at + cnt])), as_bytes(w_rec[f])), f"{msg}: record {f} differs"


LAUNCHES = ((T0, K, B | ONE), (T0 + K + 1, K, ONE))


def _singles(m, parents, clf, pol, st_np, n_per, rules, launches=LAUNCHES, window=None, force=None, first=None, block=None):
    """The yardstick: per policy, the launches on a context of n_per envs under that policy; the outputs after each launch."""
    W, eps, enabled = pol
    out = []
    for c in range(len(eps)):
        lo, hi = c * n_per, (c + 1) * n_per
        ctx = _context(m, parents, n_per, float(eps[c]), block)
        run = Run(ctx, _slice_state(st_np, lo, hi), window=None if window is None else _clip(window, lo, hi),
                  force=None if force is None else force[lo:hi])
        Wc, fa = dev(W[c]).view(-1), None if first is None else dev(first[lo:hi])
        snaps = []
        for t0, k, flags in launches:
            run.branch(Wc, clf, int(enabled[c]), t0, k, flags, rules, fa)
            snaps.append(run.outputs())
        out.append(snaps)
        ctx.close()
    return out


def _population(m, parents, clf, pol, st_np, n_per, rules, launches=LAUNCHES, window=None, force=None, first=None, block=None):
    W, eps, enabled = pol
    n_pol = len(eps)
    ctx = _context(m, parents, n_pol * n_per, 0.3, block)              # (the context's own epsilon is no policy's)
    run = Run(ctx, st_np, window=window, force=force)
    Wd, ed, md = dev(W).view(-1), dev(eps), dev(enabled)
    pop = _pop_struct(n_pol, n_per, ed, md)
    fa = None if first is None else dev(first)
    snaps = []
    for t0, k, flags in launches:
        run.population(Wd, clf, MASK_ARG, t0, k, flags, rules, pop, fa)
        snaps.append(run.outputs())
    ctx.close()
    return snaps


def _inputs(n):
    m = _map()
    parents, clf = sibling_tree(m)
    st_np = random_env_state(m, n, N_OPT, 9, id_lo=-N_OPT, id_hi=N_OPT, opt_steps_hi=10, max_episode_steps=MAX_EP)
    return m, parents, dev(clf).view(-1), st_np


def _compare(pop_snaps, singles, n_per, window, msg):
    for c, snaps in enumerate(singles):
        for j, (got, want) in enumerate(zip(pop_snaps, snaps)):
            _assert_slice(got, want, c * n_per, (c + 1) * n_per, window, f"{msg} policy {c} launch {j}")


def _conditions(singles, msg):
    """On the yardstick's side: some policy enters options, some episode ends at the goal, every episode has ended, and two
    policies end in different states."""
    last = [s[-1][0] for s in singles]
    entries = [int(o["stats.entries"].sum()) for o in last]
    goals = [int(o["stats.goals"].sum()) for o in last]
    print(f"{msg}: entries {entries}, goals {goals}, episodes {[int(o['stats.episodes'].sum()) for o in last]}")
    assert max(entries) > 0 and max(goals) > 0, msg
    if len(last) >= 2:
        assert any(not np.array_equal(last[0]["x"], o["x"]) for o in last[1:]), f"{msg}: every policy ends in the same states"


# ---------------------------------------------------------------------------------------------------- 1. the identity

SHAPES = [(1, 40), (3, 40), (3, 257), (2, 600)]


@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_policy_range_is_the_single_policy_rollout(shape, rules, monkeypatch):
    n_pol, n_per = shape
    n = n_pol * n_per
    m, parents, clf, st_np = _inputs(n)
    pol = _policies(n_pol)
    monkeypatch.delenv("SCG_ROLLOUT_EPW", raising=False)
    singles = _singles(m, parents, clf, pol, st_np, n_per, rules)
    _conditions(singles, f"{shape} rules {rules}")
    assert all(int(s[-1][0]["stats.finished"].sum()) == n_per for s in singles)         # two launches end every episode ...
    assert any(int(s[0][0]["stats.finished"].sum()) < n_per for s in singles)           # ... and the second one resumes some
    for epw in (None, 2, 32):
        if epw is not None:
            monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
        _compare(_population(m, parents, clf, pol, st_np, n_per, rules), singles, n_per, (0, n), f"{shape} rules {rules} epw {epw}")


# ---------------------------------------------------------------------------------------------------- 2. further identity cases

def test_begin_at_with_a_force_and_a_first_action():
    n_pol, n_per = 3, 40
    n = n_pol * n_per
    m, parents, clf, st_np = _inputs(n)
    pol = _policies(n_pol)
    e = np.arange(n)
    force = ((e * 5 + e // n_per) % 5 - 2).astype(np.int8)                 # -2 .. +2, another pattern in every policy's range
    first = ((e * 7 + 3 * (e // n_per)) % 6).astype(np.uint8)             # 5: not forced
    assert not np.array_equal(force[:n_per], force[n_per:2 * n_per]) and not np.array_equal(first[:n_per], first[n_per:2 * n_per])
    launches = ((T0, 2 * K, AT),)                                         # (a force needs a begin flag: one launch)
    kw = dict(launches=launches, force=force, first=first)
    singles = _singles(m, parents, clf, pol, st_np, n_per, BEST | INT, **kw)
    _conditions(singles, "begin_at")
    applied = np.concatenate([s[0][0]["audit.applied"][0] for s in singles])
    assert (applied == 1).any() and (applied == 0).any()
    assert all(np.array_equal(s[0][1]["action"][1][first[c * n_per:(c + 1) * n_per] < 5], first[c * n_per:(c + 1) * n_per][first[c * n_per:(c + 1) * n_per] < 5])
               for c, s in enumerate(singles))
    _compare(_population(m, parents, clf, pol, st_np, n_per, BEST | INT, **kw), singles, n_per, (0, n), "begin_at")


def test_a_record_window_across_a_policy_boundary():
    n_pol, n_per, window = 3, 40, (30, 35)                                # policy 0's envs 30 .. 39, policy 1's 40 .. 64, none of 2's
    m, parents, clf, st_np = _inputs(n_pol * n_per)
    pol = _policies(n_pol)
    singles = _singles(m, parents, clf, pol, st_np, n_per, 0, window=window)
    assert [bool(s[0][1]) for s in singles] == [True, True, False]
    _compare(_population(m, parents, clf, pol, st_np, n_per, 0, window=window), singles, n_per, window, "window")


@pytest.mark.parametrize("block_envs", [64, 128, 256], indirect=True)
def test_every_block_build(block_envs):
    n_pol, n_per = 3, 40
    m, parents, clf, st_np = _inputs(n_pol * n_per)
    pol = _policies(n_pol)
    singles = _singles(m, parents, clf, pol, st_np, n_per, INT, block=current_block_envs())
    pop = _population(m, parents, clf, pol, st_np, n_per, INT, block=current_block_envs())
    _compare(pop, singles, n_per, (0, n_pol * n_per), f"block {block_envs}")


# ---------------------------------------------------------------------------------------------------- 3. common random numbers

def test_equal_policies_give_equal_ranges_and_all_share_their_starts():
    n_pol, n_per = 3, 257
    n = n_pol * n_per
    m, parents, clf, st_np = _inputs(n)
    st_np = _slice_state(st_np, 0, n_per)
    st_np = {f: np.concatenate([v] * n_pol, axis=-1) for f, v in st_np.items()}          # one input state for every policy
    out, rec = _population(m, parents, clf, _policies(n_pol, same=True), st_np, n_per, BEST | INT)[-1]
    for f, v in list(out.items()) + list(rec.items()):
        for c in (1, 2):
            assert np.array_equal(as_bytes(np.ascontiguousarray(v[:, :n_per])), as_bytes(np.ascontiguousarray(v[:, c * n_per:(c + 1) * n_per]))), \
                f"{f}: policy {c}'s range differs from policy 0's"
    assert int(out["stats.episodes"].sum()) == n
    W, eps, enabled = _policies(n_pol)
    (out, rec), _ = _population(m, parents, clf, (W, np.zeros(n_pol, np.float32), enabled), st_np, n_per, 0)
    assert (rec["action"][0] == 255).all()                                               # the begin row: the drawn start state
    for f in ("x", "y", "vx", "vy"):
        for c in (1, 2):
            assert np.array_equal(as_bytes(np.ascontiguousarray(rec[f][0, :n_per])), as_bytes(np.ascontiguousarray(rec[f][0, c * n_per:(c + 1) * n_per])))
    assert len(np.unique(rec["x"][0, :n_per])) >= 5                                      # ... which differ from env to env
    assert not np.array_equal(out["x"][:, :n_per], out["x"][:, n_per:2 * n_per])       # the weights reached the kernel


# ---------------------------------------------------------------------------------------------------- 4. pop = NULL, C = 1

@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
def test_null_pop_and_one_policy_are_the_branch_rollout(rules):
    n = 130
    m, parents, clf, st_np = _inputs(n)
    W = dev(_policies(1)[0][0]).view(-1)
    first = dev(((np.arange(n) * 3) % 7).astype(np.uint8))
    ctx = _context(m, parents, n, 0.3)
    ref = Run(ctx, st_np)
    runs = {"pop = NULL": (Run(ctx, st_np), None), "C = 1, members NULL": (Run(ctx, st_np), _pop_struct(1, n, None, None))}
    for t0, k, flags in LAUNCHES:
        ref.branch(W, clf, 0b110, t0, k, flags, rules, first)
        want = ref.outputs()
        for how, (run, pop) in runs.items():
            run.population(W, clf, 0b110, t0, k, flags, rules, pop, first)
            _assert_slice(run.outputs(), want, 0, n, (0, n), f"rules {rules} {how}")
    assert int(ref.stats.entries.sum()) > 0 and int(ref.stats.goals.sum()) > 0


# ---------------------------------------------------------------------------------------------------- 5. refusals

def test_refusals_in_their_sequence_launch_nothing():
    n_pol, n_per = 3, 40
    n = n_pol * n_per
    m, parents, clf, st_np = _inputs(n)
    W, eps, enabled = _policies(n_pol)
    Wd, ed, md = dev(W).view(-1), dev(eps), dev(enabled)
    ctx = _context(m, parents, n, 0.3)
    run = Run(ctx, st_np, rows=2)
    before = clone_state(run.st)
    for f in STATS:
        getattr(run.stats, f).fill_(77)
    run.interrupts.fill_(77)
    run.overrides.fill_(77)
    first = torch.full((n,), 3, dtype=torch.uint8, device=ctx.device)
    lib = ctx.lib

    def call(pop, flags=B, n_steps=1, rules=0, c=ctx._ctx):
        keep, a = run.args(Wd, clf, MASK_ARG, 0, n_steps, flags, rules, first)
        rc = lib.scg_rollout_population(c, *a, None if pop is None else C.byref(pop))
        return rc, lib.scg_last_error(c).decode()

    name = "scg_rollout_population: "
    bad = [(_pop_struct(0, n, ed, md), "pop->n_policies out of range [1, SCG_POP_MAX]"),
           (_pop_struct(65, n, ed, md), "pop->n_policies out of range [1, SCG_POP_MAX]"),
           (_pop_struct(0, 0, ed, md), "pop->n_policies out of range [1, SCG_POP_MAX]"),       # ... before n_per
           (_pop_struct(n_pol, 0, ed, md), "pop->n_per must be >= 1"),                          # ... before the product
           (_pop_struct(n_pol, -5, ed, md), "pop->n_per must be >= 1"),
           (_pop_struct(n_pol, n_per + 1, ed, md), "pop->n_policies * pop->n_per is not the context's n_envs"),
           (_pop_struct(n_pol - 1, n_per, ed, md), "pop->n_policies * pop->n_per is not the context's n_envs"),
           (_pop_struct(64, 2 ** 31 - 1, ed, md), "pop->n_policies * pop->n_per is not the context's n_envs")]     # (64 bits)
    for pop, why in bad:
        rc, msg = call(pop)
        assert rc == -1 and msg == name + why, msg
        # scg_rollout_branch's refusals come first, under this entry point's name
        for kw, theirs in ((dict(n_steps=0), "first_action with n_steps == 0: no real step to force"), (dict(flags=0x80), "unknown flag"),
                           (dict(flags=B | AT), "SCG_ROLLOUT_BEGIN and SCG_ROLLOUT_BEGIN_AT together"), (dict(rules=4), "unknown rule"),
                           (dict(n_steps=2), "rec->rows too small for the launch's pseudo-steps")):
            rc, msg = call(pop, **kw)
            assert rc == -1 and msg == name + theirs, msg
    rc, msg = call(_pop_struct(n_pol, n_per, ed, md), c=None)
    assert rc == -1 and msg == name + "null ctx"
    W4 = dev(W)
    for Wbad, popbad in ((W4.view(-1), (ed, md)), (W4[:2].contiguous(), (ed, md)), (W4, (ed[:2].contiguous(), md)), (W4, (ed, md.to(torch.int64))),
                         (W4, (ed.cpu(), md)), (W4, ed)):
        with pytest.raises(ScgError):                              # the wrapper refuses a misshapen population before the call
            ctx.rollout(run.st, Wbad, clf, MASK_ARG, 0, 1, begin=True, population=popbad)
    torch.cuda.synchronize()
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(run.st, f)), as_bytes(getattr(before, f))), f"a refused call wrote {f}"
    for f in STATS:
        assert int((getattr(run.stats, f) != 77).sum()) == 0, f"a refused call wrote stats.{f}"
    assert int((run.interrupts != 77).sum()) == 0 and int((run.overrides != 77).sum()) == 0 and int(run.rec.len.abs().sum()) == 0
    a = run.audit
    assert all(int((getattr(a, f) != G8).sum()) == 0 for f in ("applied", "cand"))
    assert all(int((getattr(a, f) != GUARD).sum()) == 0 for f in ("v_root", "v_cand", "disc_final"))
    assert (first == 3).all() and np.array_equal(as_bytes(Wd), as_bytes(W.reshape(-1))) and np.array_equal(ed.cpu().numpy(), eps)
    run.stats.zero_()
    for pop in (_pop_struct(n_pol, n_per, None, md), _pop_struct(n_pol, n_per, ed, None), _pop_struct(n_pol, n_per, ed, md)):
        rc, _ = call(pop)                                          # null members are allowed; well-formed: it runs, the step takes the action
        torch.cuda.synchronize()
        assert rc == 0 and (run.rec.len == 2).all() and (run.rec.action[1] == 3).all() and (run.st.action == 3).all()
    # the wrapper's population launch is the entry point's
    twin = Run(ctx, st_np, rows=2)
    ctx.rollout(twin.st, W4, clf, MASK_ARG, 0, 1, stats=twin.stats, begin=True, first_action=first, population=(ed, md))
    ref = Run(ctx, st_np, rows=2)
    ref.population(Wd, clf, MASK_ARG, 0, 1, B, 0, _pop_struct(n_pol, n_per, ed, md), first)
    torch.cuda.synchronize()
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(twin.st, f)), as_bytes(getattr(ref.st, f))), f


# ---------------------------------------------------------------------------------------------------- 6. the agent

COUNTERS = ("t", "enabled_mask", "gest_mask")


def _agent():
    """tests/test_gpu_branch_fit.py's agent: options 1 and 2 on the wide chain, 24-step episodes, no completion bonus."""
    a = crossing_agent(n=256, n_opt=2)
    a.ctx.set_hparams(max_episode_steps=24, reoffer_period=1, r_option_success=0.0)
    return a


def _before(a):
    return dict(W=a.W.clone(), state=clone_state(a.state), counters={f: getattr(a, f) for f in COUNTERS})


def _assert_left_alone(a, before, calls, msg):
    torch.cuda.synchronize()
    assert calls == [], f"{msg} called into the training context: {calls}"
    assert np.array_equal(as_bytes(a.W), as_bytes(before["W"])), f"{msg}: W"
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(a.state, f)), as_bytes(getattr(before["state"], f))), f"{msg}: state {f}"
    assert {f: getattr(a, f) for f in COUNTERS} == before["counters"], msg


def _three_tables(a):
    g = torch.Generator().manual_seed(11)
    return torch.stack([a.W.clone()] + [a.W + 0.05 * torch.randn(a.W.shape, generator=g).to(a.W.device) for _ in range(2)])


def _evaluate_as(a, W, mask, **kw):
    """evaluate(discounted=True) on the agent with W and the enabled mask set to one policy's, and both put back."""
    W0, m0 = a.W.clone(), a.enabled_mask
    a.W.copy_(W)
    a.enabled_mask = int(mask)
    try:
        return a.evaluate(discounted=True, per_env=True, **kw)
    finally:
        a.W.copy_(W0)
        a.enabled_mask = m0


def _assert_same_evaluation(got, got_env, want, want_env, msg):
    assert got == want, f"{msg}: {got} != {want}"
    assert list(got_env) == list(want_env)
    for f in want_env:
        assert np.array_equal(as_bytes(got_env[f]), as_bytes(want_env[f])), f"{msg}: per-env {f}"


def test_evaluate_policies_is_evaluate_per_policy():
    a = _agent()
    W, eps, enabled = _three_tables(a), [0.0, 0.1, 0.5], [0b110, 0b110, 0b010]
    before = _before(a)
    with spy_calls(a.ctx) as (calls, _):
        summaries, paired, envs = a.evaluate_policies(W, eps, enabled, n_episodes=256, seed=5, per_env=True)
        short = a.evaluate_policies(W, eps, enabled, n_episodes=256, seed=5)
    _assert_left_alone(a, before, calls, "evaluate_policies")
    assert short == (summaries, paired) and len(summaries) == len(paired) == len(envs) == 3
    for c in range(3):
        want, want_env = _evaluate_as(a, W[c], enabled[c], n_episodes=256, epsilon=eps[c], seed=5)
        _assert_same_evaluation(summaries[c], envs[c], want, want_env, f"policy {c}")
        assert want["episodes"] == 256 and "mean_discounted_return" in want
        assert paired[c] == paired_differences(envs[c], envs[0])
    assert all(r == {"mean_diff": 0.0, "se": 0.0, "n": 256} for r in paired[0].values())
    assert paired[1]["disc_final"]["se"] > 0.0 and summaries[0] != summaries[1] and sum(summaries[0]["entries"]) > 0
    assert summaries[2]["entries"][2] == 0 and summaries[0]["entries"][2] > 0          # option 2 is off for policy 2 alone
    # a list of tables, scalars for all policies, another baseline, the rules, given start states
    x, y = (t[:64].clone() for t in (a.state.x, a.state.y))
    kw = dict(seed=6, interrupt=True, choose="value", states=(x, y))
    s2, p2, e2 = a.evaluate_policies([W[1], W[2].reshape(-1)], 0.1, None, baseline=1, per_env=True, **kw)
    for c in range(2):
        want, want_env = _evaluate_as(a, W[1 + c], a.enabled_mask, epsilon=0.1, **kw)
        _assert_same_evaluation(s2[c], e2[c], want, want_env, f"states, policy {c}")
        assert want["episodes"] == 64 and "interrupts" in want and "overrides" in want
    assert p2[0] == paired_differences(e2[0], e2[1]) and p2[1]["ret"] == {"mean_diff": 0.0, "se": 0.0, "n": 64}


FIT = dict(n_states=64, n_held=32, replicates=2, n_episodes=128, epsilon=0.5, seed=5)
EVAL_EPS = (0.1, 0.0)       # the decision is taken at 0.1: at 0 every episode of this one-start map is the same one, and se = 0


def test_improve_policy():
    a = _agent()
    before = _before(a)
    with spy_calls(a.ctx) as (calls, _):
        report, W_kept = a.improve_policy(eval_epsilons=EVAL_EPS, z=1e30, n_eval=256, **FIT)
    _assert_left_alone(a, before, calls, "improve_policy(apply=False)")
    assert report["accepted"] is False and report["chosen_lambda"] == 0.0 and np.array_equal(as_bytes(W_kept), as_bytes(a.W))
    rows = report["candidates"]
    assert [(r["lambda"], r["epsilon"]) for r in rows] == [(lam, e) for e in EVAL_EPS for lam in (0.0, 0.25, 0.5, 1.0)]
    # the candidate table is evaluate_policies by hand on the damped tables of the fit's W_new
    fit_report, W_new = a.fit_values_to_branches(apply=False, **FIT)
    assert fit_report["vf"][0]["delta_norm"] == report["fit"]["vf"][0]["delta_norm"] > 0.0
    tables = torch.cat([a.W[None], damped_tables(a.W, W_new, (0.25, 0.5, 1.0))])
    assert np.array_equal(as_bytes(tables[3]), as_bytes(W_new)) and not np.array_equal(as_bytes(tables[1]), as_bytes(a.W))
    for i, e in enumerate(EVAL_EPS):
        summaries, paired = a.evaluate_policies(tables, e, None, n_episodes=256, seed=5)
        for j in range(4):
            assert rows[4 * i + j]["summary"] == summaries[j] and rows[4 * i + j]["paired"] == paired[j], f"epsilon {e} table {j}"
    assert all(r["paired"]["disc_final"]["se"] > 0.0 for r in rows[1:4])
    assert len({str(r["summary"]) for r in rows[:4]}) >= 2                            # the damped tables act differently
    # z = -inf: whatever candidate has the highest mean is applied (W itself where it is the best)
    means = [r["summary"]["mean_discounted_return"] for r in rows[:4]]
    best = max(range(4), key=lambda j: (means[j], -j))
    report2, W_chosen = a.improve_policy(eval_epsilons=EVAL_EPS, z=-float("inf"), n_eval=256, apply=True, **FIT)
    assert report2["chosen_lambda"] == (0.0, 0.25, 0.5, 1.0)[best] and report2["accepted"] == (best != 0)
    assert np.array_equal(as_bytes(W_chosen), as_bytes(tables[best])) and np.array_equal(as_bytes(a.W), as_bytes(W_chosen))
    with pytest.raises(ValueError):
        a.improve_policy(lambdas=(0.0, 0.5), n_eval=256, **FIT)
    with pytest.raises(ValueError):
        a.improve_policy(criterion="length", n_eval=256, **FIT)
