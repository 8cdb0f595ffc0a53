"""SPEC §24.1 on the GPU (scg_rollout_population_clf): a population rollout whose policies each read their own classifier table.
Every policy's env range equals by bits what scg_rollout_branch writes on a context of n_per envs with clf = pop_clf[c] — the
yardstick is always the existing entry point on the small context, never the new one. The rig (Run, the map, the launches, the
comparison) is tests/test_gpu_population.py's; the `clf` argument of every population call here is a fourth table that is no
policy's, as MASK_ARG is no policy's mask, so that a kernel that read it would show.

The tables: 0 sibling_tree's discs; 1 the same discs with radii x 0.6; 2 radii x 1.4 with row 2 all zeros (z = +0 everywhere: the
empty set, the `> 0` edge, on an option that policy has enabled)."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_population as P
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd.core import EnvState
from gpu_util import as_bytes, block_envs, clone_state, current_block_envs, dev  # noqa: F401  (block_envs: the fixture)
from util import crossing_weights, disc_weights, sibling_tree

pytestmark = pytest.mark.gpu

INT, BEST, B, ONE, AT = P.INT, P.BEST, P.B, P.ONE, P.AT
N_OPT, K, T0, MAX_EP = P.N_OPT, P.K, P.T0, P.MAX_EP
assert MAX_EP == 12 and K == 8                          # the issue's inputs: two launches of 8 steps end every 12-step episode
MASK_ARG = 0b101010                                     # the call's own enabled_mask: no policy's
ENABLED = (0b000110, 0b111110, 0b011110)                # policy 2 (table 2) has option 2, the all-zero row, enabled
EPS = P.EPS


def _discs(m):
    """sibling_tree's five discs (tests/util.py)."""
    tx, ty = float(m.target[0]), float(m.target[1])
    sx, sy = (1.0 if tx < 0.5 else -1.0), (1.0 if ty < 0.5 else -1.0)
    return [(tx, ty, 0.30), (tx + 0.10 * sx, ty + 0.10 * sy, 0.35), (0.5, 0.5, 0.45), (tx, 0.5, 0.50), (0.5, 0.5, 0.75)]


def _scaled(m, scale, zero_row=None):
    clf = np.zeros((N_OPT + 1, 8), np.float32)
    for k, (cx, cy, r) in enumerate(_discs(m), start=1):
        clf[k] = disc_weights(cx, cy, r * scale)
    if zero_row is not None:
        clf[zero_row] = 0.0
    return clf


def _tables(m):
    """(the three policies' tables [3][6][8], the fourth table that is no policy's) on the host."""
    t0 = sibling_tree(m)[1]
    assert np.array_equal(t0, _scaled(m, 1.0))          # the mirror of sibling_tree's discs is exact
    tabs = np.stack([t0, _scaled(m, 0.6), _scaled(m, 1.4, zero_row=2)])
    return tabs, _scaled(m, 0.25)


def _policies(n_pol, same=False):
    """(W, epsilon, enabled) on the host: crossing_weights plus seeded noise per policy; `same`: one W, epsilon and mask for all."""
    W0 = crossing_weights(N_OPT + 1, 6)
    W = np.stack([W0 if same or c == 0 else
                  W0 + (np.random.default_rng(100 + c).standard_normal(W0.shape) * 0.05).astype(np.float32) for c in range(n_pol)])
    eps = np.full(n_pol, 0.1, np.float32) if same else np.asarray(EPS[:n_pol], np.float32)
    enabled = np.full(n_pol, 0b111110, np.int32) if same else np.asarray(ENABLED[:n_pol], np.int32)
    return W.astype(np.float32), eps, enabled


class Run(P.Run):
    def population_clf(self, W, clf, mask, t0, n_steps, flags, rules, pop, pop_clf, first=None):
        keep, a = self.args(W, clf, mask, t0, n_steps, flags, rules, first)
        self.ctx._call("scg_rollout_population_clf", *a, None if pop is None else C.byref(pop),
                       None if pop_clf is None else C.c_void_p(pop_clf.data_ptr()))


def _inputs(n):
    m, parents, _, st_np = P._inputs(n)
    tabs, arg = _tables(m)
    return m, parents, tabs, dev(arg).view(-1), st_np


def _singles(m, parents, tabs, pol, st_np, n_per, rules, launches=P.LAUNCHES, window=None, force=None, first=None, block=None):
    """The yardstick: per policy c, scg_rollout_branch on a context of n_per envs under W[c], epsilon[c], enabled[c], clf = tabs[c]."""
    W, eps, enabled = pol
    out = []
    for c in range(len(eps)):
        lo, hi = c * n_per, (c + 1) * n_per
        ctx = P._context(m, parents, n_per, float(eps[c]), block)
        run = P.Run(ctx, P._slice_state(st_np, lo, hi), window=None if window is None else P._clip(window, lo, hi),
                    force=None if force is None else force[lo:hi])
        Wc, clf_c, fa = dev(W[c]).view(-1), dev(tabs[c]).view(-1), None if first is None else dev(first[lo:hi])
        snaps = []
        for t0, k, flags in launches:
            run.branch(Wc, clf_c, int(enabled[c]), t0, k, flags, rules, fa)
            snaps.append(run.outputs())
        out.append(snaps)
        ctx.close()
    return out


def _population(m, parents, tabs, clf_arg, pol, st_np, n_per, rules, launches=P.LAUNCHES, window=None, force=None, first=None,
                block=None):
    W, eps, enabled = pol
    n_pol = len(eps)
    ctx = P._context(m, parents, n_pol * n_per, 0.3, block)             # (the context's own epsilon is no policy's)
    run = Run(ctx, st_np, window=window, force=force)
    Wd, ed, md, td = dev(W).view(-1), dev(eps), dev(enabled), dev(np.ascontiguousarray(tabs[:n_pol]))
    pop = P._pop_struct(n_pol, n_per, ed, md)
    fa = None if first is None else dev(first)
    snaps = []
    for t0, k, flags in launches:
        run.population_clf(Wd, clf_arg, MASK_ARG, t0, k, flags, rules, pop, td, fa)
        snaps.append(run.outputs())
    assert np.array_equal(as_bytes(td), as_bytes(np.ascontiguousarray(tabs[:n_pol]))), "pop_clf was written"
    ctx.close()
    return snaps


def _conditions(singles, n_per, msg):
    """On the yardstick's side: some policy enters options, some episode ends at the goal, every episode ends."""
    last = [s[-1][0] for s in singles]
    entries = [int(o["stats.entries"].sum()) for o in last]
    goals = [int(o["stats.goals"].sum()) for o in last]
    print(f"{msg}: entries {entries}, goals {goals}, episodes {[int(o['stats.episodes'].sum()) for o in last]}, "
          f"finished {[int(o['stats.finished'].sum()) for o in last]}")
    assert max(entries) > 0 and max(goals) > 0, msg
    assert all(int(o["stats.finished"].sum()) == n_per for o in last), f"{msg}: an episode has not ended"


# ---------------------------------------------------------------------------------------------------- 1. the identity

@pytest.mark.parametrize("rules", P.ALL_RULES, ids=P.RULE_IDS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_policy_range_is_the_single_policy_rollout_under_its_table(shape, rules, monkeypatch):
    n_pol, n_per = shape
    n = n_pol * n_per
    m, parents, tabs, clf_arg, st_np = _inputs(n)
    pol = _policies(n_pol)
    monkeypatch.delenv("SCG_ROLLOUT_EPW", raising=False)
    singles = _singles(m, parents, tabs, pol, st_np, n_per, rules)
    _conditions(singles, n_per, f"{shape} rules {rules}")
    for epw in (None, 32):                                  # unset (2 envs per wave at these sizes) and one non-default value
        if epw is not None:
            monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
        P._compare(_population(m, parents, tabs, clf_arg, pol, st_np, n_per, rules), singles, n_per, (0, n),
                   f"{shape} rules {rules} epw {epw}")


@pytest.mark.parametrize("rules", [0, BEST | INT], ids=["plain", "best+interrupt"])
def test_only_the_tables_differ(rules):
    """Equal W, epsilon and enabled mask in every policy: whatever differs between the ranges comes from pop_clf alone."""
    n_pol, n_per = 3, 257
    n = n_pol * n_per
    m, parents, tabs, clf_arg, st_np = _inputs(n)
    one = P._slice_state(st_np, 0, n_per)
    st_np = {f: np.concatenate([v] * n_pol, axis=-1) for f, v in one.items()}              # one input state for every policy
    pol = _policies(n_pol, same=True)
    singles = _singles(m, parents, tabs, pol, st_np, n_per, rules)
    _conditions(singles, n_per, f"tables only, rules {rules}")
    # the end states of the FIRST launch: what the second leaves of an ended episode is its drawn restart state, which episodes that
    # end on the same step (the time limit) share whatever they did
    first, last = [s[0][0] for s in singles], [s[-1][0] for s in singles]
    per_option = [o["stats.entries"].sum(axis=1).tolist() for o in last]
    moved = {(a, b): int((first[a]["x"] != first[b]["x"]).sum()) for a, b in ((0, 1), (0, 2), (1, 2))}
    print(f"tables only, rules {rules}: per-option entries {per_option}, envs whose x differs after the first launch {moved}")
    assert any(moved[a, b] > 0 and per_option[a] != per_option[b] for a, b in moved), \
        "no two policies differ in their end states and their per-option entries: the tables do not matter on these inputs"
    assert per_option[2][2] == 0                                                           # the all-zero row is the empty set
    P._compare(_population(m, parents, tabs, clf_arg, pol, st_np, n_per, rules), singles, n_per, (0, n), f"tables only, rules {rules}")


# ---------------------------------------------------------------------------------------------------- 2. further identity cases

def test_begin_at_with_a_force_and_a_first_action():
    n_pol, n_per = 3, 40
    n = n_pol * n_per
    m, parents, tabs, clf_arg, st_np = _inputs(n)
    pol = _policies(n_pol)
    e = np.arange(n)
    force = ((e * 5 + e // n_per) % 5 - 2).astype(np.int8)                  # -2 .. +2, another pattern in every policy's range
    first = ((e * 7 + 3 * (e // n_per)) % 6).astype(np.uint8)              # 5: not forced
    assert not np.array_equal(force[:n_per], force[n_per:2 * n_per]) and not np.array_equal(first[:n_per], first[n_per:2 * n_per])
    kw = dict(launches=((T0, 2 * K, AT),), force=force, first=first)       # (a force needs a begin flag: one launch)
    singles = _singles(m, parents, tabs, pol, st_np, n_per, BEST | INT, **kw)
    applied = [s[0][0]["audit.applied"][0] for s in singles]
    print(f"begin_at: force applied {[int((a == 1).sum()) for a in applied]} of {n_per} per policy, "
          f"entries {[int(s[0][0]['stats.entries'].sum()) for s in singles]}")
    assert (np.concatenate(applied) == 1).any() and (np.concatenate(applied) == 0).any()
    P._compare(_population(m, parents, tabs, clf_arg, pol, st_np, n_per, BEST | INT, **kw), singles, n_per, (0, n), "begin_at")


def test_a_record_window_across_a_policy_boundary():
    n_pol, n_per, window = 3, 40, (30, 35)                                 # policy 0's envs 30 .. 39, policy 1's 40 .. 64, none of 2's
    m, parents, tabs, clf_arg, st_np = _inputs(n_pol * n_per)
    pol = _policies(n_pol)
    singles = _singles(m, parents, tabs, pol, st_np, n_per, 0, window=window)
    assert [bool(s[0][1]) for s in singles] == [True, True, False]
    terms = np.concatenate([s[j][1]["term"].reshape(-1) for s in singles[:2] for j in range(2)])
    ids = np.concatenate([s[j][1]["option_id"].reshape(-1) for s in singles[:2] for j in range(2)])
    print(f"window: term codes {np.bincount(terms, minlength=6).tolist()}, option ids {sorted(set(ids.tolist()))}")
    assert (terms != 0).any() and (ids > 0).any()                          # the fields that read the classifier hold something
    pop = _population(m, parents, tabs, clf_arg, pol, st_np, n_per, 0, window=window)
    P._compare(pop, singles, n_per, window, "window")
    for j in range(2):                                                     # (P._compare covers every record field; these two by name)
        for f in ("term", "option_id"):
            got = pop[j][1][f]
            assert np.array_equal(got[:, :10], singles[0][j][1][f]) and np.array_equal(got[:, 10:], singles[1][j][1][f]), f


@pytest.mark.parametrize("block_envs", [64, 128, 256], indirect=True)
def test_every_block_build(block_envs):
    n_pol, n_per = 3, 40
    m, parents, tabs, clf_arg, st_np = _inputs(n_pol * n_per)
    pol = _policies(n_pol)
    singles = _singles(m, parents, tabs, pol, st_np, n_per, INT, block=current_block_envs())
    pop = _population(m, parents, tabs, clf_arg, pol, st_np, n_per, INT, block=current_block_envs())
    P._compare(pop, singles, n_per, (0, n_pol * n_per), f"block {block_envs}")


# ---------------------------------------------------------------------------------------------------- 3. equivalences

@pytest.mark.parametrize("rules", P.ALL_RULES, ids=P.RULE_IDS)
def test_null_table_and_identical_tables_are_the_population_rollout(rules):
    n_pol, n_per = 3, 40
    n = n_pol * n_per
    m, parents, tabs, _, st_np = _inputs(n)
    W, eps, enabled = _policies(n_pol)
    clf = dev(tabs[0]).view(-1)
    Wd, ed, md = dev(W).view(-1), dev(eps), dev(enabled)
    same = dev(np.ascontiguousarray(np.stack([tabs[0]] * n_pol)))
    first = dev(((np.arange(n) * 3) % 7).astype(np.uint8))
    ctx = P._context(m, parents, n, 0.3)
    pop = P._pop_struct(n_pol, n_per, ed, md)
    ref, null, ident = Run(ctx, st_np), Run(ctx, st_np), Run(ctx, st_np)
    for t0, k, flags in P.LAUNCHES:
        ref.population(Wd, clf, MASK_ARG, t0, k, flags, rules, pop, first)
        want = ref.outputs()
        null.population_clf(Wd, clf, MASK_ARG, t0, k, flags, rules, pop, None, first)
        P._assert_slice(null.outputs(), want, 0, n, (0, n), f"rules {rules} pop_clf = NULL")
        ident.population_clf(Wd, clf, MASK_ARG, t0, k, flags, rules, pop, same, first)
        P._assert_slice(ident.outputs(), want, 0, n, (0, n), f"rules {rules} C tables equal to clf")
    assert int(ref.stats.entries.sum()) > 0 and int(ref.stats.goals.sum()) > 0
    # pop = NULL and pop_clf = NULL: scg_rollout_branch
    ref2, both = Run(ctx, st_np), Run(ctx, st_np)
    ref2.branch(Wd, clf, 0b110, T0, K, B | ONE, rules, first)
    both.population_clf(Wd, clf, 0b110, T0, K, B | ONE, rules, None, None, first)
    P._assert_slice(both.outputs(), ref2.outputs(), 0, n, (0, n), f"rules {rules} pop = pop_clf = NULL")
    ctx.close()


# ---------------------------------------------------------------------------------------------------- 4. refusals

def test_pop_clf_without_pop_is_the_last_refusal(monkeypatch):
    n_pol, n_per = 3, 40
    n = n_pol * n_per
    m, parents, tabs, clf_arg, st_np = _inputs(n)
    W, eps, enabled = _policies(n_pol)
    Wd, ed, md, td = dev(W).view(-1), dev(eps), dev(enabled), dev(tabs)
    monkeypatch.delenv("SCG_ROLLOUT_EPW", raising=False)
    ctx = P._context(m, parents, n, 0.3)
    run = Run(ctx, st_np, rows=2)
    before = clone_state(run.st)
    for f in P.STATS:
        getattr(run.stats, f).fill_(77)
    run.interrupts.fill_(77)
    run.overrides.fill_(77)
    first = torch.full((n,), 3, dtype=torch.uint8, device=ctx.device)
    lib = ctx.lib

    def call(pop, pop_clf, flags=B, n_steps=1, rules=0, c=ctx._ctx):
        keep, a = run.args(Wd, clf_arg, MASK_ARG, 0, n_steps, flags, rules, first)
        rc = lib.scg_rollout_population_clf(c, *a, None if pop is None else C.byref(pop),
                                            None if pop_clf is None else C.c_void_p(pop_clf.data_ptr()))
        return rc, lib.scg_last_error(c).decode()

    name = "scg_rollout_population_clf: "
    rc, msg = call(None, td)
    assert rc == -1 and msg == name + "pop_clf without pop", msg
    # every earlier refusal wins over it, in the sequence of scg_rollout_population
    for kw, theirs in ((dict(rules=4), "unknown rule"), (dict(flags=B | AT), "SCG_ROLLOUT_BEGIN and SCG_ROLLOUT_BEGIN_AT together"),
                       (dict(flags=0x80), "unknown flag"), (dict(n_steps=-1), "n_steps out of range [0, SCG_ROLLOUT_MAX_STEPS]"),
                       (dict(n_steps=2), "rec->rows too small for the launch's pseudo-steps"),
                       (dict(n_steps=0), "first_action with n_steps == 0: no real step to force")):
        rc, msg = call(None, td, **kw)
        assert rc == -1 and msg == name + theirs, msg
    rc, msg = call(None, td, c=None)
    assert rc == -1 and msg == name + "null ctx"
    monkeypatch.setenv("SCG_ROLLOUT_EPW", "3")                              # the launch geometry's refusal is an earlier one too
    rc, msg = call(None, td)
    assert rc == -1 and msg == name + "SCG_ROLLOUT_EPW must be 2, 4, 8, 16 or 32", msg
    monkeypatch.delenv("SCG_ROLLOUT_EPW")
    # with a pop, scg_rollout_population's own three refusals are unchanged, under this entry point's name
    for pop, why in ((P._pop_struct(0, n, ed, md), "pop->n_policies out of range [1, SCG_POP_MAX]"),
                     (P._pop_struct(n_pol, 0, ed, md), "pop->n_per must be >= 1"),
                     (P._pop_struct(n_pol, n_per + 1, ed, md), "pop->n_policies * pop->n_per is not the context's n_envs")):
        rc, msg = call(pop, td)
        assert rc == -1 and msg == name + why, msg
    # the wrapper refuses a misshapen table before the call
    W4 = dev(W)
    for bad in (td[:2].contiguous(), td.view(-1), td[:, :5].contiguous(), td.double(), td.cpu(), tabs):
        with pytest.raises(_lib.ScgError):
            ctx.rollout(run.st, W4, clf_arg, MASK_ARG, 0, 1, begin=True, population=(ed, md, bad))
    with pytest.raises(_lib.ScgError):
        ctx.rollout(run.st, W4, clf_arg, MASK_ARG, 0, 1, begin=True, population=(ed, md, td, None))
    torch.cuda.synchronize()
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(run.st, f)), as_bytes(getattr(before, f))), f"a refused call wrote {f}"
    for f in P.STATS:
        assert int((getattr(run.stats, f) != 77).sum()) == 0, f"a refused call wrote stats.{f}"
    assert int((run.interrupts != 77).sum()) == 0 and int((run.overrides != 77).sum()) == 0 and int(run.rec.len.abs().sum()) == 0
    a = run.audit
    assert all(int((getattr(a, f) != P.G8).sum()) == 0 for f in ("applied", "cand"))
    assert all(int((getattr(a, f) != P.GUARD).sum()) == 0 for f in ("v_root", "v_cand", "disc_final"))
    assert (first == 3).all() and np.array_equal(as_bytes(td), as_bytes(tabs)) and np.array_equal(as_bytes(Wd), as_bytes(W.reshape(-1)))
    # well-formed: it runs; and the wrapper's three-element population is the entry point's launch
    run.stats.zero_()
    rc, _ = call(P._pop_struct(n_pol, n_per, ed, md), td)
    torch.cuda.synchronize()
    assert rc == 0 and (run.rec.len == 2).all() and (run.st.action == 3).all() and np.array_equal(as_bytes(td), as_bytes(tabs))
    twin, ref = Run(ctx, st_np, rows=2), Run(ctx, st_np, rows=2)
    ctx.rollout(twin.st, W4, clf_arg, MASK_ARG, 0, 1, stats=twin.stats, begin=True, first_action=first, population=(ed, md, td))
    ref.population_clf(Wd, clf_arg, MASK_ARG, 0, 1, B, 0, P._pop_struct(n_pol, n_per, ed, md), td, first)
    none = Run(ctx, st_np, rows=2)
    ctx.rollout(none.st, W4, clf_arg, MASK_ARG, 0, 1, stats=none.stats, begin=True, first_action=first, population=(ed, md, None))
    ref0 = Run(ctx, st_np, rows=2)
    ref0.population(Wd, clf_arg, MASK_ARG, 0, 1, B, 0, P._pop_struct(n_pol, n_per, ed, md), first)
    torch.cuda.synchronize()
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(twin.st, f)), as_bytes(getattr(ref.st, f))), f
        assert np.array_equal(as_bytes(getattr(none.st, f)), as_bytes(getattr(ref0.st, f))), f
    ctx.close()
