"""SPEC §19 branch rollouts on the GPU (scg_rollout_branch): without a force it is scg_rollout_audit; forcing the action the
unforced launch took changes nothing; a real force equals a construction on the already-verified entry point (one step at ε = 0
from a spiked qcache, then the rest); the forced step is scg_pinball_step's physics; a branch on the recorded random stream from
Trajectory.resume_state's state reproduces the record; skipped envs and out-of-range entries; launch geometry and block build;
the refusals; and the agent's branch_audit() end to end. The inputs are tests/audit_model.py's cases, with the four `rules`."""
import ctypes as C

import numpy as np
import pytest
import torch

import audit_model as am
from audit_model import GUARD, MASK, N_OPT
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd._lib import ScgError
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.evaluation import EpisodeStats, GateAudit
from skill_chaining_with_graphs_amd.trajectory import Trajectory
from gpu_util import (as_bytes, block_envs, clone_state, crossing_agent, current_block_envs, dev, make_context,  # noqa: F401
                      spy_calls, state_to_device)                                                            # (block_envs: the fixture)
from util import random_states

pytestmark = pytest.mark.gpu

STATS = EpisodeStats.FIELDS
INT, BEST = _lib.SELECT_INTERRUPT, _lib.SELECT_BEST
B, ONE, AT = _lib.ROLLOUT_BEGIN, _lib.ROLLOUT_ONE_EPISODE, _lib.ROLLOUT_BEGIN_AT
ALL_RULES = [0, INT, BEST, BEST | INT]
RULE_IDS = ["plain", "interrupt", "best", "best+interrupt"]
AUDIT = tuple(GateAudit.DTYPES)[1:]                    # the audit's outputs (every member but force)
G8 = 77                                                # the guard of the two byte arrays
NONE = _lib.NO_FIRST_ACTION
K, T0 = 12, 40
LONG = dict(max_episode_steps=60)                      # no episode times out inside a launch (the cases' own limit is 7)


def _setup(name, n, block=None, **hp):
    m, parents, clf, W0, st_np, _ = am.case(name, n)
    ctx = make_context(m, n, N_OPT, block, parents, 0, am.SEED, reoffer_period=am.REOFFER, **dict(am.CASE_HP, **hp))
    return ctx, m, dev(W0).view(-1), dev(clf).view(-1), st_np


class Out:
    """Everything one launch can write besides the env state: stats, the record, the two rule counters and the audit's arrays,
    the latter prefilled with guards."""

    def __init__(self, ctx, rows=K + 1):
        n = ctx.n_envs
        self.stats = EpisodeStats(ctx.n_vf, n, ctx.device)
        self.rec = Trajectory(n, rows, 0, ctx.device, n_vf=ctx.n_vf)
        self.interrupts = torch.zeros((ctx.n_vf, n), dtype=torch.int32, device=ctx.device)
        self.overrides = torch.zeros((ctx.n_vf, n), dtype=torch.int32, device=ctx.device)
        self.audit = GateAudit(n, ctx.device)
        self.audit.applied.fill_(G8)
        self.audit.cand.fill_(G8)
        for f in ("v_root", "v_cand", "disc_final"):
            getattr(self.audit, f).fill_(float(GUARD))

    def record(self):
        return {f: getattr(self.rec, f).cpu().numpy() for f in self.rec.fields}, self.rec.len.cpu().numpy()

    def arrays(self):
        return {f: getattr(self.audit, f).cpu().numpy() for f in AUDIT}


def _args(ctx, st, W, clf, t0, n_steps, flags, rules, out, audit=True, rec=True, mask=MASK):
    cs = out.stats.c_struct()
    rc = out.rec.c_struct()
    au = out.audit.c_struct()
    keep = (cs, rc, au)
    return keep, [C.c_void_p(getattr(st, f).data_ptr()) for f in EnvState.FIELDS] + [
        C.c_void_p(W.data_ptr()), C.c_void_p(clf.data_ptr()), C.c_uint32(mask), C.c_uint64(t0), C.c_int32(n_steps), C.c_uint32(flags),
        C.byref(cs), C.c_void_p(out.interrupts.data_ptr()), C.c_void_p(out.overrides.data_ptr()), C.byref(rc) if rec else None,
        C.c_uint32(rules), C.byref(au) if audit else None]


def _audit(ctx, st, W, clf, t0, n_steps, flags, rules, out, **kw):
    """The existing entry point: scg_rollout_audit."""
    keep, a = _args(ctx, st, W, clf, t0, n_steps, flags, rules, out, **kw)
    ctx._call("scg_rollout_audit", *a, ctx._stream())


def _branch(ctx, st, W, clf, t0, n_steps, flags, rules, out, first, **kw):
    """scg_rollout_branch; `first`: a uint8 device tensor, or None for NULL."""
    keep, a = _args(ctx, st, W, clf, t0, n_steps, flags, rules, out, **kw)
    ctx._call("scg_rollout_branch", *a, None if first is None else C.c_void_p(first.data_ptr()), ctx._stream())


def _same_launch(st_a, a, st_b, b, msg, record=True, audit=AUDIT, rows=None):
    torch.cuda.synchronize()
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(st_a, f)), as_bytes(getattr(st_b, f))), f"{msg}: state field {f} differs"
    for f in STATS:
        assert np.array_equal(as_bytes(getattr(a.stats, f)), as_bytes(getattr(b.stats, f))), f"{msg}: stats.{f}"
    for f in ("interrupts", "overrides"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f"{msg}: {f}"
    if record:
        (ra, la), (rb, lb) = a.record(), (b.record() if rows is None else rows)
        assert np.array_equal(la, lb), f"{msg}: len"
        R = min(ra["x"].shape[0], rb["x"].shape[0])
        assert la.max() <= R
        valid = np.arange(R)[:, None] < la[None, :]
        for f in ra:
            assert np.array_equal(as_bytes(ra[f][:R][valid]), as_bytes(rb[f][:R][valid])), f"{msg}: record field {f}"
    x, y = a.arrays(), b.arrays()
    for f in audit:
        assert np.array_equal(as_bytes(x[f]), as_bytes(y[f])), f"{msg}: audit.{f}"


def _natural(ctx, st_np, W, clf, flags, rules):
    """The unforced launch of K steps from the case's state: (its end state, its Out, the action of its first real step)."""
    st, out = state_to_device(st_np, ctx), Out(ctx)
    _audit(ctx, st, W, clf, T0, K, flags, rules, out)
    torch.cuda.synchronize()
    return st, out, out.rec.action[1 if flags & (B | AT) else 0].clone()


def _other_action(natural):
    """An action that differs from the natural one for every env: (natural + 1 + e % 4) % 5."""
    e = torch.arange(natural.numel(), device=natural.device)
    return ((natural.to(torch.int64) + 1 + e % 4) % 5).to(torch.uint8).contiguous()


# ---------------------------------------------------------------------------------------------------- 1. no force

@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
def test_no_force_is_the_audited_rollout(rules):
    n = 130
    ctx, m, W, clf, st_np = _setup("pinball_simple", n)
    none = torch.full((n,), NONE, dtype=torch.uint8, device=ctx.device)
    for audit in (True, False):                                # with the audit's arrays, and with audit = NULL
        ref_st, ref = state_to_device(st_np, ctx), Out(ctx)
        runs = {"NULL": (clone_state(ref_st), Out(ctx), None), "all 255": (clone_state(ref_st), Out(ctx), none)}
        t = T0
        for flags in (AT, 0):                                  # a launch with BEGIN_AT, then one without a begin flag
            _audit(ctx, ref_st, W, clf, t, K, flags, rules, ref, audit=audit)
            for how, (st, out, first) in runs.items():
                _branch(ctx, st, W, clf, t, K, flags, rules, out, first, audit=audit)
                _same_launch(st, out, ref_st, ref, f"rules {rules} audit {audit} first_action {how} flags {flags}")
            t += K + 1
        a = ref.arrays()
        assert (a["applied"] != G8).all() == audit and (a["disc_final"] != GUARD).any() == audit
    assert int(ref.stats.entries.sum()) > 0 and int(ref.stats.episodes.sum()) > 0
    assert torch.equal(none, torch.full_like(none, NONE))


# ---------------------------------------------------------------------------------------------------- 2. the natural action

@pytest.mark.parametrize("flags", [0, AT], ids=["no begin", "begin_at"])
@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
def test_forcing_what_would_have_happened_changes_nothing(rules, flags):
    n = 67
    ctx, m, W, clf, st_np = _setup("pinball_empty", n, epsilon=0.3)
    ref_st, ref, natural = _natural(ctx, st_np, W, clf, flags, rules)
    assert len(torch.unique(natural)) >= 3 and int(natural.max()) < 5
    st, out = state_to_device(st_np, ctx), Out(ctx)
    _branch(ctx, st, W, clf, T0, K, flags, rules, out, natural.contiguous())
    _same_launch(st, out, ref_st, ref, f"rules {rules} flags {flags}")


# ---------------------------------------------------------------------------------------------------- 3. a real force

@pytest.mark.parametrize("flags", [0, AT], ids=["no begin", "begin_at"])
@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
def test_a_real_force_equals_the_construction_on_the_audited_rollout(rules, flags):
    """The yardstick never calls scg_rollout_branch: one step of scg_rollout_audit at ε = 0 from a qcache that holds 1.0 at the
    forced action and 0 elsewhere takes that action (§4.3's greedy choice; the draws are keyed by (seed, env, t), not by ε), then
    K - 1 steps at ε = 0.3 go on from t0 + 1. With BEGIN_AT the begin pseudo-step writes qcache = Q(s0, .) itself, so a spike
    given to a launch of BEGIN_AT plus one step would be overwritten before the step reads it: the begin pseudo-step is a launch
    of its own (BEGIN_AT, 0 steps), the spike goes in behind it, and the forced step is the one-step launch at t0 + 1."""
    n = 257
    ctx, m, W, clf, st_np = _setup("pinball_simple", n, epsilon=0.3, **LONG)
    nat_st, nat, natural = _natural(ctx, st_np, W, clf, flags, rules)
    first = _other_action(natural)
    assert int((first == natural).sum()) == 0 and int(first.max()) < 5
    # ---- the yardstick: launches of scg_rollout_audit only
    y_st, ys = state_to_device(st_np, ctx), [Out(ctx), Out(ctx), Out(ctx)]
    for o in ys[1:]:                                           # one set of counters and audit arrays across the launches
        o.stats, o.interrupts, o.overrides, o.audit = ys[0].stats, ys[0].interrupts, ys[0].overrides, ys[0].audit
    t = T0
    if flags:
        _audit(ctx, y_st, W, clf, t, 0, AT, rules, ys[0])
        t += 1
    spike = torch.zeros((5, n), dtype=torch.float32, device=ctx.device)
    spike[first.to(torch.int64), torch.arange(n, device=ctx.device)] = 1.0
    y_st.qcache.copy_(spike)
    ctx.set_hparams(epsilon=0.0)
    _audit(ctx, y_st, W, clf, t, 1, 0, rules, ys[1])
    ctx.set_hparams(epsilon=0.3)
    _audit(ctx, y_st, W, clf, t + 1, K - 1, 0, rules, ys[2])
    torch.cuda.synchronize()
    parts = [o.record() for o in (ys if flags else ys[1:])]
    take = ([1] if flags else []) + [1, K - 1]                 # rows each launch wrote (no ONE_EPISODE: every pseudo-step)
    assert all((ln == k).all() for (_, ln), k in zip(parts, take))
    rows = {f: np.concatenate([r[f][:k] for (r, _), k in zip(parts, take)]) for f in parts[0][0]}
    assert np.array_equal(rows["action"][1 if flags else 0], first.cpu().numpy())
    # ---- the branch launch
    st, out = state_to_device(st_np, ctx), Out(ctx)
    _branch(ctx, st, W, clf, T0, K, flags, rules, out, first)
    _same_launch(st, out, y_st, ys[0], f"rules {rules} flags {flags}", rows=(rows, np.full(n, sum(take), np.int32)))
    # ---- non-vacuity, on the yardstick's side: the forced run is another run
    moved = (y_st.x != nat_st.x) | (y_st.y != nat_st.y)
    print(f"rules {rules} flags {flags}: {int(moved.sum())} of {n} envs end elsewhere; episodes ended {int(ys[0].stats.episodes.sum())}")
    assert int(moved.sum()) * 2 >= n


# ---------------------------------------------------------------------------------------------------- 4. the physics

def test_the_forced_step_is_the_physics_of_that_action():
    n = 130
    ctx, m, W, clf, st_np = _setup("pinball_simple", n, **LONG)
    x, y, vx, vy = random_states(m, n, 11, vmax=1.5)
    st_np = dict(st_np, x=x, y=y, vx=vx, vy=vy, ep_steps=np.zeros(n, np.int32))
    for a in range(5):
        first = torch.full((n,), a, dtype=torch.uint8, device=ctx.device)
        s = [dev(v.copy()) for v in (x, y, vx, vy)]
        rew, goal = ctx.pinball_step(s, first)
        st, out = state_to_device(st_np, ctx), Out(ctx)
        _branch(ctx, st, W, clf, T0, 1, 0, BEST | INT, out, first)
        torch.cuda.synchronize()
        row, ln = out.record()
        assert (ln == 1).all() and (row["action"][0] == a).all() and (st.action.cpu().numpy() == a).all()
        for f, want in zip(("x", "y", "vx", "vy", "reward"), s + [rew]):       # the record holds s' before a goal's reset
            assert np.array_equal(as_bytes(row[f][0]), as_bytes(want)), f"action {a}: {f}"
        assert np.array_equal(as_bytes(st.reward), as_bytes(rew)) and np.array_equal(row["done"][0] == 1, goal.cpu().numpy() != 0)


# ---------------------------------------------------------------------------------------------------- 5. the record

ROWS = 20


def _resume_on(ctx, W, src, alive):
    """A device EnvState of ctx.n_envs envs holding resume_state's `src` at the envs `alive` (the others: a blank state, to be
    skipped), qcache = Q_vf_next(s, .) by scg_q_values."""
    st = EnvState(ctx.n_envs, ctx.device, ctx.map)
    at = dev(alive)
    for f in ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps"):
        getattr(st, f)[at] = dev(src[f])
    s = [dev(src[f]) for f in ("x", "y", "vx", "vy")]
    Wk = W.view(ctx.n_vf, -1)
    for k in np.unique(src["vf_next"]):
        sel = dev(np.nonzero(src["vf_next"] == k)[0])
        st.qcache[:, at[sel]] = ctx.q_values([t[sel].contiguous() for t in s], Wk[int(k)].contiguous())
    return st


@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
def test_a_branch_on_the_recorded_stream_is_the_record(rules):
    n = 130
    ctx, m, W, clf, st_np = _setup("pinball_simple", n, epsilon=0.3, max_episode_steps=16, max_option_steps=4)
    st, rec = state_to_device(st_np, ctx), Out(ctx, ROWS + 1)
    _audit(ctx, st, W, clf, 0, ROWS, B | ONE, rules, rec)
    torch.cuda.synchronize()
    traj = rec.rec.append()
    rows, ln = rec.record()
    # a row right after an option entry: the row (3 .. 12) before which the most envs entered an option (under the root, or on
    # the row that ended another execution)
    entered = (((rows["vf"][2:12] == 0) | (rows["term"][2:12] != 0)) & (rows["option_id"][2:12] >= 1)
               & (np.arange(2, 12)[:, None] + 1 < ln[None, :]))
    j_entry = 3 + int(np.argmax(entered.sum(axis=1)))
    print(f"rules {rules}: lens {np.bincount(ln)}; entries before row {j_entry}: {int(entered.sum(axis=1).max())}")
    assert entered.sum(axis=1).max() >= 3 and ln.min() < ROWS + 1 and (rows["option_id"][:ROWS // 2] < 0).any()
    for j in (1, 2, 7, j_entry):
        alive = np.nonzero(ln > j)[0]
        assert len(alive) >= n // 4
        src = traj.resume_state(alive, np.full(len(alive), j))
        if j == j_entry:
            assert int(((src["opt_steps"] == 0) & (src["vf_next"] >= 1)).sum()) >= 3
        if j == 7:
            assert src["opt_steps"].max() >= 2 and (src["option_id"] < 0).any()
        first = np.full(n, NONE, np.uint8)
        first[alive] = rows["action"][j][alive]
        for forced in (True, False):
            b_st, out = _resume_on(ctx, W, src, alive), Out(ctx, ROWS + 1)
            out.stats.finished.fill_(1)
            out.stats.finished[dev(alive)] = 0
            _branch(ctx, b_st, W, clf, j, ROWS - j + 1, ONE, rules, out, dev(first) if forced else None)
            torch.cuda.synchronize()
            got, got_len = out.record()
            assert np.array_equal(got_len, np.where(ln > j, ln - j, 0)), f"row {j}: len"
            valid = np.arange(ROWS + 1 - j)[:, None] < got_len[None, :]
            for f in got:
                assert np.array_equal(as_bytes(got[f][:ROWS + 1 - j][valid]), as_bytes(rows[f][j:][valid])), \
                    f"rules {rules} row {j} forced {forced}: record field {f}"


# ---------------------------------------------------------------------------------------------------- 6. skipped, out of range

def test_skipped_envs_and_out_of_range_entries():
    n, pad = 130, 64
    ctx, m, W, clf, st_np = _setup("pinball_simple", n, epsilon=0.3, **LONG)
    skipped = np.random.default_rng(5).random(n) < 0.5
    buf = torch.full((n + 2 * pad,), 0xAB, dtype=torch.uint8, device=ctx.device)
    first = buf[pad:pad + n]
    entries = np.where(skipped, 2, np.array([5, 6, 254, 255], np.uint8)[np.arange(n) % 4]).astype(np.uint8)      # a real action for the skipped
    first.copy_(dev(entries))
    want = buf.clone()
    ref_st, ref, st, out = state_to_device(st_np, ctx), Out(ctx), state_to_device(st_np, ctx), Out(ctx)
    for o in (ref, out):
        o.stats.finished.copy_(dev(skipped.astype(np.uint8)))
        o.audit.disc_ret.fill_(float(GUARD)); o.audit.disc_g.fill_(float(GUARD))
        for f in ("disc_ret", "disc_g"):                       # (in/out for the stepped envs)
            getattr(o.audit, f)[dev(np.nonzero(~skipped)[0])] = 1.0
    before = clone_state(st)
    _audit(ctx, ref_st, W, clf, T0, K, ONE, BEST | INT, ref)
    _branch(ctx, st, W, clf, T0, K, ONE, BEST | INT, out, first)
    _same_launch(st, out, ref_st, ref, "entries 5, 6, 254, 255 are not forced")
    assert torch.equal(buf, want), "first_action or its guard bands were written"
    a = out.arrays()
    assert 30 < skipped.sum() < n - 30
    assert all((a[f][skipped] == GUARD).all() for f in ("disc_ret", "disc_g", "disc_final")) and (a["disc_ret"][~skipped] != GUARD).all()
    for f in EnvState.FIELDS:
        x, y = getattr(st, f).cpu().numpy(), getattr(before, f).cpu().numpy()
        assert np.array_equal(as_bytes(x[..., skipped]), as_bytes(y[..., skipped])), f"a skipped env's {f} was written"
    assert (out.rec.len.cpu().numpy()[skipped] == 0).all() and (out.rec.len.cpu().numpy()[~skipped] >= 1).all()
    # the same entries with the skipped envs stepped: their force is then a real one
    st2, out2 = state_to_device(st_np, ctx), Out(ctx)
    _branch(ctx, st2, W, clf, T0, K, 0, BEST | INT, out2, first)
    torch.cuda.synchronize()
    assert (out2.rec.action[0].cpu().numpy()[skipped] == 2).all()


# ---------------------------------------------------------------------------------------------------- 7. independence

def _forced_launches(n, rules, block=None):
    """BEGIN_AT with a real force, then a launch without a begin flag with another: (state, Out)."""
    ctx, m, W, clf, st_np = _setup("pinball_simple", n, block=block, epsilon=0.3)
    st, out = state_to_device(st_np, ctx), Out(ctx)
    first = dev((np.arange(n) % 7).astype(np.uint8))           # 5 and 6: not forced
    _branch(ctx, st, W, clf, T0, K, AT, rules, out, first)
    _branch(ctx, st, W, clf, T0 + K + 1, K, 0, rules, out, dev(((np.arange(n) + 3) % 5).astype(np.uint8)), rec=False)
    torch.cuda.synchronize()
    return st, out


def test_every_launch_geometry(monkeypatch):
    ref_st, ref = _forced_launches(257, BEST | INT)
    assert int(ref.stats.episodes.sum()) > 0 and int(ref.interrupts.sum()) > 0
    assert np.array_equal(ref.rec.action[1].cpu().numpy()[np.arange(257) % 7 < 5], (np.arange(257) % 7)[np.arange(257) % 7 < 5])
    for epw in (2, 32):
        monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
        st, out = _forced_launches(257, BEST | INT)
        _same_launch(st, out, ref_st, ref, f"epw {epw}")


@pytest.mark.parametrize("block_envs", [64, 128, 256], indirect=True)
def test_every_block_build(block_envs):
    ref_st, ref = _forced_launches(257, INT)
    st, out = _forced_launches(257, INT, block=current_block_envs())
    _same_launch(st, out, ref_st, ref, f"block {block_envs}")


# ---------------------------------------------------------------------------------------------------- 8. refusals

def test_refusals_launch_nothing():
    n = 67
    ctx, m, W, clf, st_np = _setup("pinball_simple", n)
    st = state_to_device(st_np, ctx)
    before = clone_state(st)
    out = Out(ctx, 2)
    for f in STATS:
        getattr(out.stats, f).fill_(77)
    out.interrupts.fill_(77)
    out.overrides.fill_(77)
    first = torch.full((n,), 3, dtype=torch.uint8, device=ctx.device)
    force = torch.ones(n, dtype=torch.int8, device=ctx.device)
    lib = ctx.lib

    def call(rules, flags, n_steps, fa=first, c=ctx._ctx, **au_kw):
        keep, a = _args(ctx, st, W, clf, 0, n_steps, flags, rules, out)
        for f, v in au_kw.items():
            setattr(keep[2], f, v)
        rc = lib.scg_rollout_branch(c, *a, None if fa is None else C.c_void_p(fa.data_ptr()), None)
        return rc, lib.scg_last_error(c).decode()

    for rules in ALL_RULES:
        for flags in (B, AT, B | ONE):                         # no real step to force
            rc, msg = call(rules, flags, 0)
            assert rc == -1 and msg == "scg_rollout_branch: first_action with n_steps == 0: no real step to force", msg
        # scg_rollout_audit's own refusals, under this entry point's name, with and without a first_action
        for fa in (first, None):
            for flags, n_steps, kw, why in (
                    (0, 0, {}, "n_steps == 0 without SCG_ROLLOUT_BEGIN (or _BEGIN_AT)"),
                    (0x80, 1, {}, "unknown flag"), (B | AT, 1, {}, "SCG_ROLLOUT_BEGIN and SCG_ROLLOUT_BEGIN_AT together"),
                    (B, _lib.ROLLOUT_MAX_STEPS + 1, {}, "n_steps out of range [0, SCG_ROLLOUT_MAX_STEPS]"),
                    (B, 2, {}, "rec->rows too small for the launch's pseudo-steps"),
                    (0, 1, {"force": force.data_ptr()}, "audit->force without SCG_ROLLOUT_BEGIN or _BEGIN_AT"),
                    (B, 1, {"disc_g": None}, "audit->disc_ret and audit->disc_g go together")):
                rc, msg = call(rules, flags, n_steps, fa, **kw)
                assert rc == -1 and msg == "scg_rollout_branch: " + why, msg
    rc, msg = call(4, B, 1)
    assert rc == -1 and msg == "scg_rollout_branch: unknown rule", msg
    rc, msg = call(0, B, 1, c=None)
    assert rc == -1 and msg == "scg_rollout_branch: null ctx"
    with pytest.raises(ScgError, match="first_action"):        # the wrapper refuses the same call, and a misshapen operand
        ctx.rollout(st, W, clf, MASK, 0, 0, begin=True, first_action=first)
    for bad in (first[:-1].contiguous(), first.to(torch.int8), first.cpu()):
        with pytest.raises(ScgError, match="first_action"):
            ctx.rollout(st, W, clf, MASK, 0, 1, first_action=bad)
    torch.cuda.synchronize()
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(st, f)), as_bytes(getattr(before, f))), f"a refused call wrote {f}"
    for f in STATS:
        assert int((getattr(out.stats, f) != 77).sum()) == 0, f"a refused call wrote stats.{f}"
    assert int((out.interrupts != 77).sum()) == 0 and int((out.overrides != 77).sum()) == 0 and int(out.rec.len.abs().sum()) == 0
    a = out.arrays()
    assert all((a[f] == G8).all() for f in ("applied", "cand")) and all((a[f] == GUARD).all() for f in ("v_root", "v_cand", "disc_final"))
    assert (first == 3).all()
    out.stats.zero_()
    rc, _ = call(BEST | INT, B, 1)                             # well-formed: it runs, and the step takes the action
    torch.cuda.synchronize()
    assert rc == 0 and (out.rec.len == 2).all() and (out.rec.action[1] == 3).all() and (st.action == 3).all()


# ---------------------------------------------------------------------------------------------------- 9. the agent

MAX_EP = 24


def _audit_agent():
    a = crossing_agent(n=256, n_opt=2)
    a.ctx.set_hparams(max_episode_steps=MAX_EP, reoffer_period=1)
    return a


def test_agent_branch_audit():
    a = _audit_agent()
    W0, t0 = a.W.clone(), a.t
    st0 = {f: getattr(a.state, f).clone() for f in EnvState.FIELDS}
    with pytest.raises(ScgError, match="completion bonus"):    # the test agents pay a bonus: refused for an option's values
        a.branch_audit(n_states=32, replicates=4, n_episodes=128, epsilon=0.0)
    a.ctx.set_hparams(r_option_success=0.0)
    for bad in (3, 0, 1):
        with pytest.raises(ValueError, match="even"):
            a.branch_audit(n_states=32, replicates=bad, n_episodes=128)
    with spy_calls(a.ctx) as (calls, _):
        det = a.branch_audit(n_states=32, replicates=4, n_episodes=128, epsilon=0.0, seed=5)
        again = a.branch_audit(n_states=32, replicates=4, n_episodes=128, epsilon=0.0, seed=5)
        noisy = a.branch_audit(n_states=32, replicates=4, n_episodes=128, epsilon=0.5, seed=5)
        noisy2 = a.branch_audit(n_states=32, replicates=4, n_episodes=128, epsilon=0.5, seed=5)
        taken = a.branch_audit(n_states=32, replicates=2, n_episodes=128, epsilon=0.5, seed=5, actions="taken", vfs=[0])
    torch.cuda.synchronize()
    assert calls == [], f"branch_audit called into the training context: {calls}"
    assert torch.equal(a.W, W0) and a.t == t0
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(a.state, f), st0[f]), f
    assert any(c[0].cfg.env_id_base == _lib.BRANCH_ID_BASE for c in a._branch_ctx.values())
    gamma, u = float(a.ctx.cfg.gamma), 2.0 ** -24
    assert set(det["vf"]) == {0, 1, 2} and set(taken["vf"]) == {0}
    seen = 0
    for k, rep in det["vf"].items():
        n = rep["n"]
        assert 0 <= n <= 32 and again["vf"][k]["n"] == n
        if n == 0:                                             # (at ε = 0 every recorded episode is the same one: a value function
            continue                                           # it never runs has no row)
        res = rep["result"]
        assert res.g.shape == res.ret.shape == res.goal.shape == res.steps.shape == (n, 5, 4) and res.actions.shape == (n, 5)
        assert res.finished.all() and not np.isnan(res.g).any() and (res.steps >= 1).all() and (res.steps <= MAX_EP).all()
        # one seed, one result
        assert np.array_equal(as_bytes(res.g), as_bytes(again["vf"][k]["result"].g))
        assert np.array_equal(rep["rows"][0], again["vf"][k]["rows"][0]) and np.array_equal(rep["rows"][1], again["vf"][k]["rows"][1])
        assert (rep["rows"][0] % 2 == 1).all()                                   # the held-out envs
        # ε = 0, no re-offer phase: a replicate is deterministic
        assert (as_bytes(res.g).reshape(n, 5, 4, 4) == as_bytes(res.g).reshape(n, 5, 4, 4)[:, :, :1]).all()
        assert rep["spread"]["spread_rmse"] == 0.0 and rep["spread"]["zero_variance"] == 1.0
        # ... and the recorded action's is the record's own continuation. d is L <= MAX_EP binary32 terms g_i r_i, g_i = gamma^i
        # after i rounded products: term i carries at most (i + 1) u relative error, each of the L sums at most u of a partial sum
        # that is at most S = sum gamma^i |r_i|: |d - g64| <= (2 L + 1) u S to first order; (2 L + 2) u S covers the rest
        col = res.actions == rep["taken"][:, None]
        g_rec = rep["g_recorded"]
        mine = res.g[col].reshape(n, 4)[:, 0].astype(np.float64)
        S = np.zeros(n)
        for i, (e, j) in enumerate(zip(*rep["rows"])):
            r = np.abs(det["trajectory"].per_env(e)["reward"][j:].astype(np.float64))
            S[i] = float(np.sum(gamma ** np.arange(len(r)) * r))
            assert len(r) <= MAX_EP and (res.steps[i][col[i]] == len(r)).all()
        bound = (2 * MAX_EP + 2) * u * S
        assert (np.abs(mine - g_rec) <= bound).all(), f"vf {k}: {np.abs(mine - g_rec).max()} against {bound.max()}"
        assert bound.max() < 0.04                              # (S <= 10000 + 5 MAX_EP: the bound is 3e-6 S)
        assert 0.0 <= rep["actions"]["greedy_agreement"] <= 1.0 and rep["actions"]["gap"] >= 0.0
        # at ε = 0 the recorded action IS the greedy one of the qcache the branch rebuilt
        assert np.array_equal(np.argmax(res.qcache, axis=1), rep["taken"])
        seen += n
    assert seen >= 32
    # at ε = 0.5 the episodes differ and the replicates part; one seed still gives one result
    print("states per value function:", {k: (det["vf"][k]["n"], nz["n"]) for k, nz in noisy["vf"].items()})
    assert noisy["vf"][0]["n"] == 32 and sum(nz["n"] > 0 for nz in noisy["vf"].values()) >= 2
    for k, nz in noisy["vf"].items():
        assert noisy2["vf"][k]["n"] == nz["n"] <= 32
        if nz["n"] == 0:
            continue
        assert nz["result"].g.shape == (nz["n"], 5, 4)
        assert nz["spread"]["spread_rmse"] > 0.0 and nz["spread"]["zero_variance"] < 1.0
        assert np.array_equal(as_bytes(nz["result"].g), as_bytes(noisy2["vf"][k]["result"].g)) and nz["spread"] == noisy2["vf"][k]["spread"]
        assert 0.0 <= nz["actions"]["significant"] <= 1.0
    t = taken["vf"][0]
    assert t["result"].g.shape == (t["n"], 1, 2) and "actions" not in t and t["spread"]["spread_rmse"] > 0.0
