"""SPEC §15 audited rollouts on the GPU (scg_rollout_audit): without an audit it is scg_rollout_select; a forced launch equals
tests/audit_model.py's model on the library's already-verified plain steps and on the oracle, for the four `rules`; the gate's own
choice, forced, is the unforced run; the accumulators carry over a split launch; every launch geometry and block build agree; NaN
weights, a gestating or disabled |f| and ONE_EPISODE's skipped envs; the C-ABI's refusals; and the agent's gate_audit().
The inputs of the forced launches are audit_model.case's; tests/test_audit_host.py asserts their non-vacuity conditions."""
import ctypes as C

import numpy as np
import pytest
import torch

import audit_model as am
from audit_model import GUARD, K, MASK, N, N_OPT, T0, AuditModel
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.evaluation import EpisodeStats, GateAudit
from skill_chaining_with_graphs_amd.trajectory import Trajectory
from gpu_util import (GpuBackend, as_bytes, block_envs, clone_state, crossing_agent, current_block_envs, dev,  # noqa: F401
                      make_context, spy_calls, state_to_device)                                               # (block_envs: the fixture)
from util import oracle_state, random_states

pytestmark = pytest.mark.gpu

STATS = EpisodeStats.FIELDS
INT, BEST = _lib.SELECT_INTERRUPT, _lib.SELECT_BEST
B, ONE, AT = _lib.ROLLOUT_BEGIN, _lib.ROLLOUT_ONE_EPISODE, _lib.ROLLOUT_BEGIN_AT
ALL_RULES = [0, INT, BEST, BEST | INT]
RULE_IDS = ["plain", "interrupt", "best", "best+interrupt"]
AUDIT = tuple(GateAudit.DTYPES)[1:]                    # the audit's outputs (every member but force)
G8 = 77                                                # the guard of the two byte arrays


def _setup(name, n=N, gest=0, block=None, W=None, **hp):
    m, parents, clf, W0, st_np, force = am.case(name, n)
    ctx = make_context(m, n, N_OPT, block, parents, gest, am.SEED, reoffer_period=am.REOFFER, **dict(am.CASE_HP, **hp))
    return ctx, m, dev(W0 if W is None else W).view(-1), dev(clf).view(-1), st_np, force


class Out:
    """Everything one launch can write besides the env state: stats, the record, the two rule counters and the audit's arrays,
    the latter prefilled with guards (disc_ret / disc_g too: a begin launch never reads them)."""

    def __init__(self, ctx, rows=K + 1, force=None):
        n = ctx.n_envs
        self.stats = EpisodeStats(ctx.n_vf, n, ctx.device)
        self.rec = Trajectory(n, rows, 0, ctx.device)
        self.interrupts = torch.zeros((ctx.n_vf, n), dtype=torch.int32, device=ctx.device)
        self.overrides = torch.zeros((ctx.n_vf, n), dtype=torch.int32, device=ctx.device)
        self.audit = GateAudit(n, ctx.device, force=force)
        self.audit.applied.fill_(G8)
        self.audit.cand.fill_(G8)
        for f in ("v_root", "v_cand", "disc_ret", "disc_g", "disc_final"):
            getattr(self.audit, f).fill_(float(GUARD))

    def record(self):
        ln = self.rec.len.cpu().numpy()
        return {f: getattr(self.rec, f).cpu().numpy() for f in self.rec.fields}, ln

    def arrays(self):
        return {f: getattr(self.audit, f).cpu().numpy() for f in AUDIT}


def _head(st, W, clf, mask, t0, n_steps, flags, cs):
    return [C.c_void_p(getattr(st, f).data_ptr()) for f in EnvState.FIELDS] + [
        C.c_void_p(W.data_ptr()), C.c_void_p(clf.data_ptr()), C.c_uint32(mask), C.c_uint64(t0), C.c_int32(n_steps),
        C.c_uint32(flags), None if cs is None else C.byref(cs)]


def _launch(ctx, st, W, clf, t0, n_steps, flags, rules, out, audit="given", mask=MASK, rec=True):
    """scg_rollout_audit (audit: "given" = out.audit's struct, "empty" = a struct of NULLs, None = NULL), or with
    audit = "select" scg_rollout_select."""
    cs, rc = out.stats.c_struct(), out.rec.c_struct()
    tail = [C.c_void_p(out.interrupts.data_ptr()), C.c_void_p(out.overrides.data_ptr()), C.byref(rc) if rec else None, C.c_uint32(rules)]
    if audit == "select":
        return ctx._call("scg_rollout_select", *_head(st, W, clf, mask, t0, n_steps, flags, cs), *tail, ctx._stream())
    au = out.audit.c_struct() if audit == "given" else _lib.Audit()
    ctx._call("scg_rollout_audit", *_head(st, W, clf, mask, t0, n_steps, flags, cs), *tail, None if audit is None else C.byref(au),
              ctx._stream())


def _canon(a):
    """An array's bits with every NaN made the same one."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a.view(np.uint8)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7fc00000
    return b


def _same_arrays(a, b, msg, fields=AUDIT, nan=False):
    for f in fields:
        x, y = (_canon(v[f]) if nan else as_bytes(v[f]) for v in (a, b))
        assert np.array_equal(x, y), f"{msg}: audit.{f} differs on {int(np.sum(x != y))} entries"


def _same_state(a, b, msg, nan=False):
    for f in EnvState.FIELDS:
        x, y = (getattr(s, f).cpu().numpy() if not isinstance(s, dict) else s[f] for s in (a, b))
        assert np.array_equal(_canon(x) if nan else as_bytes(x), _canon(y) if nan else as_bytes(y)), f"{msg}: {f} differs"


def _same_launch(st_a, a, st_b, b, msg, record=True, audit=AUDIT):
    torch.cuda.synchronize()
    _same_state(st_a, st_b, msg)
    for f in STATS:
        assert np.array_equal(as_bytes(getattr(a.stats, f)), as_bytes(getattr(b.stats, f))), f"{msg}: stats.{f}"
    for f in ("interrupts", "overrides"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f"{msg}: {f}"
    if record:
        (ra, la), (rb, lb) = a.record(), b.record()
        assert np.array_equal(la, lb), f"{msg}: len"
        valid = np.arange(a.rec.rows)[:, None] < la[None, :]
        for f in ra:
            assert np.array_equal(as_bytes(ra[f][valid]), as_bytes(rb[f][valid])), f"{msg}: record field {f}"
    _same_arrays(a.arrays(), b.arrays(), msg, audit)


# ---------------------------------------------------------------------------------------------------- 1. no audit

@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
def test_no_audit_is_scg_rollout_select(rules):
    ctx, m, W, clf, st_np, _ = _setup("pinball_simple")
    ref_st = state_to_device(st_np, ctx)
    ref = Out(ctx)
    runs = {how: (clone_state(ref_st), Out(ctx, force=np.zeros(N, np.int8) if how == "given" else None))
            for how in (None, "empty", "given")}
    t = T0
    for flags, steps in ((AT, K), (0, K)):
        _launch(ctx, ref_st, W, clf, t, steps, flags, rules, ref, audit="select")
        for how, (st, out) in runs.items():
            if how == "given" and not flags:
                out.audit.force = None                         # (a launch without a begin takes no force)
            _launch(ctx, st, W, clf, t, steps, flags, rules, out, audit=how)
            _same_launch(st, out, ref_st, ref, f"rules {rules} audit {how} flags {flags}", audit=())
        t += steps + 1
    for how in (None, "empty"):                               # nothing of the audit's is written without one
        a = runs[how][1].arrays()
        assert all((a[f] == G8).all() for f in ("applied", "cand")) and all((a[f] == GUARD).all() for f in AUDIT[2:])
    a = runs["given"][1].arrays()
    assert not a["applied"].any() and (a["cand"] != G8).all() and (a["v_root"] != GUARD).all() and (a["disc_final"] != GUARD).all()
    assert int(ref.stats.entries.sum()) > 0 and int(ref.stats.declines.sum()) > 0


# ---------------------------------------------------------------------------------------------------- 2. the model

def _check_model(out, st, mod, msg, nan=False):
    _same_state(st, mod.st, msg, nan)
    for f in ("entries", "declines"):
        assert np.array_equal(getattr(out.stats, f).cpu().numpy(), getattr(mod, f)), f"{msg}: {f}"
    assert np.array_equal(out.overrides.cpu().numpy(), mod.overrides), f"{msg}: overrides"
    assert np.array_equal(out.interrupts.cpu().numpy(), mod.interrupts), f"{msg}: interrupts"
    _same_arrays(out.arrays(), mod.audit_arrays(), msg, nan=nan)


def _gpu_model(ctx, st, W, clf, mask, gest, rules):
    mod = AuditModel(GpuBackend(ctx, W, clf, mask), ctx.n_vf, mask, gest, ctx.parents, ctx.cfg.reoffer_period,
                     ctx.cfg.env_id_base, gamma=ctx.cfg.gamma, interrupt=bool(rules & INT), best=bool(rules & BEST))
    mod.seat(st)
    return mod


def _oracle_model(name, n, st_np, m, W, clf, rules, mask=MASK, gest=0):
    return am.oracle_model(am.case_oracle(name, n, gest=gest, mask=mask), oracle_state(st_np, m), W.cpu().numpy(), clf.cpu().numpy(),
                           mask, gest=gest, interrupt=bool(rules & INT), best=bool(rules & BEST))


@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
@pytest.mark.parametrize("name", am.MAPS)
def test_forced_launch_equals_the_model(name, rules):
    ctx, m, W, clf, st_np, force = _setup(name)
    st = state_to_device(st_np, ctx)
    twin = clone_state(st)
    out = Out(ctx, force=force)
    _launch(ctx, twin, W, clf, T0, K, AT, rules, out)
    torch.cuda.synchronize()
    msg = f"{name} rules {rules}"
    # ---- the model on the library's own plain steps
    mod = _gpu_model(ctx, st, W, clf, MASK, 0, rules)
    mod.run(T0, K, force=force, begin_at=True)
    torch.cuda.synchronize()
    _check_model(out, twin, mod, msg)
    for f in [f for f in STATS if f not in ("entries", "declines")]:
        assert np.array_equal(as_bytes(getattr(out.stats, f)), as_bytes(getattr(mod.B.stats, f))), f"{msg}: stats.{f}"
    rows, ln = mod.record()
    got, got_len = out.record()
    assert np.array_equal(got_len, ln) and (ln == K + 1).all()
    for f in rows:
        assert np.array_equal(as_bytes(got[f]), as_bytes(rows[f])), f"{msg}: record field {f}"
    # ---- and on the oracle
    omod = _oracle_model(name, N, st_np, m, W, clf, rules)
    omod.run(T0, K, force=force, begin_at=True)
    _check_model(out, twin, omod, msg + " oracle")
    a = out.arrays()
    print(msg, mod.begin_info, int(mod.episodes.sum()), int(a["applied"].sum()))
    assert a["applied"].sum() > 0 and mod.episodes.sum() * 4 >= N


# ---------------------------------------------------------------------------------------------------- 3. the gate's own choice

@pytest.mark.parametrize("rules", ALL_RULES, ids=RULE_IDS)
def test_the_gates_own_choice_forced_is_the_unforced_run(rules):
    ctx, m, W, clf, st_np, _ = _setup("pinball_empty")
    ref_st = state_to_device(st_np, ctx)
    st, probe_st = clone_state(ref_st), clone_state(ref_st)
    probe = Out(ctx)
    _launch(ctx, probe_st, W, clf, T0, 0, AT, rules, probe)                      # the unforced begin: +cand entered, -cand declined
    force = probe_st.option_id.to(torch.int8)
    assert torch.equal(force.abs(), probe.audit.cand) and int((force > 0).sum()) > 0 and int((force < 0).sum()) > 0
    ref, out = Out(ctx), Out(ctx, force=force)
    _launch(ctx, ref_st, W, clf, T0, K, AT, rules, ref)
    _launch(ctx, st, W, clf, T0, K, AT, rules, out)
    _same_launch(st, out, ref_st, ref, f"rules {rules}", audit=AUDIT[1:])
    assert torch.equal(out.audit.applied, (probe.audit.cand >= 1).to(torch.uint8)) and not ref.audit.applied.any()


# ---------------------------------------------------------------------------------------------------- 4. carry-over

@pytest.mark.parametrize("rules", [0, BEST | INT], ids=["plain", "best+interrupt"])
def test_accumulators_carry_over_a_split_launch(rules):
    ctx, m, W, clf, st_np, force = _setup("pinball_simple")
    one_st = state_to_device(st_np, ctx)
    two_st = clone_state(one_st)
    one, two = Out(ctx, force=force), Out(ctx, force=force)
    _launch(ctx, one_st, W, clf, T0, K, AT, rules, one, rec=False)
    _launch(ctx, two_st, W, clf, T0, 5, AT, rules, two, rec=False)
    torch.cuda.synchronize()
    mid = two.arrays()
    assert (mid["disc_final"] == GUARD).sum() > N // 2 and (mid["disc_g"] != 1).sum() > N // 2      # most episodes are under way
    two.audit.force = None
    begin_outputs = {f: mid[f] for f in ("applied", "cand", "v_root", "v_cand")}
    _launch(ctx, two_st, W, clf, T0 + 6, 7, 0, rules, two, rec=False)
    _same_launch(two_st, two, one_st, one, f"rules {rules} 5 + 7", record=False)
    _same_arrays(two.arrays(), begin_outputs, "a launch without a begin wrote a begin output", tuple(begin_outputs))


# ---------------------------------------------------------------------------------------------------- 5. geometry and builds

def _forced_two_launches(name, n, rules, block=None):
    ctx, m, W, clf, st_np, force = _setup(name, n=n, block=block)
    st = state_to_device(st_np, ctx)
    out = Out(ctx, force=force)
    _launch(ctx, st, W, clf, T0, K, AT, rules, out)
    out.audit.force = None
    _launch(ctx, st, W, clf, T0 + K + 1, K, 0, rules, out, rec=False)
    torch.cuda.synchronize()
    return st, out


def test_every_launch_geometry(monkeypatch):
    ref_st, ref = _forced_two_launches("pinball_simple", N, BEST | INT)
    assert int(ref.audit.applied.sum()) > 0 and int(ref.interrupts.sum()) > 0
    for epw in (2, 32):
        monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
        st, out = _forced_two_launches("pinball_simple", N, BEST | INT)
        _same_launch(st, out, ref_st, ref, f"epw {epw}")


@pytest.mark.parametrize("block_envs", [64, 256], indirect=True)
def test_every_block_build(block_envs):
    ref_st, ref = _forced_two_launches("pinball_empty", N, INT)
    st, out = _forced_two_launches("pinball_empty", N, INT, block=current_block_envs())
    assert int(ref.audit.applied.sum()) > 0
    _same_launch(st, out, ref_st, ref, f"block {block_envs}")


@pytest.mark.parametrize("n", [1, 257])
def test_edge_launch_sizes_equal_the_oracle_model(n):
    ctx, m, W, clf, st_np, force = _setup("pinball_simple", n=n)
    if n == 1:                                                 # the one env's force opposes what the gate does with its own offer
        first = _oracle_model("pinball_simple", n, st_np, m, W, clf, BEST | INT)
        first.run(T0, 0, begin_at=True)
        assert first.cand[0] >= 1
        force[:] = -first.st["option_id"][0]
    st = state_to_device(st_np, ctx)
    out = Out(ctx, force=force)
    _launch(ctx, st, W, clf, T0, K, AT, BEST | INT, out)
    torch.cuda.synchronize()
    omod = _oracle_model("pinball_simple", n, st_np, m, W, clf, BEST | INT)
    omod.run(T0, K, force=force, begin_at=True)
    _check_model(out, st, omod, f"n {n}")
    assert int(out.audit.applied.sum()) > 0 and (out.rec.len.cpu().numpy() == K + 1).all()


# ---------------------------------------------------------------------------------------------------- 6. edges

@pytest.mark.parametrize("name", am.MAPS)
def test_forced_entry_into_an_option_whose_values_are_nan(name):
    W = am.case(name)[3].copy()
    W[1] = np.nan
    ctx, m, Wd, clf, st_np, force = _setup(name, W=W)
    st = state_to_device(st_np, ctx)
    out = Out(ctx, force=force)
    _launch(ctx, st, Wd, clf, T0, K, AT, BEST | INT, out)
    torch.cuda.synchronize()
    omod = _oracle_model(name, N, st_np, m, Wd, clf, BEST | INT)
    omod.run(T0, K, force=force, begin_at=True)
    _check_model(out, st, omod, name, nan=True)
    a = out.arrays()
    on1 = (a["applied"] == 1) & (force == 1)
    assert on1.sum() >= 3 and np.isnan(a["v_cand"][on1]).all() and (out.stats.entries[1].cpu().numpy()[on1] >= 1).all()


@pytest.mark.parametrize("mask,gest,k", [(MASK & ~0b1000, 0b1000, 3), (MASK & ~0b100, 0, 2), (0b110, 0, 5)],
                         ids=["gestating", "not enabled", "two options"])
def test_a_force_that_names_no_candidate_is_not_applied(mask, gest, k):
    name = "pinball_simple"
    ctx, m, W, clf, st_np, force = _setup(name, gest=gest)
    st = state_to_device(st_np, ctx)
    out = Out(ctx, force=force)
    _launch(ctx, st, W, clf, T0, K, AT, BEST | INT, out, mask=mask)
    torch.cuda.synchronize()
    omod = _oracle_model(name, N, st_np, m, W, clf, BEST | INT, mask=mask, gest=gest)
    omod.run(T0, K, force=force, begin_at=True)
    _check_model(out, st, omod, f"option {k}")
    a = out.arrays()
    named = np.abs(force.astype(np.int64)) == k
    assert named.sum() >= 20 and not a["applied"][named].any() and a["applied"].sum() > 0
    assert int(out.stats.entries[k].sum()) == 0 and int(out.stats.declines[k].sum()) == 0
    none = a["cand"] == 0                                      # no candidate: nothing offered, v_cand keeps its guard value
    assert (a["v_cand"][none] == GUARD).all() and (a["v_cand"][~none] != GUARD).all() and (a["v_root"] != GUARD).all()
    assert k != 5 or none.sum() >= 20
    # a force outside 1 .. n_options names nothing either
    far = np.where(np.arange(N) % 2 == 0, 6, -128).astype(np.int8)
    st2, ref_st = state_to_device(st_np, ctx), state_to_device(st_np, ctx)
    out2, ref = Out(ctx, force=far), Out(ctx)
    _launch(ctx, st2, W, clf, T0, K, AT, BEST | INT, out2, mask=mask)
    _launch(ctx, ref_st, W, clf, T0, K, AT, BEST | INT, ref, mask=mask)
    _same_launch(st2, out2, ref_st, ref, "a force outside the options")
    assert not out2.audit.applied.any()


def test_one_episode_skipped_envs_write_nothing():
    ctx, m, W, clf, st_np, force = _setup("pinball_simple")
    st = state_to_device(st_np, ctx)
    first = Out(ctx, force=force)
    _launch(ctx, st, W, clf, T0, 3, AT, BEST | INT, first)
    skipped = torch.as_tensor(np.random.default_rng(5).random(N) < 0.5, device=ctx.device)
    first.stats.finished.copy_(skipped.to(torch.uint8))
    before = clone_state(st)
    out = Out(ctx)
    out.stats = first.stats
    _launch(ctx, st, W, clf, T0 + 4, 4, ONE, BEST | INT, out)
    torch.cuda.synchronize()
    s = skipped.cpu().numpy()
    a = out.arrays()
    assert 50 < s.sum() < N - 50
    assert all((a[f][s] == G8).all() for f in ("applied", "cand")) and all((a[f][s] == GUARD).all() for f in AUDIT[2:])
    assert (a["disc_ret"][~s] != GUARD).all() and (a["disc_g"][~s] != GUARD).all()
    assert (a["applied"] == G8).all() and (a["cand"] == G8).all() and (a["v_root"] == GUARD).all()         # no begin: no begin output
    for f in EnvState.FIELDS:
        x, y = getattr(st, f).cpu().numpy(), getattr(before, f).cpu().numpy()
        assert np.array_equal(as_bytes(x[..., s]), as_bytes(y[..., s])), f"a skipped env's {f} was written"
    assert (st.ep_steps.cpu().numpy()[~s] != before.ep_steps.cpu().numpy()[~s]).all()
    assert (out.rec.len.cpu().numpy()[s] == 0).all()


# ---------------------------------------------------------------------------------------------------- 7. refusals

def test_c_abi_refusals_launch_nothing():
    n = 64
    ctx, m, W, clf, st_np, force = _setup("pinball_simple", n=n)
    st = state_to_device(st_np, ctx)
    before = clone_state(st)
    lib = ctx.lib
    out = Out(ctx, 2, force=force)
    for f in STATS:
        getattr(out.stats, f).fill_(77)
    out.interrupts.fill_(77)
    out.overrides.fill_(77)
    cs, rec = out.stats.c_struct(), out.rec.c_struct()
    full = out.audit.c_struct()

    def variant(**kw):
        au = out.audit.c_struct()
        for f, v in kw.items():
            setattr(au, f, v)
        return au

    def call(rules, flags, n_steps, au, c=ctx._ctx):
        rc = lib.scg_rollout_audit(c, *_head(st, W, clf, MASK, 0, n_steps, flags, cs), C.c_void_p(out.interrupts.data_ptr()),
                                   C.c_void_p(out.overrides.data_ptr()), C.byref(rec), C.c_uint32(rules),
                                   None if au is None else C.byref(au), None)
        return rc, lib.scg_last_error(c).decode()

    for rules in ALL_RULES:
        for flags in (0, ONE):                                 # a force needs the begin pseudo-step
            rc, msg = call(rules, flags, 1, full)
            assert rc == -1 and msg == "scg_rollout_audit: audit->force without SCG_ROLLOUT_BEGIN or _BEGIN_AT", msg
        for au in (variant(disc_g=None), variant(disc_ret=None), variant(force=None, disc_g=None)):
            rc, msg = call(rules, B, 1, au)
            assert rc == -1 and msg == "scg_rollout_audit: audit->disc_ret and audit->disc_g go together", msg
        # scg_rollout_select's own refusals, with and without an audit
        for au in (full, None):
            for flags, n_steps, why in ((0x80, 1, "unknown flag"), (B | AT, 1, "SCG_ROLLOUT_BEGIN and SCG_ROLLOUT_BEGIN_AT together"),
                                        (B, _lib.ROLLOUT_MAX_STEPS + 1, "n_steps out of range [0, SCG_ROLLOUT_MAX_STEPS]"),
                                        (B, 2, "rec->rows too small for the launch's pseudo-steps")):
                rc, msg = call(rules, flags, n_steps, au)
                assert rc == -1 and msg == "scg_rollout_audit: " + why, msg
    for rules in (4, 8 | BEST, 0xfffffffc):
        rc, msg = call(rules, B, 1, full)
        assert rc == -1 and msg == "scg_rollout_audit: unknown rule", msg
    rc, msg = call(BEST, B, 1, full, c=None)
    assert rc == -1 and msg == "scg_rollout_audit: null ctx"
    torch.cuda.synchronize()
    _same_state(st, before, "a refused call wrote the state")
    for f in STATS:
        assert int((getattr(out.stats, f) != 77).sum()) == 0, f"a refused call wrote stats.{f}"
    assert int((out.interrupts != 77).sum()) == 0 and int((out.overrides != 77).sum()) == 0 and int(out.rec.len.abs().sum()) == 0
    a = out.arrays()
    assert all((a[f] == G8).all() for f in ("applied", "cand")) and all((a[f] == GUARD).all() for f in AUDIT[2:])
    out.stats.zero_()
    cs = out.stats.c_struct()
    rc, _ = call(BEST | INT, B, 1, full)                       # well-formed: it runs
    torch.cuda.synchronize()
    assert rc == 0 and (out.rec.len == 2).all() and (out.audit.applied != G8).all()


# ---------------------------------------------------------------------------------------------------- 8. the agent

def test_agent_gate_audit():
    a = crossing_agent(n_opt=2)
    W0, t0 = a.W.clone(), a.t
    st0 = {f: getattr(a.state, f).clone() for f in EnvState.FIELDS}
    n = 1000
    x, y, _, _ = random_states(a.map, n, 7)
    states = (dev(x), dev(y))
    a.evaluate(states=states)                                  # (creates the evaluation context)
    eval_calls = []
    with spy_calls(a.ctx) as (calls, _), spy_calls(a._eval_ctx[n][0], eval_calls):
        res = a.gate_audit(states=states)
        only2 = a.gate_audit(k=2, states=states)
        summary, per_env = a.evaluate(states=states, per_env=True, discounted=True)
        plain = a.evaluate(states=states)
        for bad in (0, 3, -1):
            with pytest.raises(ValueError):
                a.gate_audit(k=bad, states=states)
    torch.cuda.synchronize()
    assert calls == [], f"gate_audit called into the training context: {calls}"
    assert "scg_rollout_audit" in eval_calls
    assert torch.equal(a.W, W0) and a.t == t0
    for f in EnvState.FIELDS:
        assert torch.equal(getattr(a.state, f), st0[f]), f
    # ---- counts add up
    o, per = res["overall"], res["per_state"]
    assert 0 < o["n"] <= n and o["n"] == len(per["index"]) == sum(r["n"] for r in res["options"].values())
    assert set(res["options"]) == set(np.unique(per["option"]).tolist()) <= {1, 2}
    for k, r in res["options"].items():
        assert r["n"] == int((per["option"] == k).sum())
    assert all(len(v) == o["n"] for v in per.values()) and (np.diff(per["index"]) > 0).all()
    assert 0.0 < o["enter_rate"] < 1.0 and 0.0 <= o["agreement"] <= 1.0 and o["regret"] >= 0.0
    assert o["mean_advantage"] == pytest.approx(o["mean_g_enter"] - o["mean_g_decline"], rel=1e-9, abs=1e-6)
    assert set(only2["options"]) == {2} and only2["options"][2]["n"] == only2["overall"]["n"] >= res["options"].get(2, {"n": 0})["n"]
    # ---- the branch the gate chose is the unforced evaluation of the same states
    with np.errstate(invalid="ignore"):
        chosen = np.where(per["v_k"] >= per["v_0"], per["g_enter"], per["g_decline"])
    unforced = per_env["disc_final"].cpu().numpy()
    assert np.array_equal(chosen.view(np.uint32), unforced[per["index"]].view(np.uint32))
    assert not np.array_equal(per["g_enter"], per["g_decline"]), "both branches give the same return everywhere"
    assert summary["mean_discounted_return"] == pytest.approx(float(unforced.astype(np.float64).mean()), rel=1e-9)
    assert {k: v for k, v in summary.items() if k != "mean_discounted_return"} == plain
