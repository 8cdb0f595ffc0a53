"""SPEC §15 audited rollouts, host side (no GPU): tests/audit_model.py's model on the oracle backend (a forced choice is what it
says, the gate's own choice forced is the unforced run, the accumulators are §9's arithmetic and carry over), the non-vacuity
conditions of tests/test_gpu_audit.py's exact inputs, GateAudit's summary arithmetic on hand-made arrays, the header and the
binding of scg_rollout_audit, and its refusal of a null ctx."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audit_model as am
from util import oracle_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scg_abi.h")
RULES = [(False, False), (True, False), (False, True), (True, True)]          # (interrupt, best)
RULE_IDS = ["plain", "interrupt", "best", "best+interrupt"]


def _model(name, force, interrupt=False, best=False, steps=am.K, W=None, mask=am.MASK, gest=0):
    m, _, clf, W0, st, _ = am.case(name)
    mod = am.oracle_model(am.case_oracle(name, gest=gest, mask=mask), oracle_state(st, m), W0 if W is None else W, clf, mask,
                          gest=gest, interrupt=interrupt, best=best)
    mod.run(am.T0, steps, force=force, begin_at=True)
    return mod


# ---------------------------------------------------------------------------------------------------- the model on the oracle

@pytest.mark.parametrize("interrupt,best", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("name", am.MAPS)
def test_forced_begin_choice_on_the_oracle(name, interrupt, best):
    force = am.case(name)[5]
    mod = _model(name, force, interrupt, best, steps=0)
    f = force.astype(np.int64)
    on = mod.applied == 1
    oid = mod.st["option_id"]
    assert np.array_equal(oid[on], f[on]) and np.array_equal(mod.cand[on], np.abs(f[on]))
    ent, dec = mod.entries.sum(axis=0), mod.declines.sum(axis=0)
    assert np.array_equal(ent + dec, (mod.cand >= 1).astype(np.int64))           # one offer per env at most, entered or declined
    assert np.array_equal(ent[on], (f[on] > 0).astype(np.int64))
    assert (mod.v_cand[mod.cand == 0] == am.GUARD).all() and (mod.v_cand[mod.cand >= 1] != am.GUARD).all()
    assert (mod.v_root != am.GUARD).all() and (mod.disc_ret == 0).all() and (mod.disc_g == 1).all()
    assert (mod.overrides.sum() > 0) == best
    # the forced envs aside, the choice is the unforced run's
    ref = _model(name, None, interrupt, best, steps=0)
    assert not ref.applied.any()
    assert np.array_equal(oid[~on], ref.st["option_id"][~on]) and np.array_equal(mod.cand[~on], ref.cand[~on])
    assert np.array_equal(mod.st["qcache"][:, ~on].view(np.uint32), ref.st["qcache"][:, ~on].view(np.uint32))


@pytest.mark.parametrize("interrupt,best", RULES, ids=RULE_IDS)
def test_the_gates_own_choice_forced_is_the_unforced_run(interrupt, best):
    name = "pinball_simple"
    ref = _model(name, None, interrupt, best)
    own = ref.cand >= 1                                                          # (offered envs)
    first = _model(name, None, interrupt, best, steps=0)
    force = first.st["option_id"].astype(np.int8)                                # +cand where it entered, -cand where it declined
    assert np.array_equal(np.abs(force), first.cand) and own.sum() > 0
    mod = _model(name, force, interrupt, best)
    assert np.array_equal(mod.applied, (first.cand >= 1).astype(np.uint8))
    for f in ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "qcache"):
        assert np.array_equal(mod.st[f].view(np.uint8), ref.st[f].view(np.uint8)), f
    for f in ("entries", "declines", "overrides", "interrupts"):
        assert np.array_equal(getattr(mod, f), getattr(ref, f)), f
    for f in ("cand", "v_root", "v_cand", "disc_ret", "disc_g", "disc_final"):
        assert np.array_equal(getattr(mod, f).view(np.uint8), getattr(ref, f).view(np.uint8)), f


def test_accumulators_are_the_rounded_recurrence_and_carry_over():
    name = "pinball_empty"
    force = am.case(name)[5]
    one = _model(name, force, True, True)
    # by hand, from the steps' rewards: replay the same model step by step
    mod = _model(name, force, True, True, steps=0)
    d, g = np.zeros(am.N, np.float32), np.ones(am.N, np.float32)
    fin = np.full(am.N, am.GUARD)
    for j in range(am.K):
        if j == 5:                                             # a second launch goes on from the first one's arrays
            mod.carry(d.copy(), g.copy())
        mod.step(am.T0 + 1 + j)
        r, dn = mod.st["reward"], mod.st["done"] != 0
        d = np.float32(d + np.float32(g * r))
        g = np.float32(g * np.float32(0.99))
        fin[dn] = d[dn]
        d[dn], g[dn] = 0.0, 1.0
        assert np.array_equal(mod.disc_ret.view(np.uint32), d.view(np.uint32)) and np.array_equal(mod.disc_g.view(np.uint32), g.view(np.uint32))
    for f in ("disc_ret", "disc_g", "disc_final"):
        assert np.array_equal(getattr(one, f).view(np.uint32), getattr(mod, f).view(np.uint32)), f
    assert np.array_equal(one.disc_final.view(np.uint32), fin.view(np.uint32))
    assert (fin != am.GUARD).all() and len(np.unique(fin)) > 10                  # every env ended an episode, returns differ


# ---------------------------------------------------------------------------------------------------- non-vacuity of the GPU cases

@pytest.mark.parametrize("interrupt,best", RULES, ids=RULE_IDS)
@pytest.mark.parametrize("name", am.MAPS)
def test_gpu_case_inputs_are_not_vacuous(name, interrupt, best):
    """The conditions the issue sets for the forced launch of tests/test_gpu_audit.py, on that test's exact inputs."""
    force = am.case(name)[5]
    assert set(np.unique(force)) == set(range(-am.N_OPT, am.N_OPT + 1))
    mod = _model(name, force, interrupt, best)
    b = mod.begin_info
    print(name, interrupt, best, b, int(mod.episodes.sum()), int(mod.interrupts.sum()), int(mod.overrides.sum()))
    assert b["against_decline"] >= 0.10, "forced in against a declining gate on fewer than 10 % of the envs"
    assert b["against_enter"] >= 0.10, "forced out against an entering gate on fewer than 10 % of the envs"
    assert b["not_lowest"] >= 0.05, "forced into a k in C other than min C on fewer than 5 % of the envs"
    assert b["not_in_c"] >= 0.05, "|f| outside C on fewer than 5 % of the envs"
    assert mod.episodes.sum() * 4 >= am.N, "fewer than one episode per 4 envs ends inside the launch"
    assert (mod.interrupts.sum() > 0) == interrupt
    assert not best or mod.overrides.sum() > 0
    assert mod.entries.sum() > mod.applied.sum() and mod.declines.sum() > 0      # later steps offer again


def test_edge_case_inputs_are_not_vacuous():
    """tests/test_gpu_audit.py's edges: a NaN candidate is still entered by force; a gestating or disabled |f| is not applied."""
    name = "pinball_simple"
    m, _, clf, W, st, force = am.case(name)
    Wn = W.copy()
    Wn[1] = np.nan
    mod = _model(name, force, True, True, W=Wn)
    on1 = (mod.applied == 1) & (force == 1)
    assert on1.sum() >= 3 and np.isnan(mod.v_cand[on1]).all() and (mod.entries[1][on1] >= 1).all()
    base = _model(name, force, True, True)
    for mask, gest, k in ((am.MASK & ~0b1000, 0b1000, 3), (am.MASK & ~0b100, 0, 2), (0b110, 0, 5)):
        mod = _model(name, force, True, True, mask=mask, gest=gest)
        assert k != 5 or (mod.cand == 0).sum() >= 20           # with options 1 and 2 alone some states have no candidate
        named = np.abs(force.astype(np.int64)) == k
        assert (base.applied[named] == 1).sum() >= 5 and not mod.applied[named].any()
        assert mod.applied.sum() > 0


# ---------------------------------------------------------------------------------------------------- GateAudit's arithmetic

def test_gate_audit_pair_summary_on_hand_made_arrays():
    from skill_chaining_with_graphs_amd.evaluation import GateAudit
    nan = float("nan")
    #            gate enters; right     enters; wrong    declines; right   declines; wrong   NaN value: declines; tie in G: "enter" is right
    opt = np.array([1, 1, 2, 2, 2])
    v_k = np.array([2.0, 3.0, 0.0, 1.0, nan], np.float32)
    v_0 = np.array([1.0, 1.0, 1.0, 2.0, 0.0], np.float32)
    g_e = np.array([5.0, 1.0, 0.0, 9.0, 4.0], np.float32)
    g_d = np.array([4.0, 3.0, 2.0, 1.0, 4.0], np.float32)
    s = GateAudit.pair_summary(opt, v_k, v_0, g_e, g_d, [1, 0, 0, 1, 1], [1, 1, 0, 0, 1])
    o = s["overall"]
    assert o["n"] == 5 and o["enter_rate"] == 2 / 5
    assert o["mean_g_enter"] == 19 / 5 and o["mean_g_decline"] == 14 / 5 and o["mean_advantage"] == 1.0
    assert o["agreement"] == 2 / 5                             # rows 0 and 2
    assert o["regret"] == (0 + 2 + 0 + 8 + 0) / 5
    assert o["goal_rate_enter"] == 3 / 5 and o["goal_rate_decline"] == 3 / 5
    assert np.isnan(o["mean_v_k"]) and np.isnan(o["calib_enter"]) and o["mean_v_0"] == 1.0
    assert o["calib_decline"] == (-3 - 2 - 1 + 1 - 4) / 5
    assert list(s["options"]) == [1, 2]
    o1, o2 = s["options"][1], s["options"][2]
    assert o1["n"] == 2 and o1["enter_rate"] == 1.0 and o1["agreement"] == 0.5 and o1["regret"] == 1.0
    assert o1["mean_v_k"] == 2.5 and o1["calib_enter"] == (-3 + 2) / 2
    assert o2["n"] == 3 and o2["enter_rate"] == 0.0 and o2["agreement"] == 1 / 3 and o2["regret"] == 8 / 3
    assert o1["n"] + o2["n"] == o["n"]
    e = GateAudit.pair_summary([], [], [], [], [], [], [])
    assert e["overall"]["n"] == 0 and np.isnan(e["overall"]["agreement"]) and e["options"] == {}


def test_gate_audit_buffers_and_struct():
    import torch
    from skill_chaining_with_graphs_amd import _lib
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats, GateAudit
    ga = GateAudit(7, "cpu", force=[0, 1, -1, 5, -5, 0, 2])
    assert ga.force.dtype == torch.int8 and ga.applied.dtype == torch.uint8 and ga.cand.dtype == torch.int8
    assert torch.isnan(ga.v_cand).all() and torch.isnan(ga.disc_final).all() and (ga.disc_g == 1).all()
    cs = ga.c_struct()
    assert isinstance(cs, _lib.Audit) and cs.force == ga.force.data_ptr() and cs.disc_final == ga.disc_final.data_ptr()
    assert GateAudit(3).c_struct().force is None
    with pytest.raises(ValueError):
        GateAudit(3, force=[1, 2])
    assert [f for f, _ in _lib.Audit._fields_] == list(GateAudit.DTYPES)
    st = EpisodeStats(2, 3)
    assert "disc_final" not in st.per_env() and "mean_discounted_return" not in st.summary()
    st.audit = GateAudit(3)
    st.audit.disc_final.copy_(torch.tensor([1.0, 2.0, 6.0]))
    st.episodes.copy_(torch.tensor([1, 0, 1], dtype=torch.int32))
    assert st.per_env()["disc_final"] is st.audit.disc_final and st.summary()["mean_discounted_return"] == 3.5
    assert st.zero_().audit is None


# ---------------------------------------------------------------------------------------------------- the header and the binding

def test_header_binding_and_every_build_carry_scg_rollout_audit():
    """Fails without the feature: the header, the binding and every build carry scg_rollout_audit; the ABI version stays 5."""
    from skill_chaining_with_graphs_amd import _lib
    src = open(HEADER).read()
    assert re.search(r"#define\s+SCG_ABI_VERSION\s+5\b", src)
    body = re.search(r"typedef struct \{([^}]*)\}\s*scg_audit;", src).group(1)
    names = re.findall(r"\*\s*(\w+)", body)
    assert names == [f for f, _ in _lib.Audit._fields_] == ["force", "applied", "cand", "v_root", "v_cand", "disc_ret", "disc_g", "disc_final"]
    assert C.sizeof(_lib.Audit) == 8 * C.sizeof(C.c_void_p)
    sel = re.search(r"int\s+scg_rollout_select\s*\(([^;]*)\);", src).group(1)
    aud = re.search(r"int\s+scg_rollout_audit\s*\(([^;]*)\);", src).group(1)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(aud) == norm(sel).replace(", void *stream", ", const scg_audit *audit, void *stream")
    res, sig = _lib._SIGS["scg_rollout_audit"]
    sel_sig = _lib._SIGS["scg_rollout_select"][1]
    assert res is C.c_int and sig == sel_sig[:-1] + [C.POINTER(_lib.Audit), C.c_void_p]
    assert "scg_rollout_audit" in _lib.EXPORTED_SYMBOLS
    for b in _lib.BLOCK_ENVS_BUILDS:
        assert hasattr(C.CDLL(_lib.lib_path(b)), "scg_rollout_audit"), b


def test_null_ctx_and_unknown_rules_are_refused_without_a_device():
    from skill_chaining_with_graphs_amd import _lib
    lib = _lib.load()
    au = _lib.Audit()
    for rules in (0, 1, 2, 3, 4, 0xffffffff):
        for audit in (None, C.byref(au)):
            args = [None] * 13 + [C.c_uint32(0), C.c_uint64(0), C.c_int32(1), C.c_uint32(0), None, None, None, None,
                                  C.c_uint32(rules), audit, None]
            assert lib.scg_rollout_audit(None, *args) == -1
            assert lib.scg_last_error(None).decode() == "scg_rollout_audit: null ctx"


# ---------------------------------------------------------------------------------------------------- the report tool's host half

def test_report_tool_picks_offer_states_and_prints_every_column():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gate_audit_report as tool
    finally:
        sys.path.pop(0)
    from skill_chaining_with_graphs_amd.evaluation import GateAudit

    class Traj:                                                # rows: begin, root + offer, root no offer, option, root + stay at the end
        def to_numpy(self):
            f = lambda *v: np.array(v, np.float32)
            return dict(x=f(.1, .2, .3, .4, .5), y=f(.5, .4, .3, .2, .1), vx=f(0, 1, 2, 3, 4), vy=f(0, -1, -2, -3, -4),
                        vf=np.array([0, 0, 0, 2, 0], np.uint8), done=np.array([0, 0, 0, 0, 1], np.uint8),
                        option_id=np.array([0, -2, 0, 2, -1], np.int8))
    x, y, vx, vy = tool.offer_states(Traj(), 10)
    assert x.tolist() == [np.float32(.2)] and vx.tolist() == [1.0] and vy.tolist() == [-1.0] and y.dtype == np.float32
    assert len(tool.offer_states(Traj(), 0)[0]) == 0
    s = GateAudit.pair_summary([1, 2, 2], [1.0, 2.0, 0.5], [0.5, 2.5, 0.5], [3.0, 1.0, 2.0], [2.0, 2.0, 2.0], [1, 0, 1], [1, 1, 1])
    lines = tool.fmt_audit(s)
    assert len(lines) == 4 and [ln.split()[0] for ln in lines] == ["option", "1", "2", "all"]
    assert all(len(ln.split()) == 1 + len(tool.COLS) for ln in lines) and len(set(map(len, lines))) == 1
    assert lines[3].split()[1] == "3" and lines[3].split()[2] == "0.667"
