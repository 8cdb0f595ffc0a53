"""SPEC §19 branch rollouts, host side (no GPU): the header and the binding of scg_rollout_branch and its export by every build;
Trajectory.resume_state on hand-made rows (the opt_steps recurrence against a plain loop, every term code, a declined id, a
TIMEOUT followed by re-entry, both refusals) and against the oracle's own state arrays over a recorded ε-greedy run; and
BranchResult's statistics on hand-made returns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audit_model as am
import option_rules as rules
from util import HP, SCALE, SIBLING_PARENTS, oracle_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scg_abi.h")
BEGIN = 255


# ---------------------------------------------------------------------------------------------------- header, binding, exports

def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/scg_abi.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_point_and_the_binding_matches(pkg):
    from skill_chaining_with_graphs_amd import _lib
    branch, audit = _declaration("scg_rollout_branch"), _declaration("scg_rollout_audit")
    # scg_rollout_audit's arguments up to and including `audit`, then first_action, then the stream
    assert branch[:-2] == audit[:-1] and audit[-2] == "const scg_audit *audit"
    assert branch[-2:] == ["const uint8_t *first_action", "void *stream"]
    res, args = _lib._SIGS["scg_rollout_branch"]
    _, a_args = _lib._SIGS["scg_rollout_audit"]
    assert res is C.c_int and len(args) == len(branch)
    assert args[:-2] == a_args[:-1] and args[-2:] == [C.c_void_p, C.c_void_p]
    assert "scg_rollout_branch" in pkg.EXPORTED_SYMBOLS
    assert _lib.NO_FIRST_ACTION == 255 and _lib.NO_FIRST_ACTION >= _lib.NUM_ACTIONS and _lib.BRANCH_ID_BASE == 2 ** 40
    assert _lib.ABI_VERSION == 5


def test_every_build_exports_it_and_refuses_a_null_ctx(pkg):
    from skill_chaining_with_graphs_amd import _lib
    for b in _lib.BLOCK_ENVS_BUILDS:
        lib = _lib.load(b)
        assert hasattr(lib, "scg_rollout_branch"), b
        _, args = _lib._SIGS["scg_rollout_branch"]
        zeros = [None if (a is C.c_void_p or hasattr(a, "contents")) else a(0) for a in args]
        assert lib.scg_rollout_branch(*zeros) == -1
        assert b"scg_rollout_branch" in lib.scg_last_error(None)


# ---------------------------------------------------------------------------------------------------- resume_state by hand

def _traj(rows, n_vf=4):
    """A one-env host Trajectory from a list of rows (dicts; missing fields 0); x = the row index, so that the state a
    resume takes is recognisable."""
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    tr = Trajectory(1, len(rows), 0, "cpu", n_vf=n_vf)
    launch = {"len": np.array([len(rows)], np.int32)}
    for f in tr.fields:
        dt = np.float32 if f in ("x", "y", "vx", "vy", "reward") else np.int8 if f == "option_id" else np.uint8
        launch[f] = np.array([[r.get(f, 0)] for r in rows]).astype(dt)
    launch["x"] = np.arange(len(rows), dtype=np.float32)[:, None]
    launch["y"] = 10 + launch["x"]
    return tr.append(launch)


def _plain_loop(rows, row):
    """The kernel's recurrence, spelled as a loop: opt_steps before step `row`."""
    s = 0
    for r in rows[:row]:
        s = s + 1 if (r.get("vf", 0) >= 1 and r.get("term", 0) == 0 and r.get("action") != BEGIN) else 0
    return s


def _rows_with_option_ended_by(term):
    """Begin, two root rows (the second enters option 2), option 2 kept for three rows and ended on its fourth by `term`; then a
    root row. term 5 (interrupted) leaves -3; term 4 (TIMEOUT) re-enters option 2 at once; term 2 ends the episode."""
    after = {1: 1, 2: 0, 3: 0, 4: 2, 5: -3}[term]
    rows = [dict(action=BEGIN, done=2, option_id=0),
            dict(action=1, option_id=-1),                                       # a declined id
            dict(action=0, option_id=2),                                        # enters 2
            dict(action=2, vf=2, option_id=2), dict(action=2, vf=2, option_id=2), dict(action=3, vf=2, option_id=2),
            dict(action=4, vf=2, term=term, option_id=after, done=1 if term == 2 else 0)]
    if term != 2:
        rows += [dict(action=0, vf=after if after >= 1 else 0, option_id=after), dict(action=1, vf=after if after >= 1 else 0, option_id=after)]
    return rows


@pytest.mark.parametrize("term", [1, 2, 3, 4, 5])
def test_resume_state_on_hand_made_rows(term):
    rows = _rows_with_option_ended_by(term)
    tr = _traj(rows)
    last = len(rows) - 1
    at = np.arange(1, last + 1)
    got = tr.resume_state(np.zeros(len(at), np.int64), at)
    assert np.array_equal(got["ep_steps"], at - 1) and got["ep_steps"].dtype == np.int32
    assert np.array_equal(got["x"], (at - 1).astype(np.float32)) and np.array_equal(got["y"], (at + 9).astype(np.float32))
    assert np.array_equal(got["option_id"], [rows[j - 1]["option_id"] for j in at]) and got["option_id"].dtype == np.int32
    assert np.array_equal(got["opt_steps"], [_plain_loop(rows, j) for j in at])
    # spelled out: 0 behind the begin row and the root rows, 0 on entry, then 1, 2, 3 while option 2 goes on
    assert list(got["opt_steps"][:6]) == [0, 0, 0, 1, 2, 3]
    assert list(got["vf_next"][:6]) == [0, 0, 2, 2, 2, 2]                       # -1: the root runs
    if term != 2:
        # behind the row that ended the option the counter is 0 whatever the code (5: interrupted; 4: entered again at once)
        assert got["opt_steps"][6] == 0
        assert got["vf_next"][6] == {1: 1, 3: 0, 4: 2, 5: 0}[term] and got["option_id"][6] == {1: 1, 3: 0, 4: 2, 5: -3}[term]
        assert got["opt_steps"][7] == (1 if term in (1, 4) else 0)             # the re-entered option's first kept row counts 1


def test_resume_state_refusals_and_out_of_range_ids():
    rows = _rows_with_option_ended_by(2)                                        # row 6 ends the episode
    tr = _traj(rows + [dict(action=0, option_id=0)])                            # (a row behind it, as a longer record would hold)
    tr.resume_state([0], [6])
    with pytest.raises(ValueError, match="ended the episode"):
        tr.resume_state([0], [7])
    for bad in (0, 8, 9, -1):
        with pytest.raises(ValueError, match="row outside"):
            tr.resume_state([0], [bad])
    with pytest.raises(ValueError, match="env outside"):
        tr.resume_state([1], [1])
    # the begin row's done = 2 is no episode end: row 1 resumes behind it
    assert tr.resume_state([0], [1])["ep_steps"][0] == 0
    # an id at or beyond n_vf names the root
    tr = _traj([dict(action=BEGIN, done=2, option_id=4), dict(action=0, option_id=3), dict(action=0, vf=3, option_id=3)], n_vf=4)
    got = tr.resume_state([0, 0], [1, 2])
    assert list(got["vf_next"]) == [0, 3] and list(got["option_id"]) == [4, 3]


# ---------------------------------------------------------------------------------------------------- resume_state on the oracle

N_ENVS, STEPS, T0 = 64, 30, 11


def _oracle_record(name):
    """A plain ε-greedy run of the oracle (audit_model's case with its five options, BEGIN_AT then STEPS steps) as a host
    one-episode Trajectory, plus the oracle's own (option_id, opt_steps, ep_steps, x, y, vx, vy) BEFORE every step."""
    import sc_oracle
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    m, parents, clf, W, st_np, _ = am.case(name, N_ENVS)
    orc = sc_oracle.Oracle(scg.load_map(name), SCALE, n_envs=N_ENVS, n_options=am.N_OPT, seed=am.SEED, enabled_mask=am.MASK,
                           n_threads=4, reoffer_period=am.REOFFER, **dict(HP, epsilon=0.3, max_option_steps=6))
    orc.set_parents(SIBLING_PARENTS)
    mod = am.oracle_model(orc, oracle_state(st_np, m), W, clf, am.MASK)
    keys = ("option_id", "opt_steps", "ep_steps", "x", "y", "vx", "vy")
    mod.begin(T0, begin_at=True)
    st = mod.st
    z = lambda dt: np.zeros((STEPS + 1, N_ENVS), dt)
    rec = {"x": z(np.float32), "y": z(np.float32), "vx": z(np.float32), "vy": z(np.float32), "reward": z(np.float32),
           "action": z(np.uint8), "done": z(np.uint8), "vf": z(np.uint8), "term": z(np.uint8), "option_id": z(np.int8)}
    for f in ("x", "y", "vx", "vy", "option_id"):
        rec[f][0] = st[f]
    rec["action"][0], rec["done"][0] = BEGIN, 2
    before = []
    ln = np.full(N_ENVS, STEPS + 1, np.int32)
    for j in range(1, STEPS + 1):
        before.append({f: np.array(st[f], copy=True) for f in keys})
        o = rules.vf_of(st["option_id"], am.N_VF)
        mod.step(T0 + j)
        for f in ("x", "y", "vx", "vy", "reward", "action", "done", "option_id"):
            rec[f][j] = st[f]                                   # (a done row's state is the reset's: no resume reads it)
        rec["vf"][j] = o
        rec["term"][j] = np.where((o >= 1) & ~mod.keep, 4, 0)   # some code where the option ended: resume_state reads != 0 only
        ended = (st["done"] != 0) & (ln == STEPS + 1)
        ln[ended] = j + 1
    tr = Trajectory(N_ENVS, STEPS + 1, 0, "cpu", n_vf=am.N_VF)
    return tr.append(dict(rec, len=ln)), before, ln


@pytest.mark.parametrize("name", am.MAPS)
def test_resume_state_is_the_oracles_state_at_every_row(name, oracle_mod):
    tr, before, ln = _oracle_record(name)
    env = np.concatenate([np.full(ln[e] - 1, e) for e in range(N_ENVS)])
    row = np.concatenate([np.arange(1, ln[e]) for e in range(N_ENVS)])
    got = tr.resume_state(env, row)
    for f in ("option_id", "opt_steps", "ep_steps"):
        want = np.array([before[j - 1][f][e] for e, j in zip(env, row)])
        assert np.array_equal(got[f], want), f"{name}: {f} differs on {int(np.sum(got[f] != want))} of {len(want)} rows"
    for f in ("x", "y", "vx", "vy"):
        want = np.array([before[j - 1][f][e] for e, j in zip(env, row)], np.float32)
        assert np.array_equal(got[f].view(np.uint32), want.view(np.uint32)), f"{name}: {f}"
    assert np.array_equal(got["vf_next"], rules.vf_of(got["option_id"], am.N_VF))
    # non-vacuity: options run for several steps and end, ids are declined, and the rows go well past the first steps
    assert got["opt_steps"].max() >= 3 and (got["option_id"] < 0).sum() >= 10 and (got["vf_next"] >= 1).sum() >= 50
    assert len(row) >= 10 * N_ENVS and int(np.sum((got["opt_steps"] == 0) & (got["vf_next"] >= 1) & (row > 1))) >= 5


# ---------------------------------------------------------------------------------------------------- BranchResult by hand

def _result(g, actions=None):
    from skill_chaining_with_graphs_amd.evaluation import BranchResult
    g = np.asarray(g, np.float32)
    M, A, R = g.shape
    acts = np.tile(np.arange(A, dtype=np.uint8), (M, 1)) if actions is None else np.asarray(actions, np.uint8)
    return BranchResult(acts, g, g.astype(np.float64), np.zeros(g.shape, bool), np.ones(g.shape, np.int64))


def test_spread_of_known_variances():
    # state 0: replicates -1, 1, -1, 1: variance 4/3; state 1: 0, 2, 4, 6: variance 20/3; state 2: constant
    g = np.array([[[-1, 1, -1, 1]], [[0, 2, 4, 6]], [[5, 5, 5, 5]]], np.float32)
    s = _result(g).spread(g_recorded=[1.0, 3.0, 5.0])
    assert s["n"] == 3 and s["spread_rmse"] == pytest.approx(np.sqrt((4 / 3 + 20 / 3 + 0) / 3), rel=1e-12)
    assert s["zero_variance"] == pytest.approx(1 / 3)
    # z^2 over the two states with variance: (1 - 0)^2 / (4/3 * 5/4) and (3 - 3)^2 / ...
    assert s["recorded_z2"] == pytest.approx(0.5 * (1.0 / (4 / 3 * 1.25)), rel=1e-12)
    assert s["recorded_z2_median"] == pytest.approx(0.5 * (1.0 / (4 / 3 * 1.25)), rel=1e-12)      # (of 0.6 and 0)
    # the recorded action's column, one per state
    g2 = np.stack([np.zeros((3, 4), np.float32), g[:, 0]], axis=1)
    assert _result(g2).spread(column=np.array([1, 1, 1]))["spread_rmse"] == pytest.approx(s["spread_rmse"], rel=1e-12)
    assert _result(g2).spread(column=0)["spread_rmse"] == 0.0


def test_equal_replicates_give_zero_spread():
    g = np.repeat(np.arange(6, dtype=np.float32).reshape(3, 2, 1), 4, axis=2)
    s = _result(g).spread(g_recorded=[0.0, 2.0, 4.0])
    assert s["spread_rmse"] == 0.0 and s["zero_variance"] == 1.0 and np.isnan(s["recorded_z2"])


def test_action_table_where_the_halves_disagree():
    # one state, three actions, four replicates (even-indexed: 0, 2; odd-indexed: 1, 3)
    #   action 0: a_W, always 1             action 1: 5 on the even half, -3 on the odd   action 2: always 2
    g = np.array([[[1, 1, 1, 1], [5, -3, 5, -3], [2, 2, 2, 2]]], np.float32)
    t = _result(g).action_table([0])
    assert t["greedy_agreement"] == 0.0
    assert t["gap"] == pytest.approx(1.0)                    # the means are 1, 1, 2: action 2 is best by 1
    assert t["gap_holdout"] == pytest.approx(-4.0)           # the even half picks action 1, whose odd half is -3: -3 - 1
    assert t["significant"] == 1.0                           # actions 2 and 0 have no variance: any gap > 0 is beyond 2 se
    assert list(t["per_state"]["best"]) == [2]
    # a_W the best action: agreement 1, gap 0, never significant
    t = _result(g).action_table([2])
    assert t["greedy_agreement"] == 1.0 and t["gap"] == 0.0 and t["significant"] == 0.0
    assert t["gap_holdout"] == pytest.approx(-5.0)           # picks action 1 again: -3 - 2
    # noise alone: the gap is biased upwards, the held-out gap is not
    rng = np.random.default_rng(5)
    t = _result(rng.standard_normal((4000, 5, 8))).action_table(np.zeros(4000, np.int64))
    assert t["gap"] > 0.3 and abs(t["gap_holdout"]) < 0.05
    # actions given by id: a_W is looked up among the state's columns
    t = _result(g, actions=[[4, 0, 3]]).action_table([3])
    assert t["greedy_agreement"] == 1.0 and list(t["per_state"]["best"]) == [3]
    with pytest.raises(ValueError, match="not among"):
        _result(g, actions=[[4, 0, 3]]).action_table([1])


def test_odd_replicates_are_refused():
    g = np.zeros((2, 5, 3), np.float32)
    with pytest.raises(ValueError, match="even"):
        _result(g).action_table([0, 0])
    with pytest.raises(ValueError, match="at least 2"):
        _result(np.zeros((2, 5, 1), np.float32)).spread()
    _result(g).spread()                                      # (the spread needs no halves)
