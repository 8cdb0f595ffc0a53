"""tests/option_rules.py against known answers written out env by env (no GPU, no oracle): the end of an option (SPEC §4.2, the
§9 / §10 term codes), `keep` read off the counters, §11's comparison and the small selectors. §14's `choose` and the candidate set
have theirs in tests/test_choice_host.py."""
import numpy as np

import option_rules as rules

NAN = np.float32("nan")
N_VF, PARENTS, MAX_OPT = 4, [0, 0, 1, 2], 10            # option 1 leads to the goal, 2 into 1, 3 into 2


def _end(o, in_sets, goal=0, done=0, steps=0, known=0b1110):
    """option_end for ONE env: in_sets the options whose initiation set holds s'."""
    in_p = np.zeros((N_VF, 1), bool)
    for k in in_sets:
        in_p[k] = True
    r = rules.option_end(in_p, np.array([goal]), np.array([done]), np.array([o]), np.array([steps]), PARENTS, known, MAX_OPT)
    return {k: v[0].item() for k, v in r.items()}


def test_option_end_one_env_per_term_code():
    r = _end(2, [2])                                           # still in its own set, not yet in the parent's: goes on
    assert r["keep"] and r["code"] == 0 and not (r["succ"] or r["fail"] or r["otime"] or r["term"]) and r["o"] == 2
    r = _end(2, [1, 2])                                        # 1 success: reached the parent's set
    assert r["succ"] and not r["fail"] and not r["keep"] and r["code"] == 1
    r = _end(1, [1], goal=1, done=1)                           # 1 success: parent 0 is the goal (success before the episode end)
    assert r["succ"] and r["code"] == 1 and not r["keep"]
    r = _end(1, [1, 2, 3], goal=0)                             # parent 0: no set counts, only the goal
    assert not r["succ"] and r["keep"]
    r = _end(2, [2], done=2)                                   # 2 episode end (time limit), in its set
    assert not r["succ"] and not r["fail"] and r["term"] and not r["keep"] and r["code"] == 2
    r = _end(2, [3])                                           # 3 left its own set
    assert r["fail"] and not r["succ"] and not r["keep"] and r["code"] == 3
    r = _end(2, [3], done=2)                                   # the episode end goes before the failure
    assert r["fail"] and r["code"] == 2
    r = _end(2, [2], steps=MAX_OPT - 1)                        # 4 time-out: the last allowed step
    assert r["otime"] and not r["keep"] and r["code"] == 4 and not (r["succ"] or r["fail"])
    r = _end(2, [2], steps=MAX_OPT - 2)                        # ... and the one before it
    assert not r["otime"] and r["keep"] and r["code"] == 0
    r = _end(2, [1, 2], steps=MAX_OPT - 1, done=2)             # success goes before everything
    assert r["code"] == 1 and r["outcome"] == 1


def test_option_end_unknown_parent_and_ids_out_of_range():
    r = _end(2, [1, 2], known=0b1100)                          # the parent is not known: its bit gives no success
    assert not r["succ"] and r["keep"] and r["code"] == 0
    r = _end(2, [1], known=0b1100)                             # ... and leaving the own set is still a failure
    assert r["fail"] and r["code"] == 3
    for oid in (0, -2, N_VF, -N_VF, 9, -9, 2 ** 31 - 1, -2 ** 31):   # no option runs: the root, no code, nothing kept
        r = _end(oid, [1, 2, 3], steps=MAX_OPT)
        assert r["o"] == 0 and not r["keep"] and r["code"] == 0, oid
    r = _end(N_VF - 1, [3])                                    # the last option is one
    assert r["o"] == 3 and r["keep"]


def test_option_end_is_per_env():
    """A batch of every case above at once equals the cases one by one."""
    rng = np.random.default_rng(5)
    n = 300
    in_p = rng.random((N_VF, n)) < 0.5
    in_p[0] = False
    goal, done = rng.integers(0, 2, n), rng.choice([0, 0, 1, 2], n)
    oid, steps = rng.integers(-N_VF - 1, N_VF + 2, n), rng.choice([0, 3, MAX_OPT - 2, MAX_OPT - 1, MAX_OPT], n)
    got = rules.option_end(in_p, goal, done, oid, steps, PARENTS, 0b0110, MAX_OPT)
    for i in range(n):
        one = _end(int(oid[i]), [k for k in range(N_VF) if in_p[k, i]], int(goal[i]), int(done[i]), int(steps[i]), known=0b0110)
        assert all(got[f][i] == one[f] for f in one), i
    assert set(got["code"].tolist()) == {0, 1, 2, 3, 4}


def test_kept_by_counters():
    #               runs 2, +1   runs 2, reset   runs 2, unchanged   id 0   stays out (-2)   beyond the options   the last option
    o = np.array([2,           2,              2,                  0,     -2,              N_VF,                N_VF - 1])
    before = np.array([3,      3,              3,                  0,     0,               5,                   0])
    after = np.array([4,       0,              3,                  1,     1,               6,                   1])
    assert rules.kept_by_counters(o, before, after, N_VF).tolist() == [True, False, False, False, False, False, True]
    assert rules.kept_by_counters(np.array([1], np.int32), np.array([2 ** 31 - 2], np.int32), np.array([2 ** 31 - 1], np.int32),
                                  N_VF).tolist() == [True]


def test_interrupted_ties_and_nans():
    V = np.array([[1.0, 1.0, 1.0, NAN, 1.0, 1.0],              # V_0
                  [2.0, 1.0, 0.5, 1.0, NAN, 0.5],              # V_1
                  [9.0, 9.0, 9.0, 9.0, 9.0, 9.0]], np.float32)
    o = np.ones(6, np.int64)
    keep = np.array([True, True, True, True, True, False])
    assert rules.interrupted(keep, V, o).tolist() == [False, False, True, True, True, False]    # a tie holds; a NaN cuts
    v_o = np.array([0.0, 0.0, 3.0, 3.0, 3.0, 3.0], np.float32)                                  # (the qcache reading replaces V[o])
    assert rules.interrupted(keep, V, o, v_o).tolist() == [True, True, False, True, False, False]


def test_vf_of_vmax_and_membership():
    assert rules.vf_of(np.array([-5, -1, 0, 1, 3, 4, 77], np.int32), 4).tolist() == [0, 0, 0, 1, 3, 0, 0]
    q = np.array([[1.0, NAN, NAN], [3.0, 2.0, NAN], [2.0, NAN, NAN], [0.0, 1.0, NAN], [-1.0, NAN, NAN]], np.float32)
    m = rules.vmax(q)
    assert m[:2].tolist() == [3.0, 2.0] and np.isnan(m[2])     # maxNum: a NaN loses to a number
    calls = []
    bits = rules.membership(lambda x, y, k: (calls.append(k), np.full(len(x), k, np.uint8))[1], np.zeros(3), np.zeros(3), 4, 0b1010)
    assert calls == [1, 3] and bits.tolist() == [[False] * 3, [True] * 3, [False] * 3, [True] * 3]   # no bit for an unknown option
