"""The option rules of the SPEC on the host, each ONE time, in pure numpy (no oracle, no torch, no device).

The host models of the acting tests (tests/acting_emulator.py, tests/interrupt_learning_model.py, the step-loop models of the
§8 / §9 / §10 tests) and the reporting tools take every rule from here; the float64 / exact models (ref64.py, phys64.py,
collect_model.py and their tests) do NOT: they are independent derivations and keep their own spelling.

Conventions. Arrays over envs have length n. `option_id` is an env's id as the state holds it (k: running option k, -k: staying
out of option k, 0: none; any int32 may occur). Membership bits are bool [n_vf][n] with row 0 False and no bit for an option
that is not KNOWN (known = enabled | gestating): an unknown parent therefore gives no success and an unknown option is never a
candidate. `parents[k]` is option k's parent (0: the goal)."""
import numpy as np

NACT = 5


def vf_of(option_id, n_vf):
    """SPEC §4.2: the value function an id names: k for a running option 1 <= k < n_vf, the root (0) for every other id."""
    o = np.asarray(option_id, np.int64)
    return np.where((o >= 1) & (o < n_vf), o, 0)


def vmax(q):
    """SPEC §5: max over actions in the kernel's order (IEEE maxNum, a = 0 first); q [5][m]."""
    m = q[0].copy()
    for a in range(1, q.shape[0]):
        m = np.fmax(m, q[a])
    return m


def membership(predict, x, y, n_vf, known):
    """SPEC §4.2's membership bits of the positions (x, y): out[k] = predict(x, y, k) != 0 for the known options, False for the
    others and for row 0. `predict(x, y, k)` is the classifier of option k on a backend (the oracle's, the library's)."""
    out = np.zeros((n_vf, len(x)), bool)
    for k in range(1, n_vf):
        if (known >> k) & 1:
            out[k] = np.asarray(predict(x, y, k)) != 0
    return out


def candidate_mask(in_n, enabled, parents, n_vf):
    """SPEC §4.2 / §14's candidate set C at s_next from its membership bits in_n: C[k] = option k is enabled, s_next lies in
    its initiation set and outside its target region (its parent's set; the goal's region ends the episode instead)."""
    n = in_n.shape[1]
    C = np.zeros((n_vf, n), bool)
    for k in range(1, n_vf):
        p = int(parents[k])
        ok = ((enabled >> k) & 1) == 1
        C[k] = in_n[k] & ok & ~(in_n[p] if p != 0 else np.zeros(n, bool))
    return C


def min_c(C):
    """The lowest member of C per env (0: none): §4.2's choice."""
    c = np.zeros(C.shape[1], np.int64)
    for k in range(C.shape[0] - 1, 0, -1):
        c = np.where(C[k], k, c)
    return c


def candidates(in_n, enabled, parents, n_vf):
    """SPEC §4.2's selection at s_next: the smallest enabled option whose initiation set holds s_next and whose target region
    does not (0: none)."""
    return min_c(candidate_mask(in_n, enabled, parents, n_vf))


def option_end(in_p, goal, done, option_id, opt_steps, parents, known, max_option_steps):
    """SPEC §4.2's end of an option, for one step of every env. in_p: membership bits of s' (before a reset) [n_vf][n]; goal:
    s' reached the goal; done: §1.4's episode end code; option_id, opt_steps: the env's id and option-step counter at the step's
    ENTRY. Returns a dict of [n] arrays:
      o      the value function the step ran (vf_of);
      succ   s' lies in the target region of o: the parent's initiation set, or the goal for parent 0 (an unknown parent: never);
      fail   not succ, and s' left o's own initiation set;
      otime  this was the option's last allowed step;
      term   done, succ, fail or otime;    keep   o >= 1 and not term: the option goes on;
      code   SPEC §9 / §10's term code: 1 success, 2 episode end, 3 left the set, 4 time-out (in that priority); 0 where no
             option ran or it goes on. `outcome` is the same code without that mask (a trial's outcome, read where it ended).
    For o = 0 succ, fail and term are computed like any other row and mean nothing."""
    n_vf, n = in_p.shape
    idx = np.arange(n)
    o = vf_of(option_id, n_vf)
    par = np.asarray([int(p) for p in parents], np.int64)[o]
    par_known = ((known >> par) & 1) == 1
    succ = np.where(par == 0, np.asarray(goal) != 0, in_p[par, idx] & par_known)
    fail = ~succ & ~in_p[o, idx]
    otime = np.asarray(opt_steps, np.int64) + 1 >= max_option_steps
    ended = np.asarray(done) != 0
    term = ended | succ | fail | otime
    keep = (o >= 1) & ~term
    outcome = np.where(succ, 1, np.where(ended, 2, np.where(fail, 3, 4)))
    return dict(o=o, succ=succ, fail=fail, otime=otime, term=term, keep=keep, outcome=outcome,
                code=np.where((o >= 1) & ~keep, outcome, 0))


def kept_by_counters(o_before, opt_steps_before, opt_steps_after, n_vf):
    """`keep` read off an acting step's outputs instead of derived from the physics: the env ran an option and its option-step
    counter went up by one (every end of an option, and every env not stepped, leaves it at 0 or unchanged)."""
    o = np.asarray(o_before, np.int64)
    return (o >= 1) & (o < n_vf) & (np.asarray(opt_steps_after, np.int64) == np.asarray(opt_steps_before, np.int64) + 1)


def interrupted(keep, V, o, v_o=None):
    """SPEC §11: a kept option is interrupted unless V_o(s_next) >= V_0(s_next) (a NaN on either side interrupts). V [n_vf][n]
    the action maxima at s_next; o the value function per env; v_o, where given, replaces V[o] (the option's qcache reading)."""
    v_o = V[o, np.arange(len(o))] if v_o is None else v_o
    with np.errstate(invalid="ignore"):
        return np.asarray(keep, bool) & ~(v_o >= V[0])


def choose(C, V, keep, done, option_id, t, gid, reoffer_period):
    """SPEC §14 for the envs of one (pseudo-)step. C bool [n_vf][n]; V float32 [n_vf][n] = max_a Q_k(s_next, a) (read only where
    C holds, and row 0); keep: the env's option goes on (no choice is made); done: §1.4's episode end code of the step; option_id:
    the id at the step's entry (the begin pseudo-step: 0); t: the step's counter; gid: the global env ids. Returns a dict of [n]
    arrays: stay, offer, minc, cstar (offered envs: c*; else 0), declined, override, option_id (the id after the step: of a
    keeping env its entry id) and vf (the value function whose Q(s_next, .) is the env's qcache afterwards)."""
    n_vf, n = C.shape
    idx = np.arange(n)
    oid = np.asarray(option_id, np.int64)
    keep = np.asarray(keep, bool)
    anyc = C[1:].any(axis=0)
    neg = np.clip(-oid, 0, n_vf - 1)
    member = (oid < 0) & (-oid < n_vf) & C[neg, idx]
    due = ((np.uint64(t) + np.asarray(gid, np.uint64)) % np.uint64(reoffer_period)) == 0
    stay = ~keep & anyc & (np.asarray(done) == 0) & member & ~due
    offer = ~keep & anyc & ~stay
    minc = min_c(C)
    cs = np.zeros(n, np.int64)
    vbest = np.zeros(n, np.float32)
    for k in range(1, n_vf):                                   # ascending: a tie stays with the lower k; a NaN never wins
        better = C[k] & ~np.isnan(V[k]) & ((cs == 0) | (V[k] > vbest))
        cs = np.where(better, k, cs)
        vbest = np.where(better, V[k], vbest)
    cs = np.where(cs == 0, minc, cs)                           # every candidate's value a NaN: min C
    cstar = np.where(offer, cs, 0)
    with np.errstate(invalid="ignore"):
        declined = offer & ~(V[cstar, idx] >= V[0])
    entered = offer & ~declined
    new_id = np.where(keep, oid, np.where(stay, oid, np.where(offer, np.where(declined, -cstar, cstar), 0)))
    vf = np.where(keep, vf_of(oid, n_vf), np.where(entered, cstar, 0))
    return dict(stay=stay, offer=offer, minc=minc, cstar=cstar, declined=declined, override=entered & (cstar != minc),
                option_id=new_id, vf=vf)


def sort_keys(option_id, n_vf):
    """SPEC §5's sort key of an env: the option it runs (1 .. n_vf - 1), 0 for the root, n_vf for an id beyond the options."""
    o = np.asarray(option_id, np.int64)
    return np.where(o <= 0, np.where(o > -n_vf, 0, n_vf), np.where(o < n_vf, o, n_vf))


def env_order(option_id, n_vf, block_envs):
    """SPEC §5's env order: perm[position] = env, for the option ids at entry."""
    key = sort_keys(option_id, n_vf)
    n = len(key)
    lst = [np.nonzero(key == k)[0] for k in range(7)]
    tot = [len(v) for v in lst]
    S, R, Bf = sum(tot[1:]), sum(1 for v in tot[1:] if v > 0), n // block_envs
    c = block_envs if (Bf <= R or S == 0) else min(block_envs, -(-S // (Bf - R)))
    U = sum(-(-v // c) for v in tot[1:])
    perm, fill = [], 0
    if U * block_envs <= n:                                        # chunked
        for k in range(1, 7):
            for r in range(0, tot[k], c):
                m = min(c, tot[k] - r)
                perm += list(lst[k][r:r + m])
                perm += list(lst[0][fill:fill + block_envs - m])
                fill += block_envs - m
    else:                                                          # padded
        for k in range(1, 7):
            perm += list(lst[k])
            if tot[k] > 0:
                pad = min((-len(perm)) % block_envs, tot[0] - fill)
                perm += list(lst[0][fill:fill + pad])
                fill += pad
    perm += list(lst[0][fill:])
    assert sorted(perm) == list(range(n))
    return np.array(perm, np.int64)
