"""The acting rules the oracle does not know, emulated round PLAIN acting steps: SPEC §11's interruption and §14's value-ranked
choice, one emulator for every test that needs either (the rules themselves are tests/option_rules.py's).

A plain acting step applies §4.2 whole. By §4.2 an env's physics, episode bookkeeping and `keep` do not depend on the choice made
at the step's end, so a step of scg_rollout_interrupt / scg_rollout_select differs from it only in option_id, qcache and the
interrupted envs' opt_steps. `Emulator` takes one plain step from a BACKEND and patches exactly those:
  * `interrupt` (§11): an env that keeps its option and fails V_o >= V_0 at s_next leaves it: id -min C, opt_steps 0, the root's Q;
  * `best` (§14): an env that does not keep its option chooses by option_rules.choose. With `best` off such an env keeps the plain
    step's own (§4.2) choice, unpatched;
  * both off: the plain step loop.
`v_option` says where V_o of a kept env is read: "q_values" (Q_o evaluated at s_next by the backend) or "qcache" (the plain step
left Q_o(s_next, .) in the env's qcache: the derivation the §11 tests have used from the start). Two derivations, kept apart on
purpose.

A backend is the plain step on one implementation: `OracleBackend` below (sco_step, sco_q_values, sco_classifier_predict,
sco_pinball_step) and gpu_util.GpuBackend (the library's verified entry points). Its interface:
  seat(st)            take the env state to run from;             st      the host view of that state (dict of numpy arrays)
  begin(t, **flags)   the begin pseudo-step at counter t;          step(t) one plain acting step; both refresh `st` and return it
  push()              make the emulator's patches of st["option_id" / "opt_steps" / "qcache"] the backend's state
  q_values(s, k)      Q_k at the states s = (x, y, vx, vy), [5][m];  predict(x, y, k)   option k's membership bits, bool [m]
  pinball(s, a)       (s', reward, goal) of one physics step;      row, len   the step's record row and lengths, or None
A step's view may also hold "succ_ctr", the successes-counter delta of the step ([n_vf][n]), where the backend counts."""
import numpy as np

import option_rules as rules
from skill_chaining_with_graphs_amd import _lib

STATE = ("x", "y", "vx", "vy")


class OracleBackend:
    """Plain acting steps on the CPU oracle (W never applied). Parents, enabled mask and gestation are the oracle's own."""
    row = len = None

    def __init__(self, orc, W, clf, enabled=None):
        self.orc, self.enabled = orc, enabled
        self.W = np.ascontiguousarray(W, np.float32).reshape(orc.n_vf, rules.NACT, -1)
        self.clf = np.ascontiguousarray(clf, np.float32).reshape(orc.n_vf, -1)

    def seat(self, st):
        self.st = st
        return st

    def begin(self, t, begin_at=True):
        """BEGIN_AT only: the state as given, a new episode. The oracle makes no first choice: that is §14's, by the emulator."""
        assert begin_at
        self.st["ep_steps"][:] = 0
        self.st["opt_steps"][:] = 0
        return self.st

    def step(self, t):
        args = () if self.enabled is None else (self.enabled,)
        self.orc.step(self.st, self.W, self.clf, t, *args)
        return self.st

    def push(self):
        pass                                                   # (st is the oracle's state itself)

    def q_values(self, s, k):
        return self.orc.q_values(*[np.ascontiguousarray(v, np.float32) for v in s], self.W[k])

    def predict(self, x, y, k):
        return self.orc.classifier_predict(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32), self.clf[k]) != 0

    def pinball(self, s, a):
        c = [np.array(v, np.float32, copy=True) for v in s]
        rew, goal = self.orc.pinball_step(*c, np.array(a, copy=True))
        return c, rew, goal


def oracle_emulator(orc, st, W, clf, enabled, gest=0, **kw):
    """An Emulator on the oracle with the oracle's own parents, re-offer period and env id base."""
    p = orc.p
    emu = Emulator(OracleBackend(orc, W, clf, enabled), orc.n_vf, enabled, gest, [int(p.parents[k]) for k in range(8)],
                   int(p.reoffer_period), int(p.env_id_base), **kw)
    emu.seat(st)
    return emu


class Emulator:
    """K (pseudo-)steps of an acting rollout with the rules `interrupt` (§11) and `best` (§14) from a backend's plain steps.
    Tallies, all [n_vf][n]: entries, declines, overrides (with `best`), interrupts (with `interrupt`). `kept` / `interrupted`
    count the envs that kept an option / were cut (`keep`: the last step's mask); `events` and `begin_stats` hold what the §14
    tests' non-vacuity conditions read; `rows` / `lens` the record row of every pseudo-step where the backend records (an interrupted env's row carries its
    new id and ROLLOUT_TERM_INTERRUPTED)."""

    def __init__(self, backend, n_vf, enabled, gest, parents, reoffer_period, env_id_base=0, interrupt=False, best=False,
                 v_option="q_values"):
        assert v_option in ("q_values", "qcache")
        self.B, self.n_vf, self.enabled, self.known = backend, n_vf, enabled, enabled | gest
        self.parents, self.period, self.base = [int(p) for p in parents], int(reoffer_period), env_id_base
        self.interrupt, self.best, self.v_option = interrupt, best, v_option
        self.kept = self.interrupted = 0
        self.events = dict(sibling_rescues=0, sibling_stays=0, offers=0, multi=0)
        self.begin_stats = None
        self.rows, self.lens = [], []

    @property
    def st(self):
        return self.B.st

    def seat(self, st):
        st = self.B.seat(st)
        self.n = len(st["x"])
        self.gid = np.arange(self.n, dtype=np.uint64) + np.uint64(self.base)
        z = lambda: np.zeros((self.n_vf, self.n), np.int64)
        self.entries, self.declines, self.overrides, self.interrupts = z(), z(), z(), z()

    def _masks(self):
        """(C, Q, V) at the state the step left: the candidate set, every value function's Q [n_vf][5][n] and its maxima."""
        st = self.st
        s = [st[f] for f in STATE]
        in_n = rules.membership(self.B.predict, s[0], s[1], self.n_vf, self.known)
        Q = np.stack([self.B.q_values(s, k) for k in range(self.n_vf)])
        V = np.stack([rules.vmax(Q[k]) for k in range(self.n_vf)])
        return rules.candidate_mask(in_n, self.enabled, self.parents, self.n_vf), Q, V

    def _apply(self, t, keep, done, oid_in):
        """Patch the state after a plain (pseudo-)step at counter t; returns (choice dict or None, interrupted mask, C)."""
        st, idx, ch = self.st, np.arange(self.n), None
        if not (self.best or self.interrupt):
            return None, np.zeros(self.n, bool), None
        C, Q, V = self._masks()
        if self.best:
            ch = rules.choose(C, V, keep, done, oid_in, t, self.gid, self.period)
            e = np.nonzero(~keep)[0]
            st["option_id"][e] = ch["option_id"][e].astype(np.int32)
            st["qcache"][:, e] = Q[ch["vf"][e], :, e].T
            entered = ch["offer"] & ~ch["declined"]
            np.add.at(self.entries, (ch["cstar"][entered], idx[entered]), 1)
            np.add.at(self.declines, (ch["cstar"][ch["declined"]], idx[ch["declined"]]), 1)
            np.add.at(self.overrides, (ch["cstar"][ch["override"]], idx[ch["override"]]), 1)
            with np.errstate(invalid="ignore"):
                self.events["sibling_rescues"] += int((ch["override"] & ~(V[ch["minc"], idx] >= V[0])).sum())
            self.events["sibling_stays"] += int((ch["stay"] & (-np.asarray(oid_in, np.int64) != ch["minc"])).sum())
            self.events["offers"] += int(ch["offer"].sum())
            self.events["multi"] += int((ch["offer"] & (C.sum(axis=0) >= 2)).sum())
        cut = np.zeros(self.n, bool)
        if self.interrupt:                                     # SPEC §11, unchanged by §14: -min C, the root's Q
            o = rules.vf_of(oid_in, self.n_vf)
            cut = rules.interrupted(keep, V, o, rules.vmax(st["qcache"]) if self.v_option == "qcache" else None)
            c = np.nonzero(cut)[0]
            st["option_id"][c] = (-rules.min_c(C)[c]).astype(np.int32)
            st["opt_steps"][c] = 0
            st["qcache"][:, c] = Q[0][:, c]
            np.add.at(self.interrupts, (o[c], c), 1)
            self.kept += int(keep.sum())
            self.interrupted += len(c)
        return ch, cut, C

    def _finish(self, cut):
        self.B.push()
        if self.B.row is not None:
            row = self.B.row
            row["option_id"] = self.st["option_id"].astype(np.int8)
            row["term"][cut] = _lib.ROLLOUT_TERM_INTERRUPTED
            self.rows.append(row)
            self.lens.append(self.B.len)

    def begin(self, t, **flags):
        """The begin pseudo-step at counter t (SPEC §8's BEGIN, §10's BEGIN_AT: the backend's flags). Nothing is kept, so §11
        has nothing to cut; with `best` the first choice is §14's."""
        self.B.begin(t, **flags)
        n = self.n
        cut = np.zeros(n, bool)
        if self.best:
            ch, cut, C = self._apply(t, np.zeros(n, bool), np.full(n, 2), np.zeros(n, np.int64))
            multi = C.sum(axis=0) >= 2
            self.begin_stats = dict(multi=float(multi.mean()),
                                    not_lowest=float((ch["cstar"] != ch["minc"])[multi].mean()) if multi.any() else 0.0)
        self._finish(cut)

    def step(self, t):
        o_b, s_b = self.st["option_id"].astype(np.int64), self.st["opt_steps"].copy()
        st = self.B.step(t)
        keep = self.keep = rules.kept_by_counters(o_b, s_b, st["opt_steps"], self.n_vf)
        ch, cut, _ = self._apply(t, keep, st["done"].astype(np.int64), o_b)
        self._finish(cut)
        return ch, cut

    def run(self, t0, K, **begin):
        """K steps from counter t0; with begin flags (begin=True / begin_at=True) a begin pseudo-step at t0 first, the steps
        from t0 + 1."""
        t = t0
        if any(begin.values()):
            self.begin(t0, **begin)
            t += 1
        for j in range(K):
            self.step(t + j)

    def record(self):
        """The rows a recorded launch of all these pseudo-steps holds: [rows][n] per field, and len."""
        return {f: np.stack([r[f] for r in self.rows]) for f in self.rows[0]}, np.sum(self.lens, axis=0)
