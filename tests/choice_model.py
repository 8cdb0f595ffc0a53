"""SPEC §14 (value-ranked option choice) in numpy, from the oracle's primitives: the counterpart of interrupt_learning_model.py.

The oracle knows §4.2's lowest-numbered choice only, so a step of scg_rollout_select(BEST [| INTERRUPT]) is rebuilt round a plain
acting step:
  * `candidate_mask` is ilm.candidates generalised from its minimum to the whole set C;
  * `choose` is §14's rule on C, the maxima V_k (ilm.vmax of sco_q_values) and the env's bookkeeping: stay, offer, c*, the gate;
  * `Emulator` patches a plain step's outputs with it (and with §11's interruption, unchanged by §14). By §4.2 an env's physics,
    episode bookkeeping and `keep` do not depend on the choice, so only option_id, qcache and the interrupted envs' opt_steps of
    the plain step differ. `OracleEmulator` takes the plain step, Q and the membership bits from the oracle; the GPU tests
    subclass Emulator on already-verified entry points of the library.
`sibling_tree` is the layout the tests (and tools/choice_report.py's hand-set tree) use: five discs whose initiation sets overlap,
two of them leading to the goal, so that most states have several candidates."""
import numpy as np

import interrupt_learning_model as ilm
from util import disc_weights

NACT = 5
SIBLING_PARENTS = [0, 0, 0, 1, 1, 2]


def sibling_tree(m):
    """(parents, clf [6][8]) of the sibling layout on map `m`: options 1 and 2 lead to the goal, 3 and 4 into option 1, 5 into
    option 2; (tx, ty) the target, s = +-1 pointing from it towards the map centre."""
    tx, ty = float(m.target[0]), float(m.target[1])
    sx, sy = (1.0 if tx < 0.5 else -1.0), (1.0 if ty < 0.5 else -1.0)
    clf = np.zeros((6, 8), np.float32)
    for k, (cx, cy, r) in enumerate([(tx, ty, 0.30), (tx + 0.10 * sx, ty + 0.10 * sy, 0.35), (0.5, 0.5, 0.45), (tx, 0.5, 0.50),
                                     (0.5, 0.5, 0.75)], start=1):
        clf[k] = disc_weights(cx, cy, r)
    return list(SIBLING_PARENTS), clf


def candidate_mask(in_n, enabled, parents, n_vf):
    """§14's C from the membership bits in_n[k] of s_next (known options): C[k] = option k is enabled, s_next lies in its
    initiation set and outside its target region. bool [n_vf][n], row 0 False. Its lowest member is ilm.candidates."""
    n = in_n.shape[1]
    C = np.zeros((n_vf, n), bool)
    for k in range(1, n_vf):
        p = int(parents[k])
        ok = ((enabled >> k) & 1) == 1
        C[k] = in_n[k] & ok & ~(in_n[p] if p != 0 else np.zeros(n, bool))
    return C


def min_c(C):
    """The lowest member of C per env (0: none)."""
    c = np.zeros(C.shape[1], np.int64)
    for k in range(C.shape[0] - 1, 0, -1):
        c = np.where(C[k], k, c)
    return c


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
    o_keep = np.where((oid >= 1) & (oid < n_vf), oid, 0)
    new_id = np.where(keep, oid, np.where(stay, oid, np.where(offer, np.where(declined, -cstar, cstar), 0)))
    vf = np.where(keep, o_keep, np.where(entered, cstar, 0))
    return dict(stay=stay, offer=offer, minc=minc, cstar=cstar, declined=declined, override=entered & (cstar != minc),
                option_id=new_id, vf=vf)


class Emulator:
    """K steps of scg_rollout_select(BEST [| INTERRUPT]) from plain steps. A subclass supplies `plain_step(t)` (one plain acting
    step of self.st, a dict of host arrays, in place), `q_values(k)` (Q_k at self.st's state, [5][n]) and `predict(k)` (membership
    bits of self.st's position). Tallies: entries, declines, overrides, interrupts [n_vf][n]; `begin_stats` and `events` hold
    what the tests' non-vacuity conditions read."""

    def __init__(self, st, n_vf, enabled, gest, parents, reoffer_period, env_id_base=0, interrupt=False):
        self.st, self.n_vf, self.enabled, self.known = st, n_vf, enabled, enabled | gest
        self.parents, self.period, self.interrupt = [int(p) for p in parents], int(reoffer_period), interrupt
        self.n = len(st["x"])
        self.gid = np.arange(self.n, dtype=np.uint64) + np.uint64(env_id_base)
        z = lambda: np.zeros((n_vf, self.n), np.int64)
        self.entries, self.declines, self.overrides, self.interrupts = z(), z(), z(), z()
        self.events = dict(sibling_rescues=0, sibling_stays=0, offers=0, multi=0, kept=0, interrupted=0)
        self.begin_stats = None

    def _masks(self):
        in_n = np.zeros((self.n_vf, self.n), bool)
        for k in range(1, self.n_vf):
            if (self.known >> k) & 1:
                in_n[k] = self.predict(k) != 0
        Q = np.stack([self.q_values(k) for k in range(self.n_vf)])
        V = np.stack([ilm.vmax(Q[k]) for k in range(self.n_vf)])
        return candidate_mask(in_n, self.enabled, self.parents, self.n_vf), Q, V

    def _apply(self, t, keep, done, oid_in):
        """Patch self.st after a plain (pseudo-)step at counter t; returns (choice dict, interrupted mask)."""
        st, idx = self.st, np.arange(self.n)
        C, Q, V = self._masks()
        ch = choose(C, V, keep, done, oid_in, t, self.gid, self.period)
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
            o = np.where((oid_in >= 1) & (oid_in < self.n_vf), oid_in, 0)
            with np.errstate(invalid="ignore"):
                cut = keep & ~(V[o, idx] >= V[0])
            c = np.nonzero(cut)[0]
            st["option_id"][c] = (-ch["minc"][c]).astype(np.int32)
            st["opt_steps"][c] = 0
            st["qcache"][:, c] = Q[0][:, c]
            np.add.at(self.interrupts, (o[c], c), 1)
            self.events["kept"] += int(keep.sum())
            self.events["interrupted"] += len(c)
        return ch, cut, C

    def begin_at(self, t):
        """SPEC §10's BEGIN_AT pseudo-step at counter t: the state as given, a new episode, the first choice."""
        self.plain_begin(t)
        n = self.n
        ch, _, C = self._apply(t, np.zeros(n, bool), np.full(n, 2), np.zeros(n, np.int64))
        multi = C.sum(axis=0) >= 2
        self.begin_stats = dict(multi=float(multi.mean()), not_lowest=float((ch["cstar"] != ch["minc"])[multi].mean()) if multi.any() else 0.0)
        return ch, np.zeros(n, bool)

    def step(self, t):
        o_b, s_b = self.st["option_id"].astype(np.int64), self.st["opt_steps"].copy()
        self.plain_step(t)
        keep = (o_b >= 1) & (o_b < self.n_vf) & (self.st["opt_steps"] == s_b + 1)
        ch, cut, _ = self._apply(t, keep, self.st["done"].astype(np.int64), o_b)
        return ch, cut

    def run(self, t0, K, begin_at=True):
        t = t0
        if begin_at:
            self.begin_at(t0)
            t += 1
        for j in range(K):
            self.step(t + j)


class OracleEmulator(Emulator):
    """The emulator on the CPU oracle: sco_step (acting; parents, enabled and gestation set on `orc`), sco_q_values,
    sco_classifier_predict."""

    def __init__(self, orc, st, W, clf, enabled, gest=0, interrupt=False):
        p = orc.p
        super().__init__(st, orc.n_vf, enabled, gest, [int(p.parents[k]) for k in range(8)], int(p.reoffer_period),
                         int(p.env_id_base), interrupt)
        self.orc, self.W, self.clf = orc, np.ascontiguousarray(W, np.float32).reshape(orc.n_vf, NACT, -1), clf

    def _s(self):
        return [np.ascontiguousarray(self.st[f], np.float32) for f in ("x", "y", "vx", "vy")]

    def plain_begin(self, t):
        self.st["ep_steps"][:] = 0
        self.st["opt_steps"][:] = 0

    def plain_step(self, t):
        self.orc.step(self.st, self.W, self.clf, t, self.enabled)

    def q_values(self, k):
        return self.orc.q_values(*self._s(), self.W[k])

    def predict(self, k):
        s = self._s()
        return self.orc.classifier_predict(s[0], s[1], self.clf[k])
