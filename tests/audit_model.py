"""SPEC §15's audited rollout on the host: tests/acting_emulator.py's Emulator with a begin pseudo-step whose choice may be forced
per env, and the two discounted-return accumulators. It never calls scg_rollout_audit: the plain steps are a backend's (the
oracle's, or the library's already-verified entry points), the rules are tests/option_rules.py's.

The begin pseudo-step. §4.2 (rules without BEST) offers min C, §14 (BEST) offers c*; §4.2's gate enters it where V_cand >= V_0.
§15 then replaces both the offer and the gate's result for an env whose force names a member of C. The model makes this choice
itself for every backend and both rule sets (a backend's own begin choice, where it makes one, is overwritten), so the tallies
of the begin pseudo-step are the model's, and so are the tallies of every later step without BEST, which the Emulator leaves to
its backend: `_count_42` derives them from §4.2.

The accumulators are numpy float32, one rounded product and one rounded sum per step, fed from the step views' reward and done.

The cases the GPU tests run are built here (`case`, `draw_force`) so that tests/test_audit_host.py can assert their non-vacuity
conditions on the oracle without a GPU."""
import numpy as np

import option_rules as rules
import skill_chaining_with_graphs_amd as scg
from acting_emulator import Emulator, OracleBackend
from util import HP, SCALE, SIBLING_PARENTS, crossing_weights, random_env_state, sibling_tree

F32 = np.float32
GUARD = F32(-777.25)                  # what the tests prefill every float audit array with
N, K, T0, N_OPT, MASK, REOFFER = 300, 12, 40, 5, 0b111110, 4
N_VF = N_OPT + 1
MAX_EP = 7                            # episodes end and restart inside a 12-step launch
CASE_HP = dict(HP, max_episode_steps=MAX_EP)
MAPS = ["pinball_simple", "pinball_empty"]
SEED = 3                              # the contexts' (the random numbers')
# the seeds of the weights, the states and the forces per map: chosen, as the non-vacuity conditions allow, so that every condition
# of tests/test_audit_host.py holds (a uniform force opposes a declining gate on 7 % of the envs on average, the bound is 10 %)
CASE_SEEDS = {"pinball_simple": (6, 9, 21), "pinball_empty": (6, 8, 21)}


def draw_force(n, seed):
    """One force per env from {0, +-1 .. +-5}, each of the eleven values equally likely."""
    return np.random.default_rng(seed).integers(-N_OPT, N_OPT + 1, n).astype(np.int8)


def case(name, n=N):
    """The inputs of one audited launch on map `name`: (map, parents, clf [6][8], W [6][5][1296], env state dict, force)."""
    w_seed, state_seed, force_seed = CASE_SEEDS[name]
    m = scg.load_map(name)
    parents, clf = sibling_tree(m)
    st = random_env_state(m, n, N_OPT, state_seed, id_lo=-N_OPT, id_hi=N_OPT, opt_steps_hi=10, max_episode_steps=MAX_EP)
    return m, parents, clf, crossing_weights(N_VF, w_seed), st, draw_force(n, force_seed)


def case_oracle(name, n=N, seed=SEED, gest=0, mask=MASK):
    import sc_oracle
    orc = sc_oracle.Oracle(scg.load_map(name), SCALE, n_envs=n, n_options=N_OPT, seed=seed, enabled_mask=mask, n_threads=8,
                           reoffer_period=REOFFER, **CASE_HP)
    orc.set_parents(SIBLING_PARENTS)
    if gest:
        orc.set_gestation(gest)
    return orc


class AuditModel(Emulator):
    """An Emulator whose begin pseudo-step is SPEC §15's. After run(): applied, cand, v_root, v_cand, disc_ret, disc_g,
    disc_final ([n]; v_cand and disc_final hold GUARD where the launch writes nothing), `episodes` ended per env, and
    `begin_info`, what the non-vacuity conditions read."""

    def __init__(self, *a, gamma=CASE_HP["gamma"], **kw):
        super().__init__(*a, **kw)
        self.gamma = F32(gamma)

    def seat(self, st):
        super().seat(st)
        n = self.n
        self.applied, self.cand = np.zeros(n, np.uint8), np.zeros(n, np.int8)
        self.v_root, self.v_cand = np.full(n, GUARD), np.full(n, GUARD)
        self.disc_ret, self.disc_g, self.disc_final = np.zeros(n, F32), np.ones(n, F32), np.full(n, GUARD)
        self.episodes = np.zeros(n, np.int64)

    def carry(self, disc_ret, disc_g):
        """Take the accumulators of an earlier launch (a launch without a begin goes on from them)."""
        self.disc_ret, self.disc_g = np.array(disc_ret, F32), np.array(disc_g, F32)

    # ------------------------------------------------------------------ the begin pseudo-step
    def begin(self, t, force=None, **flags):
        self.B.begin(t, **flags)
        st, n, idx = self.st, self.n, np.arange(self.n)
        C, Q, V = self._masks()
        minc = rules.min_c(C)
        if self.best:                                          # §14: c*
            ch = rules.choose(C, V, np.zeros(n, bool), np.full(n, 2), np.zeros(n, np.int64), t, self.gid, self.period)
            cand = ch["cstar"].copy()
        else:                                                  # §4.2: min C
            cand = minc.copy()
        with np.errstate(invalid="ignore"):
            gate = V[cand, idx] >= V[0]                        # §4.2's gate on the offered option (cand = 0: not read)
            declined = (cand >= 1) & ~gate
        f = np.zeros(n, np.int64) if force is None else np.asarray(force, np.int64)
        k = np.abs(f)
        in_range = (k >= 1) & (k < self.n_vf)
        applied = in_range & C[np.where(in_range, k, 0), idx]  # §15: |f| in C (C[0] is empty)
        with np.errstate(invalid="ignore"):
            own = V[np.where(applied, k, 0), idx] >= V[0]      # what the gate says of the forced option
        cand = np.where(applied, k, cand)
        declined = np.where(applied, f < 0, declined)
        offer = cand >= 1
        entered = offer & ~declined
        st["option_id"][:] = np.where(declined, -cand, cand).astype(np.int32)
        st["opt_steps"][:] = 0
        st["qcache"][:] = Q[np.where(entered, cand, 0), :, idx].T
        np.add.at(self.entries, (cand[entered], idx[entered]), 1)
        np.add.at(self.declines, (cand[declined], idx[declined]), 1)
        if self.best:
            ov = entered & (cand != minc)
            np.add.at(self.overrides, (cand[ov], idx[ov]), 1)
        self.applied, self.cand = applied.astype(np.uint8), cand.astype(np.int8)
        self.v_root = V[0].astype(F32)
        self.v_cand = np.where(offer, V[cand, idx], GUARD).astype(F32)
        self.disc_ret, self.disc_g = np.zeros(n, F32), np.ones(n, F32)
        self.begin_info = dict(
            against_decline=float((applied & (f > 0) & ~own).mean()),      # forced in where the gate would decline
            against_enter=float((applied & (f < 0) & own).mean()),        # forced out where the gate would enter
            not_lowest=float((applied & (f > 0) & (k != minc)).mean()),
            not_in_c=float(((f != 0) & ~applied).mean()))
        self._finish(np.zeros(n, bool))

    # ------------------------------------------------------------------ a real step
    def _count_42(self, t, keep, done, oid_in):
        """§4.2's entries and declines of a step without BEST (the Emulator tallies only §14's)."""
        C, _, V = self._masks()
        idx, minc = np.arange(self.n), rules.min_c(C)
        due = ((np.uint64(t) + self.gid) % np.uint64(self.period)) == 0
        stay = ~keep & (minc >= 1) & (done == 0) & (oid_in == -minc) & ~due
        offer = ~keep & (minc >= 1) & ~stay
        with np.errstate(invalid="ignore"):
            declined = offer & ~(V[minc, idx] >= V[0])
        entered = offer & ~declined
        np.add.at(self.entries, (minc[entered], idx[entered]), 1)
        np.add.at(self.declines, (minc[declined], idx[declined]), 1)

    def step(self, t):
        oid_in = self.st["option_id"].astype(np.int64)
        out = super().step(t)
        st = self.st
        done = st["done"].astype(np.int64)
        if not self.best:
            self._count_42(t, self.keep, done, oid_in)
        d = (self.disc_ret + (self.disc_g * st["reward"].astype(F32)).astype(F32)).astype(F32)
        g = (self.disc_g * self.gamma).astype(F32)
        end = done != 0
        self.disc_final = np.where(end, d, self.disc_final).astype(F32)
        self.disc_ret, self.disc_g = np.where(end, F32(0), d).astype(F32), np.where(end, F32(1), g).astype(F32)
        self.episodes += end
        return out

    def run(self, t0, K, force=None, **begin):
        t = t0
        if any(begin.values()):
            self.begin(t0, force=force, **begin)
            t += 1
        for j in range(K):
            self.step(t + j)

    def audit_arrays(self):
        return {f: getattr(self, f) for f in ("applied", "cand", "v_root", "v_cand", "disc_ret", "disc_g", "disc_final")}


def oracle_model(orc, st, W, clf, enabled, gest=0, **kw):
    """An AuditModel on the oracle with the oracle's own parents, re-offer period, env id base and gamma."""
    p = orc.p
    mod = AuditModel(OracleBackend(orc, W, clf, enabled), orc.n_vf, enabled, gest, [int(p.parents[k]) for k in range(8)],
                     int(p.reoffer_period), int(p.env_id_base), gamma=float(p.gamma), **kw)
    mod.seat(st)
    return mod
