"""A plain float64 model of one step-batch (SPEC §2, §4, §5, §7), written from the SPEC and not from the oracle or the kernel.

It has no blocks, no env order and no summation order: every sum is the sum the SPEC means, taken in float64. Its answers are
compared with a binary32 implementation (the CPU oracle or the HIP path) to a tolerance that is derived per element from sums
of absolute values (constants below), so that it checks WHAT is summed — which env is an update item of which value function,
with which target — and not how.

Borrowed piece: the physics (SPEC §1.3). `s'`, the reward and the goal flag come from the oracle's `pinball_step` on the
pre-state and the model's own action, so that the rest of the step follows the binary32 physics exactly. The borrowed
physics is checked: on every env that the float64 physics model (tests/phys64.py) does not call ambiguous, `s'` agrees
with it to its tolerance and the reward and the goal flag exactly.

Everything else is computed here: Philox4x32-10 in vectorised numpy (pinned by the published vectors), the action, the episode
bookkeeping, the classifier (float64 quadratic), the option logic, the value gate, the update items and their targets, the
gradient sums G64, n_k, qcache, W_next, events and gest_succ.

Ambiguity. A binary32 decision can differ from the float64 one where the float64 value lies within the error bound of the
binary32 evaluation: a classifier `|z| <= tol_z` or a gate `|V_k - V_0| <= tol_V`. Such an env is AMBIGUOUS: the model takes the
decision the system under test made (where it can be read off the outputs) and carries on from it; it reports the env. When
`W_k` and `W_0` are bitwise identical the tie is exact (both sides evaluate the same sum in the same order) and the env enters.

Interruption (SPEC §11 acting, §12 learning), `step(..., interrupt=True)`: an env whose option o goes on is interrupted when
`!(V_o >= V_0)` at s_next. It is ambiguous where `|V_o - V_0| <= tol_V_o + tol_V_0` and W_o, W_0 are not bitwise equal; the model
then takes the SUT's decision (a kept env whose written id is not o, or whose opt_steps is 0, was interrupted). Equal weights
tie exactly and keep the option; a NaN on either side interrupts. An interrupted env's candidate c follows the SUT where a
membership at s_next is ambiguous, as the selection does.
"""
from __future__ import annotations

import numpy as np

import phys64
from util import fourier_reference

NACT, NF = 5, 1296
U32 = 2.0 ** -24                      # unit roundoff of binary32

# ---- error-bound constants (binary32 evaluation against the exact value)
# features: |phi32 - cos| <= C_PHI. sincospi is accurate to 3e-7 (test_oracle_primitives); AB / CD are products of up to
# 10 unit complex numbers (each cmul two roundings); phi is one more fma: <= ~24 roundings of unit-size values.
C_PHI = 32 * U32
# Q = sum_f w_f phi_f in the factorised form of SPEC §3.1 (an fma chain of 36 + 9 + 3 = 48 terms deep). Every rounding is
# relative to a partial sum, bounded by sum |w| |AB| |CD| <= 2 sum |w| (the re.re and im.im halves separately).
#   tol_Q = C_PHI * sum|w|  +  C_Q * sum|w| (|Re AB Re CD| + |Im AB Im CD|)
C_Q = 48 * U32
# classifier: 6 fmas + 3 products + the two fma(x, 2, -1), all of values bounded by the terms: tol_z = C_Z sum_j |w_j| (|psi_j| + U)
C_Z = 12 * U32
# G = sum_i delta_i phi_i: a per-block fma chain over the block's items of one action (two fmas per item, up to 2 * 256
# deep), then 16-block segments and the segment chain. Rounding errors of such chains are unbiased in practice; the bound used
# is the probabilistic one of Higham & Mary (2019) with lambda = 8: C_G sqrt(L) U sum_i |delta_i| (|Re AB Re CD| + |Im AB Im CD|)
C_G = 8.0
L_BLOCK = 2 * 256 + 16
# ---- absolute terms: below 2^-126 a binary32 rounding is no longer relative to the value but at most half a unit of the
# subnormal grid, 2^-150. A tolerance that has to hold for subnormal results adds that once per rounding of the chain.
SUB = 2.0 ** -150
# Q of SPEC §3.1: per (c12, part) a chain of 36 fmas (2 * 36 * 36), the 2 * 36 fmas over c12, 4 + 2 + 1 adds
N_Q = 2 * 36 * 36 + 2 * 36 + 7
Q_FLOOR = N_Q * SUB
# sigmoid of SPEC §6 against the exact logistic of the clamped argument, RELATIVE to the value: the two-step reduction of a
# leaves r with one rounding of a value below 0.35 (n * LN2HI is exact), the degree-7 polynomial truncates exp(r) by
# 0.35^8 / 8! < 0.1 U and rounds 7 times at values between 0.7 and 1.5, the scaling by 2^n is exact (n >= -126 and
# p >= 1: e stays normal), then 1 + e and the division: under 12 roundings. z >= 0 gives 1/(1+e), relative to a value >= 1/2.
C_SIG = 16 * U32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """SPEC §2, vectorised: uint32 numpy arrays in, (u0, u1, u2, u3) out."""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, np.uint64) & M for v in (c0, c1, c2, c3)]
    k0 = np.uint64(k0) & M
    k1 = np.uint64(k1) & M
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return [v.astype(np.uint64) for v in c]


def mulhi32(a, b):
    return ((np.asarray(a, np.uint64) * np.uint64(b)) >> np.uint64(32)).astype(np.int64)


def _half_products(x, y, vx, vy):
    """|Re AB Re CD| + |Im AB Im CD| per (state, feature) in float64: the magnitudes the factorised sums of SPEC §3.1 / §5
    round against (AB = exp(i pi (c1 x + c2 y)), CD = exp(i pi (c3 vx^ + c4 vy^)))."""
    s = np.stack([x, y, np.asarray(vx, np.float64) * 0.25 + 0.5, np.asarray(vy, np.float64) * 0.25 + 0.5], 1).astype(np.float64)
    c = np.arange(6, dtype=np.float64)
    t12 = np.pi * (s[:, 0, None, None] * c[None, :, None] + s[:, 1, None, None] * c[None, None, :]).reshape(len(s), 36)
    t34 = np.pi * (s[:, 2, None, None] * c[None, :, None] + s[:, 3, None, None] * c[None, None, :]).reshape(len(s), 36)
    h = np.abs(np.cos(t12))[:, :, None] * np.abs(np.cos(t34))[:, None, :] + \
        np.abs(np.sin(t12))[:, :, None] * np.abs(np.sin(t34))[:, None, :]
    return h.reshape(len(s), NF)


def q_model(x, y, vx, vy, Wk, tables=None):
    """float64 Q_k(s, a) [n, 5] and its binary32 error bound [n, 5] (SPEC §3.1). tables: (phi, half products) of the states."""
    phi, h = tables if tables is not None else (fourier_reference(x, y, vx, vy), _half_products(x, y, vx, vy))
    W = np.asarray(Wk, np.float64).reshape(NACT, NF)
    aW = np.abs(W)
    aW = np.where(np.isfinite(aW), aW, 0.0)
    q = phi @ W.T
    tol = C_PHI * aW.sum(1)[None, :] + C_Q * (h @ aW.T)
    return q, tol


def clf_model(w8, x, y):
    """float64 classifier value z (SPEC §4.1) and its binary32 error bound."""
    w = np.asarray(w8, np.float64)[:6]
    u = 2.0 * np.asarray(x, np.float64) - 1.0
    v = 2.0 * np.asarray(y, np.float64) - 1.0
    psi = np.stack([np.ones_like(u), u, v, u * u, u * v, v * v], 1)
    return psi @ w, C_Z * ((np.abs(psi) + U32) @ np.abs(w))


class StepModel:
    """Hyper-parameters and map of one configuration; `step()` models one step-batch."""

    def __init__(self, orc, pmap, n_options, *, seed, env_id_base, gamma, alpha, epsilon, r_option_success,
                 max_episode_steps, max_option_steps, update_count_floor=0, reoffer_period=4, parents=None, scale=None):
        self.orc, self.map = orc, pmap
        self.n_options, self.n_vf = n_options, n_options + 1
        self.seed, self.env_id_base = int(seed), int(env_id_base)
        self.gamma, self.alpha = float(np.float32(gamma)), float(np.float32(alpha))
        self.epsilon, self.r_succ = float(np.float32(epsilon)), float(np.float32(r_option_success))
        self.max_ep, self.max_opt = int(max_episode_steps), int(max_option_steps)
        self.floor, self.period = int(update_count_floor), int(reoffer_period)
        self.parents = np.zeros(8, int)
        self.parents[1:] = np.arange(0, 7)                 # the default chain k -> k - 1
        if parents is not None:
            for k in range(1, self.n_vf):
                self.parents[k] = int(parents[k])
        self.scale = np.asarray(scale, np.float64)

    # ------------------------------------------------------------------ SPEC §2, §4.3
    def act(self, st, t):
        n = len(st["x"])
        t = int(t) % 2 ** 64                                  # Python ints: a 64-bit counter or id does not fit float64 or int64
        g = np.array([(self.env_id_base + e) % 2 ** 32 for e in range(n)], np.uint64)      # c0 = g mod 2^32 (two's complement)
        u0, u1, u2, _ = philox4x32_10(g, np.full(n, t & 0xFFFFFFFF, np.uint64), np.full(n, t >> 32, np.uint64),
                                      np.zeros(n, np.uint64), self.seed & 0xFFFFFFFF, self.seed >> 32)
        explore = (u0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 < self.epsilon
        a_rand = mulhi32(u1, 5)
        q = st["qcache"]
        best, a_greedy = q[0].copy(), np.zeros(n, np.int64)
        for a in range(1, NACT):                              # first maximum wins (a NaN is never a maximum)
            up = q[a] > best
            best = np.where(up, q[a], best)
            a_greedy = np.where(up, a, a_greedy)
        return np.where(explore, a_rand, a_greedy), mulhi32(u2, len(self.map.starts))

    # ------------------------------------------------------------------ the step-batch
    def step(self, pre, W, clf, t, enabled, gest=0, sut=None, learn=True, interrupt=False):
        """pre: the pre-step state dict (numpy, not modified). W [n_vf, 5, 1296] f32, clf [n_vf, 8]. sut: the outputs of the
        system under test (state dict after its step + 'events'), used only to follow it on ambiguous decisions.
        learn=False: the acting outputs only (SPEC §8's acting step); G, n_k, W and their tolerances are None.
        interrupt: an option that goes on is interrupted where the root's value at s_next is higher (SPEC §11 acting, §12 with
        learn). Returns a dict of model outputs, tolerances, resolutions and the ambiguous envs."""
        n, nvf, gam = len(pre["x"]), self.n_vf, self.gamma
        ar = np.arange(n)
        known = enabled | gest
        a, si = self.act(pre, t)
        s = [pre[k].astype(np.float32).copy() for k in ("x", "y", "vx", "vy")]
        sp = [v.copy() for v in s]
        reward, goal = self.orc.pinball_step(*sp, a.astype(np.uint8))          # the borrowed physics: s', reward, goal
        phys64.compare(phys64.step(self.map, *s, a), *sp, reward, goal, msg="borrowed physics against tests/phys64.py:")
        reward = reward.astype(np.float64)
        goal = goal.astype(bool)
        eps1 = pre["ep_steps"].astype(np.int64) + 1
        timeout = ~goal & (eps1 >= self.max_ep)
        done = np.where(goal, 1, np.where(timeout, 2, 0))
        starts = np.asarray(self.map.starts, np.float32)
        sn = [np.where(done != 0, starts[si, 0], sp[0]), np.where(done != 0, starts[si, 1], sp[1]),
              np.where(done != 0, 0.0, sp[2]).astype(np.float32), np.where(done != 0, 0.0, sp[3]).astype(np.float32)]
        amb = np.zeros(n, bool)

        def member(pts):
            """in_k for every option k [n_vf, n] (row 0 unused) and the ambiguity of each decision."""
            inn = np.zeros((nvf, n), bool)
            am = np.zeros((nvf, n), bool)
            for k in range(1, nvf):
                if (known >> k) & 1:
                    z, tz = clf_model(clf[k], pts[0], pts[1])
                    inn[k] = z > 0
                    am[k] = np.abs(z) <= tz
            return inn, am

        inA, amA = member(sp)            # in_k(s')
        inB, amB = member(sn)            # in_k(s_next)
        inS, amS = member(s)             # in_k(s)  (gestating options only)
        for k in range(1, nvf):
            if not (gest >> k) & 1:
                inS[k] = False
                amS[k] = False
        # follow the system under test where its outputs show its decision
        if sut is not None and "events" in sut:
            ev = sut["events"].astype(np.int64)
            rows = amA.any(0)
            for k in range(1, nvf):
                inA[k, rows] = ((ev[rows] >> k) & 1).astype(bool)
        amb |= amA.any(0)
        if learn:                        # in_k(s) only makes gestation items
            amb |= amS.any(0)

        # ---- SPEC §4.2: the env's own option, termination, selection
        oid = pre["option_id"].astype(np.int64)
        o = np.where((oid >= 1) & (oid < nvf), oid, 0)        # an id outside (-n_vf, n_vf) names no option: the env runs the root
        par_o = self.parents[np.clip(o, 0, 7)]
        succ_o = np.where(par_o == 0, goal, inA[np.clip(par_o, 0, nvf - 1), np.arange(n)])
        fail_o = ~succ_o & ~inA[o, np.arange(n)]
        otime = pre["opt_steps"].astype(np.int64) + 1 >= self.max_opt
        term = (done != 0) | succ_o | fail_o | otime
        running = o >= 1
        keep = running & ~term
        r_o = reward + np.where(succ_o, self.r_succ, 0.0)
        cont_o = np.where(term, 0.0, gam)
        exit_o = running & term & (done == 0)

        free = np.zeros(n, np.int64)                          # the candidate as if the env's option had ended (SPEC §11's c)
        for k in range(nvf - 1, 0, -1):                       # the lowest-numbered qualifying option wins
            if not (enabled >> k) & 1:
                continue
            pk = self.parents[k]
            tgt = inB[pk] if pk != 0 else np.zeros(n, bool)
            free = np.where(inB[k] & ~tgt, k, free)
        cand = np.where(keep, o, free)
        amb_b = ~keep & amB.any(0)
        if sut is not None:
            cand = np.where(amb_b, np.abs(sut["option_id"].astype(np.int64)), cand)
        amb |= amb_b
        # (t + g) mod 2^64 in Python ints (t = 2^64 - 1 overflows int64), g the 64-bit two's complement of env_id_base + e
        tg = [(int(t) + self.env_id_base + e) % 2 ** 64 for e in range(n)]
        stagger = np.array([v % max(self.period, 1) != 0 for v in tg], bool)          # §4.2: a period of 0 means 1
        stay = ~keep & (cand >= 1) & (done == 0) & (oid == -cand) & stagger
        entering = ~keep & (cand >= 1) & ~stay

        # ---- values at s_next (frozen W) and the gate
        qn, qn_tol = [], []
        tab_n = (fourier_reference(*sn), _half_products(*sn))
        for k in range(nvf):
            q, tq = q_model(*sn, W[k], tab_n)
            qn.append(q); qn_tol.append(tq)
        V = np.stack([np.fmax.reduce(q, axis=1) for q in qn])  # SPEC §5's max is IEEE maxNum: a NaN is passed over, V is NaN only
        V_tol = np.stack([tq.max(1) for tq in qn_tol])
        ci = np.clip(cand, 0, nvf - 1)
        Vc, V0 = V[ci, np.arange(n)], V[0]
        same = np.array([np.array_equal(W[k].view(np.uint32), W[0].view(np.uint32)) for k in range(nvf)])
        exact_tie = same[ci]
        accept = Vc >= V0                                      # NaN on either side: False (declines)
        gate_amb = entering & ~exact_tie & np.isfinite(Vc) & np.isfinite(V0) & (np.abs(Vc - V0) <= V_tol[ci, np.arange(n)] + V_tol[0])
        accept = np.where(entering & exact_tie & ~np.isnan(Vc), True, accept)
        if sut is not None:
            accept = np.where(gate_amb, sut["option_id"].astype(np.int64) > 0, accept)
        amb |= gate_amb
        declined = entering & ~accept

        # ---- SPEC §11 / §12: an option that goes on is interrupted where the root's value at s_next is higher
        interrupted, c = np.zeros(n, bool), np.zeros(n, np.int64)
        if interrupt:
            m_o, m_0 = V[o, ar], V[0]
            nan = np.isnan(m_o) | np.isnan(m_0)
            tie = same[o] & ~nan                               # bitwise-equal weights: an exact tie, which keeps the option
            interrupted = keep & ~tie & ~(m_o >= m_0)          # a NaN on either side interrupts
            amb_i = keep & ~tie & ~nan & (np.abs(m_o - m_0) <= V_tol[o, ar] + V_tol[0])
            if sut is not None:                                # the SUT interrupted where it wrote an id other than o, or opt_steps 0
                cut = (sut["option_id"].astype(np.int64) != o) | (sut["opt_steps"].astype(np.int64) == 0)
                interrupted = np.where(amb_i, cut, interrupted)
            c = np.where(interrupted, free, 0)
            amb_c = interrupted & amB.any(0)
            if sut is not None:
                c = np.where(amb_c, np.abs(sut["option_id"].astype(np.int64)), c)
            amb |= amb_i | amb_c
        o_next = np.where(stay | declined | interrupted, 0, cand)
        option_id_next = np.where(interrupted, -c, np.where(stay | declined, -cand, cand))
        qcache = np.stack([qn[k][np.arange(n), :] for k in range(nvf)])[o_next, np.arange(n)].T       # [5, n]
        qcache_tol = np.stack(qn_tol)[o_next, np.arange(n)].T
        code = np.where(succ_o, 1, np.where(done != 0, 2, np.where(fail_o, 3, 4)))      # SPEC §9's outcome, first match wins
        events = goal.astype(np.int64)
        for k in range(1, min(nvf, 6)):
            events |= inA[k].astype(np.int64) << k
        out = dict(
            x=sn[0], y=sn[1], vx=sn[2], vy=sn[3], action=a, reward=reward, done=done,
            option_id=option_id_next, opt_steps=np.where(keep & ~interrupted, pre["opt_steps"].astype(np.int64) + 1, 0),
            ep_steps=np.where(done != 0, 0, eps1), events=events, ev_len=eps1, qcache=qcache, qcache_tol=qcache_tol,
            ambiguous=np.nonzero(amb)[0], entering=entering, stay=stay, declined=declined, cand=cand, keep=keep,
            interrupted=interrupted, c=c, vf=o, succ_o=succ_o, sp=sp,
            term=np.where(interrupted, 5, np.where(running & term, code, 0)),      # SPEC §10's record code, 5: §11's interrupt
            G=None, G_tol=None, n_k=None, W=None, W_tol=None, gest_succ=None, resolution=None, items=None)
        if not learn:
            return out

        # ---- SPEC §5: update items, targets, deltas, G
        del tab_n
        qs, qs_tol, phi_s, h_s = [], [], fourier_reference(*s), _half_products(*s)
        for k in range(nvf):
            q, tq = q_model(*s, W[k], (phi_s, h_s))
            qs.append(q[np.arange(n), a]); qs_tol.append(tq[np.arange(n), a])
        G = np.zeros((nvf, NACT, NF))
        G_tol = np.zeros((nvf, NACT, NF))
        n_k = np.zeros(nvf, np.int64)
        resolution = np.full((nvf, NACT), np.inf)
        gest_succ = np.zeros(nvf, np.int64)
        items, item_targets, item_rewards = {}, {}, {}
        for k in range(nvf):
            if k == 0:
                upd = np.ones(n, bool)
                r, cont, boot = reward, np.where(done != 0, 0.0, gam), np.zeros(n, bool)
            else:
                own = o == k
                gst = ~own & inS[k]
                pk = self.parents[k]
                succ_k = goal if pk == 0 else inA[pk]
                fail_k = ~succ_k & ~inA[k]
                gest_succ[k] = int(np.sum(inS[k] & succ_k))
                upd = own | gst
                r = np.where(own, r_o, reward + np.where(succ_k, self.r_succ, 0.0))
                cont = np.where(own, cont_o, np.where((done != 0) | succ_k | fail_k, 0.0, gam))
                boot = np.where(own, exit_o | interrupted, (succ_k | fail_k) & (done == 0)) & upd     # §12: r_o + γ m_0
            m_k, tm_k = V[k], V_tol[k]
            target = np.where(boot, r + gam * V[0], np.where(cont > 0, r + cont * m_k, r))
            t_tol = np.where(boot, gam * V_tol[0], np.where(cont > 0, cont * tm_k, 0.0)) + U32 * 4 * np.abs(target)
            delta = target - qs[k]
            d_tol = t_tol + qs_tol[k] + U32 * 2 * np.abs(delta)
            idx = np.nonzero(upd)[0]
            n_k[k] = len(idx)
            items[k] = idx
            item_targets[k], item_rewards[k] = target[idx], np.asarray(r, np.float64)[idx]
            nblk = max(1, -(-n // 256))
            Lg = L_BLOCK + -(-nblk // 16)
            for act in range(NACT):
                ii = idx[a[idx] == act]
                if len(ii) == 0:
                    continue
                dd = delta[ii]
                G[k, act] = dd @ phi_s[ii]
                ad = np.abs(dd)
                ad = np.where(np.isfinite(ad), ad, 0.0)
                G_tol[k, act] = d_tol[ii] @ np.abs(phi_s[ii]) + C_PHI * ad.sum() + C_G * np.sqrt(Lg) * U32 * (ad @ h_s[ii])
                resolution[k, act] = np.min(np.max(np.abs(dd[:, None] * phi_s[ii]), 1))

        # ---- apply
        W64 = W.astype(np.float64)
        W_next, W_tol = W64.copy(), np.zeros_like(W64)
        for k in range(nvf):
            if n_k[k] > 0:
                st = self.alpha / max(n_k[k], self.floor)
                W_next[k] = W64[k] + st * self.scale[None, :] * G[k]
                W_tol[k] = st * self.scale[None, :] * (G_tol[k] + 4 * U32 * np.abs(G[k])) + 2 * U32 * np.abs(W_next[k])

        out.update(G=G, G_tol=G_tol, n_k=n_k, W=W_next, W_tol=W_tol, gest_succ=gest_succ, resolution=resolution, items=items,
                   item_targets=item_targets, item_rewards=item_rewards)
        return out


def env_order_layout(option_id, n_vf, block_envs):
    """'chunked' or 'padded': which layout SPEC §5 prescribes for these option ids (used to show both are covered)."""
    o = np.asarray(option_id, np.int64)
    key = np.where(o <= 0, np.where(o > -n_vf, 0, n_vf), np.where(o < n_vf, o, n_vf))
    tot = np.bincount(key, minlength=7)
    S, R, Bf = int(tot[1:].sum()), int((tot[1:] > 0).sum()), len(o) // block_envs
    c = block_envs if (Bf <= R or S == 0) else min(block_envs, -(-S // (Bf - R)))
    U = int(sum(-(-int(x) // c) for x in tot[1:]))
    return "chunked" if U * block_envs <= len(o) else "padded"


def compare(m, got, G, n_k, W, events=None, ev_len=None, gest_succ=None, check_resolution=False, msg=""):
    """Assert that the outputs of a system under test (state dict `got`, G, n_k, W after apply, trace / gestation counters
    when given) agree with the model output `m`: discrete fields exactly (ambiguous envs excepted), floats to tolerance.
    An acting step (a model of learn=False) passes n_k = G = W = None. Returns the number of ambiguous envs."""
    n = len(m["x"])
    ok = np.ones(n, bool)
    ok[m["ambiguous"]] = False
    for k in ("x", "y", "vx", "vy", "action", "reward", "done", "option_id", "opt_steps", "ep_steps"):
        a = np.asarray(got[k]).astype(np.float64)
        b = np.asarray(m[k]).astype(np.float64)
        bad = np.nonzero(ok & ~((a == b) | (np.isnan(a) & np.isnan(b))))[0]
        assert len(bad) == 0, f"{msg} field {k}: {len(bad)} envs differ, first {bad[:5].tolist()}: got {a[bad[:5]].tolist()} model {b[bad[:5]].tolist()}"
    if events is not None:
        bad = np.nonzero(ok & (np.asarray(events).astype(np.int64) != m["events"]))[0]
        assert len(bad) == 0, f"{msg} events: {len(bad)} envs differ, first {bad[:5].tolist()}"
        assert np.array_equal(np.asarray(ev_len).astype(np.int64), m["ev_len"]), f"{msg} ev_len"
    if gest_succ is not None:
        assert np.array_equal(np.asarray(gest_succ).astype(np.int64), m["gest_succ"]), f"{msg} gest_succ {gest_succ} model {m['gest_succ']}"
    if n_k is not None:
        assert np.array_equal(np.asarray(n_k).astype(np.int64), m["n_k"]), f"{msg} n_k {np.asarray(n_k).tolist()} model {m['n_k'].tolist()}"
    q = np.asarray(got["qcache"]).astype(np.float64)
    err = np.abs(q - m["qcache"])[:, ok]
    fin = np.isfinite(m["qcache"][:, ok])
    assert np.array_equal(np.isfinite(q[:, ok]), fin), f"{msg} qcache: finiteness differs"
    assert np.all(err[fin] <= m["qcache_tol"][:, ok][fin]), f"{msg} qcache: max excess {np.max(err[fin] - m['qcache_tol'][:, ok][fin])}"
    for name, got_a, want, tol in (("G", G, m["G"], m["G_tol"]), ("W", W, m["W"], m["W_tol"])):
        if got_a is None:
            continue
        got_a = np.asarray(got_a).astype(np.float64)
        for k in range(len(want)):
            fin = np.isfinite(want[k])
            assert np.array_equal(np.isfinite(got_a[k]), fin), f"{msg} {name}[{k}]: finiteness differs"
            e = np.abs(got_a[k] - want[k])[fin]
            assert np.all(e <= tol[k][fin]), \
                f"{msg} {name}[{k}]: {np.sum(e > tol[k][fin])} elements out of tolerance, max excess {np.max(e - tol[k][fin])}"
    if check_resolution:                   # a dropped, duplicated or misrouted item moves G_k[a] by more than the tolerance
        for k in range(len(m["n_k"])):
            for a in range(NACT):
                if np.isfinite(m["resolution"][k, a]):
                    assert np.max(m["G_tol"][k, a]) < m["resolution"][k, a], \
                        f"{msg} VF {k} action {a}: tolerance {np.max(m['G_tol'][k, a])} not below the single-item resolution {m['resolution'][k, a]}"
    return len(m["ambiguous"])


def q_update_model(s, a, r, cont, sn, Wk):
    """SPEC §5 on explicit transitions (scg_q_update): G64[a] = sum_i delta_i phi(s_i), delta = r + cont max_a' Q(s', a') - Q(s, a)
    (the max only where cont > 0), with the per-element tolerance of the step model."""
    n = len(a)
    q, tq = q_model(*s, Wk)
    qn, tqn = q_model(*sn, Wk)
    cont = np.asarray(cont, np.float64)
    r = np.asarray(r, np.float64)
    m = np.where(cont > 0, np.fmax.reduce(qn, axis=1), 0.0)
    target = np.where(cont > 0, r + cont * m, r)
    delta = target - q[np.arange(n), a]
    d_tol = np.where(cont > 0, cont * tqn.max(1), 0.0) + tq[np.arange(n), a] + U32 * (4 * np.abs(target) + 2 * np.abs(delta))
    phi, h = fourier_reference(*s), _half_products(*s)
    G, G_tol = np.zeros((NACT, NF)), np.zeros((NACT, NF))
    Lg = L_BLOCK + -(-max(1, -(-n // 256)) // 16)
    for act in range(NACT):
        ii = np.nonzero(a == act)[0]
        if len(ii):
            G[act] = delta[ii] @ phi[ii]
            ad = np.abs(delta[ii])
            G_tol[act] = d_tol[ii] @ np.abs(phi[ii]) + C_PHI * ad.sum() + C_G * np.sqrt(Lg) * U32 * (ad @ h[ii])
    return G, G_tol


def q_update_floor(a, n_vf_blocks=1):
    """The absolute term of q_update_model's G tolerance where delta, P and G are subnormal, per action [5]: every item of
    the action carries the floors of Q(s, a) and of max Q(s', .) (Q_FLOOR each), one rounding each for the target's fma and
    the subtraction, two for P = delta * (AB.re, -AB.im) and two for its fmas into G (|phi|, |AB|, |CD| <= 1); then the
    block and segment additions, one rounding per block of the segment chain and 16 per segment."""
    n = len(a)
    nblk = max(1, -(-n // 256))
    per_item = 2 * Q_FLOOR + 6 * SUB
    return np.array([np.sum(np.asarray(a) == act) * per_item + (16 + -(-nblk // 16)) * SUB for act in range(NACT)])


def sigmoid_model(z):
    """SPEC §6's sigmoid in float64: the exact logistic of the argument clamped to |z| <= 87 (`a = max(-|z|, -87)` is part of
    the formula, so sigmoid(-100) is sigmoid(-87) ~ 1.64e-38 and not 3.7e-44), and its binary32 error bound C_SIG * p."""
    z = np.clip(np.asarray(z, np.float64), -87.0, 87.0)
    e = np.exp(-np.abs(z))
    p = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return p, C_SIG * p


def fit_model(xy, lab, w, iters, lr, l2):
    """SPEC §6 in float64: `iters` steps of full-batch gradient descent from w [8]; returns (w, per-weight bound [6]).
    The gradient descent of tests/test_gpu_ref64.py with a bound that stays meaningful where the sigmoid saturates: the
    sigmoid is the clamped one with a relative error (C_SIG), and every chain carries the absolute term of its roundings
    (SUB), so that gradients of 1e-38 and the subnormal weights they produce are resolved. The gradient sum keeps that
    test's constant (C_G sqrt(M / 8192 + 40) U32 sum |e| |psi|), psi adds 4 roundings (u, v, their products)."""
    w = np.asarray(w, np.float64).copy()
    xy, lab = np.asarray(xy, np.float64), np.asarray(lab, np.float64)
    M = len(lab)
    u, v = 2.0 * xy[:, 0] - 1.0, 2.0 * xy[:, 1] - 1.0
    psi = np.stack([np.ones_like(u), u, v, u * u, u * v, v * v], 1)
    apsi = np.abs(psi)
    n_sum = -(-M // 8192) + 6 + 15 + 7                  # roundings of one g_j: the chain, the butterfly, 15 + 7 ordered adds
    carry = np.r_[1.0, np.full(5, 1.0 + lr * l2)]       # a carried error of w_j comes back through l2 w_j (and through z, below)
    bound = np.zeros(6)
    for _ in range(iters):
        z = psi @ w[:6]
        tz = C_Z * ((apsi + U32) @ np.abs(w[:6])) + apsi @ bound          # binary32 z of the binary32 weights against this z
        p, tp = sigmoid_model(z)
        e = p - lab
        # sigmoid' = p (1 - p) changes by at most e^|dz| over dz; where both arguments are certain to be clamped it is 0
        te = tp + np.where(np.abs(z) - tz < 87.0, p * (1.0 - p) * np.exp(np.minimum(tz, 50.0)) * tz, 0.0) + U32 * np.abs(e)
        g = psi.T @ e / M
        gt = (te @ apsi + (4 + C_G * np.sqrt(M / 8192 + 40)) * U32 * (np.abs(e) @ apsi) + n_sum * SUB) / M
        reg = np.r_[0.0, l2 * w[1:6]]
        w_new = w[:6] - lr * (g + reg)
        # invM, g invM, l2 w, their sum and lr (..): 5 relative roundings and 2 that can be subnormal; then the subtraction
        bound = carry * bound + lr * (gt + 6 * U32 * (np.abs(g) + np.abs(reg)) + 2 * SUB) + U32 * np.abs(w_new) + SUB
        w[:6] = w_new
    return w, bound
