"""Host models of SPEC §17 for the tests.

`cross(phi, phi2, offsets, rows, cols)` is §17.1 on index lists: §16.1's two-level chains (tests/gram_model.py) with phi_i(s_n)
and phi_j(s2_n) as the operands, rows of the result the features of s, columns those of s2. `cross_chain_bound` is
gram_model.chain_bound's formula with sum |phi_i(s) phi_j(s2)| and the float64 product it bounds the distance to.
`lattice_cross` is the whole-matrix form through gram_model.chain (lattice prefix exact, real tail by the fma32 chain).

`scalar_items` and `scalar_residual` are §17.2 for one env and one sample as plain loops, the yardsticks of valuefit.td_samples
and of the residuals SkillChainingAgent.fit_values_lstdq forms."""
import numpy as np

from gram_model import SLAB, chain, fma32, slabs

CONT, BOOT, END = 0, 1, 2
SUCCESS = 1                                                  # SCG_TRIAL_SUCCESS


def cross(phi, phi2, offsets, rows, cols):
    """C_g[rows][cols] for every segment: float32 [n_seg][len(rows)][len(cols)]."""
    phi, phi2 = np.asarray(phi, np.float32), np.asarray(phi2, np.float32)
    rows, cols = np.asarray(rows), np.asarray(cols)
    out = np.zeros((len(offsets) - 1, len(rows), len(cols)), np.float32)
    for g in range(len(offsets) - 1):
        for lo, hi in slabs(int(offsets[g]), int(offsets[g + 1])):
            P = np.zeros(out.shape[1:], np.float32)
            for n in range(lo, hi):
                P = fma32(phi[n, rows][:, None], phi2[n, cols][None, :], P)
            out[g] = out[g] + P
    return out


def lattice_cross(phi, phi2, offsets, lattice=None, rows=None, cols=None):
    """C_g by gram_model.chain: whole (rows / cols None) or on index lists; `lattice` marks the samples both of whose states are
    lattice states, a prefix of every slab."""
    phi, phi2 = np.asarray(phi, np.float32), np.asarray(phi2, np.float32)
    return chain(phi if rows is None else phi[:, rows], phi2 if cols is None else phi2[:, cols], offsets, lattice)


def cross_chain_bound(phi, phi2, offsets):
    """The float64 product phi^T phi2 per segment and the bound on |C_g - it| per entry, both [n_seg][F][F]:
    (1024 + n_slabs) 2^-24 sum_n |phi_i(s_n) phi_j(s2_n)| (1 + 2^-10), the standard chain bound for each of the two levels."""
    p, q = np.asarray(phi, np.float32).astype(np.float64), np.asarray(phi2, np.float32).astype(np.float64)
    ref, bound = [], []
    for g in range(len(offsets) - 1):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        ref.append(p[lo:hi].T @ q[lo:hi])
        bound.append((SLAB + len(slabs(lo, hi))) * 2.0 ** -24 * (np.abs(p[lo:hi]).T @ np.abs(q[lo:hi])) * (1 + 2.0 ** -10))
    return np.stack(ref), np.stack(bound)


def scalar_items(reward, done, vf, term, k, r_succ):
    """§17.2 for one env (its rows, the begin row first) and value function k: [(row, kind, r)] in row order, r in float64."""
    out = []
    for j in range(1, len(reward)):
        if k == 0:
            out.append((j, CONT if done[j] == 0 else END, float(reward[j])))
        elif vf[j] == k:
            r = float(reward[j]) + (float(r_succ) if term[j] == SUCCESS else 0.0)
            if term[j] == 0:
                kind = CONT
            elif done[j] == 0:
                kind = BOOT
            else:
                kind = END
            out.append((j, kind, r))
    return out


def scalar_residual(r, kind, gamma, q_sa, qn_k, qn_0):
    """(a', delta) of one sample: qn_k / qn_0 the five binary32 values of Q_k / Q_0 at s', q_sa = Q_k(s, a). The max in §5's order,
    a' its lowest index; delta = (r + gamma m) - q_sa in float64, rounded to binary32 once."""
    m = np.float32(qn_k[0])
    for a in range(1, 5):
        m = max(m, np.float32(qn_k[a]))
    a2 = [a for a in range(5) if np.float32(qn_k[a]) == m][0]
    t = float(r)
    if kind == CONT:
        t = t + float(gamma) * float(m)
    elif kind == BOOT:
        m0 = np.float32(qn_0[0])
        for a in range(1, 5):
            m0 = max(m0, np.float32(qn_0[a]))
        t = t + float(gamma) * float(m0)
    return a2, np.float32(t - float(q_sa))
