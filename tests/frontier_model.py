"""SPEC §13 frontier collection, modelled in numpy on the trace arrays of SPEC §7 (the oracle's ring_x / ring_y / events /
ev_len after sco_step, or hand-built ones). The cover test is the oracle's sco_classifier_predict (SPEC §4.1's z in its fma
order, no `known` term); everything else is integer bookkeeping and data movement, so the model is exact by construction."""
import numpy as np

import sc_oracle


def covered(x, y, clf, cover_mask):
    """True where (x, y) lies in an initiation set of cover_mask (rows of clf[n_vf, 8])."""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    cov = np.zeros(len(x), bool)
    out = np.empty(len(x), np.uint8)
    for k in range(1, clf.shape[0]):
        if (cover_mask >> k) & 1:
            w8 = np.ascontiguousarray(clf[k], np.float32)
            sc_oracle.lib().sco_classifier_predict(len(x), sc_oracle._p(x), sc_oracle._p(y), sc_oracle._p(w8),
                                                   sc_oracle._p(out))
            cov |= out != 0
    return cov


_oracle_covered = covered          # (collect_frontier's `covered=` argument shadows the name)


def collect_frontier(ring_x, ring_y, events, ev_len, target_mask, cover_mask, clf, l_pos, l_neg, ex_xy, ex_label, count,
                     covered=None, cap=None):
    """Append every node's hits in place: ex_xy[n_vf, cap, 2] f32, ex_label[n_vf, cap] u8, count[n_vf] i32. `covered` (bool per
    env: s_t lies in a set of cover_mask) replaces the oracle's predict when the test decides the cover itself; `cap` is given
    when the arrays carry a guard region behind each node's buffer."""
    ring_len, n = ring_x.shape
    n_vf = ex_label.shape[0]
    cap = ex_label.shape[1] if cap is None else int(cap)
    L = l_pos + l_neg
    el = np.asarray(ev_len, np.int64)
    live = el >= 1
    age0 = (np.maximum(el, 1) - 1) & (ring_len - 1)
    envs = np.arange(n)
    if covered is None:
        unc = ~_oracle_covered(ring_x[age0, envs], ring_y[age0, envs], clf, cover_mask)
    else:
        unc = ~np.asarray(covered, bool)
    v = np.minimum(np.minimum(L, el), ring_len)
    for p in range(n_vf):
        if not (target_mask >> p) & 1:
            continue
        hit = np.nonzero(live & unc & (((np.asarray(events) >> p) & 1) != 0))[0]     # env order
        he = np.repeat(hit, v[hit])
        j = np.concatenate([np.arange(v[e]) for e in hit]) if len(hit) else np.zeros(0, np.int64)  # ages ascending
        pos = int(count[p]) + np.arange(len(he))
        keep = (pos >= 0) & (pos < cap)
        he, j, pos = he[keep], j[keep], pos[keep]
        row = (el[he] - 1 - j) & (ring_len - 1)
        ex_xy[p, pos, 0] = ring_x[row, he]
        ex_xy[p, pos, 1] = ring_y[row, he]
        ex_label[p, pos] = (j < l_pos).astype(np.uint8)
        count[p] = min(cap, int(count[p]) + int(v[hit].sum()))


def collect_frontier_oracle(orc, target_mask, cover_mask, clf, l_pos, l_neg, ex_xy, ex_label, count):
    """The same on an oracle's attached trace buffers (sc_oracle.Oracle.set_trace)."""
    collect_frontier(orc.ring_x, orc.ring_y, orc.events, orc.ev_len, target_mask, cover_mask, clf, l_pos, l_neg, ex_xy,
                     ex_label, count)
