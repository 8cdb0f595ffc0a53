"""The host model of SPEC §29: §29.1's cross row values from any q_values, as lambda_model.row_values is §27.1's — the valuing
table's entry at the selecting table's argmax, or at a given action — and §29.2's double targets: the record's tables (tab0, tabk,
tabA) formed as SPEC §28.2 states them, the cross values, and trace_model's recurrence. What scg_row_values_cross and
valuefit.double_targets are held to, bit for bit."""
import numpy as np

import trace_model as TM
from lambda_model import ROW_NONE

NACT = 5


def row_values_cross(q_values, states, tab, W_sel, W_val, act=None):
    """(v float32 [n], a uint8 [n], vs float32 [n]) of SPEC §29.1 from `q_values(states_subset, Wk) -> [5][m]`. Without `act`: per
    table its rows' qs under W_sel[k] and qv under W_val[k]; m = SPEC §5's max of qs (m = qs[0]; m = max(m, qs[1]); ...), a* the
    lowest index with qs[a*] == m (five NaNs: 0), vs = m, v = qv[a*]. With `act` (the given mode): a* = act, only W_val is read, a
    row with act >= 5 is a row without a table, and vs is None. A row whose tab is >= len(W_val) gets +0 / 255 / +0."""
    tab = np.asarray(tab)
    n = len(tab)
    v, a = np.zeros(n, np.float32), np.full(n, 255, np.uint8)
    vs = np.zeros(n, np.float32) if act is None else None
    for k in range(len(W_val)):
        at = np.nonzero(tab == k)[0] if act is None else np.nonzero((tab == k) & (np.asarray(act) < NACT))[0]
        if not len(at):
            continue
        sub = [s[at] for s in states]
        qv = np.asarray(q_values(sub, W_val[k]), np.float32)
        if act is None:
            qs = np.asarray(q_values(sub, W_sel[k]), np.float32) if W_sel is not W_val else qv
            m = qs[0].copy()
            for j in range(1, NACT):
                m = np.maximum(m, qs[j])                       # (valuefit.greedy_max's chain; a NaN state makes all five NaN)
            best = np.zeros(len(at), np.int64)
            for j in range(NACT - 1, -1, -1):
                best = np.where(qs[j] == m, j, best)
            vs[at] = m
        else:
            best = np.asarray(act)[at].astype(np.int64)
        v[at], a[at] = qv[best, np.arange(len(at))], best.astype(np.uint8)
    return v, a, vs


def record_tables(flat):
    """(tab0, tabk, tabA) uint8 [total] of SPEC §28.2: the root's table on the rows that are not done; the row's own table on the
    rows with vf >= 1 whose option goes on; and the table that acts on the NEXT row, where that row is in the same env and this row
    ended no episode (done = 0, or an env's row 0)."""
    off = np.asarray(flat["offsets"], np.int64)
    done, vf, term = (np.asarray(flat[f], np.uint8) for f in ("done", "vf", "term"))
    total = len(done)
    tab0 = np.where(done == 0, 0, ROW_NONE).astype(np.uint8)
    tabk = np.where((vf >= 1) & (term == 0) & (done == 0), vf, ROW_NONE).astype(np.uint8)
    tabA = np.full(total, ROW_NONE, np.uint8)
    for e in range(len(off) - 1):
        for i in range(int(off[e]), int(off[e + 1]) - 1):
            if i == off[e] or done[i] == 0:
                tabA[i] = vf[i + 1]
    return tab0, tabk, tabA


def double_targets(q_values, flat, W_sel, W_val, gamma, lam_vf, r_succ, cut):
    """SPEC §29.2: dict of y0, yk, h (float64), v0, vk, vs0, vsk (float32) and ag (uint8): v0 / vk the cross values on tab0 / tabk,
    ag W_sel's greedy action on tabA, then trace_model.trace_returns."""
    states = [np.asarray(flat[f], np.float32) for f in ("x", "y", "vx", "vy")]
    tab0, tabk, tabA = record_tables(flat)
    v0, _, vs0 = row_values_cross(q_values, states, tab0, W_sel[:1], W_val[:1])
    vk, _, vsk = row_values_cross(q_values, states, tabk, W_sel, W_val)
    _, ag, _ = row_values_cross(q_values, states, tabA, W_sel, W_sel)
    total = len(flat["reward"])
    y0, yk, h = TM.trace_returns(flat["offsets"], total, flat["reward"], flat["done"], flat["vf"], flat["term"], flat["action"], ag, v0,
                                 vk, gamma, np.atleast_1d(lam_vf), TM.TRACE_CUT if cut else 0, r_succ)
    return {"y0": y0, "yk": yk, "h": h, "v0": v0, "vk": vk, "vs0": vs0, "vsk": vsk, "ag": ag}
