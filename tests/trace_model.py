"""The host model of SPEC §28.1: scg_trace_returns' two streams and the horizon over a flat record, the recurrence in plain Python
binary64 (a Python float operation is one IEEE binary64 operation, rounded once, never fused), one row at a time. The cases are
lambda_model.lambda_returns'; the one change is the trace coefficient, which is a per-row operand here: the mix at local row j takes
the coefficient of the row behind it. What scg_trace_returns is held to, bit for bit."""
import numpy as np

from lambda_model import TRIAL_SUCCESS

TRACE_CUT = 1              # include/scg_abi.h SCG_TRACE_CUT


def coefficient(i, vf, action, ag, lam_vf, flags):
    """c_i of SPEC §28.1 for a row i that is not its env's row 0: selected, never computed."""
    if (flags & TRACE_CUT) and int(action[i]) != int(ag[i - 1]):
        return 0.0
    k = int(vf[i])
    return float(lam_vf[k if k < len(lam_vf) else 0])


def trace_returns(offsets, total, reward, done, vf, term, action, ag, v0, vk, gamma, lam_vf, flags, r_succ, coefficients=None):
    """(y0, yk, h) float64 [total] of SPEC §28.1. Env e owns rows lo .. hi - 1 with lo = offsets[e] clamped into [0, total] and hi =
    offsets[e + 1] clamped into [lo, total]; rows no env owns keep +0. `lam_vf`: a sequence of 1 .. n_vf coefficients. With
    `coefficients` a list, (row, place, c) is appended for every coefficient a mix reads: place "root", "own" (an option going on)
    or "boot" (an option ended, the root carries on)."""
    gamma, R = float(gamma), float(r_succ)
    lam_vf = [float(v) for v in np.atleast_1d(lam_vf)]
    y0, yk, h = (np.zeros(total, np.float64) for _ in range(3))
    for e in range(len(offsets) - 1):
        lo = min(max(int(offsets[e]), 0), total)
        hi = min(max(int(offsets[e + 1]), lo), total)
        L = hi - lo
        n0 = nk = nh = 0.0                                     # y0, yk and h of row j + 1
        for j in range(L - 1, 0, -1):
            i = lo + j
            r, b0, bk, o = float(reward[i]), float(v0[i]), float(vk[i]), int(vf[i])
            end, last = done[i] != 0, j == L - 1
            c = omc = None
            if not last:                                       # rows without a row j + 1 in their env read no coefficient
                c = coefficient(i + 1, vf, action, ag, lam_vf, flags)
                omc = 1.0 - c                                  # per row, one subtraction

            def note(place):
                if coefficients is not None:
                    coefficients.append((i, place, c))

            if end:
                a0, ah = r, 1.0
            elif last:
                a0, ah = r + gamma * b0, 1.0
            else:
                a0, ah = r + gamma * (omc * b0 + c * n0), 1.0 + c * nh
                note("root")
            ak = 0.0
            if o >= 1:
                rb = r + (R if term[i] == TRIAL_SUCCESS else 0.0)
                if end:
                    ak = rb
                elif term[i] != 0:                             # the option ended, the root carries on
                    if last:
                        ak = rb + gamma * b0
                    else:
                        ak = rb + gamma * (omc * b0 + c * n0)
                        note("boot")
                elif not last and int(vf[i + 1]) == o:         # the option goes on
                    ak = rb + gamma * (omc * bk + c * nk)
                    note("own")
                else:
                    ak = rb + gamma * bk
            y0[i], yk[i], h[i] = a0, ak, ah
            n0, nk, nh = a0, ak, ah
    return y0, yk, h


def synthetic_actions(rng, flat, p_same=0.7):
    """SPEC §28.3's pattern on a flattened record: `action` uniform in 0 .. 4; ag[i] = action[i + 1] with probability p_same, else
    another action or 255 (ag of a record's last row: any of the six)."""
    total = len(flat["reward"])
    action = rng.integers(0, 5, total).astype(np.uint8)
    nxt = np.concatenate([action[1:], rng.integers(0, 5, min(total, 1)).astype(np.uint8)])
    other = (nxt + rng.integers(1, 5, total)) % 5
    other = np.where(rng.random(total) < 0.25, 255, other)
    ag = np.where(rng.random(total) < p_same, nxt, other).astype(np.uint8)
    return action, ag
