"""A plain float64 model of one Pinball env step (SPEC §1.3), written from the SPEC and not from the oracle or the kernel.

Every env is stepped with the SPEC's operations taken in float64: the impulse and the clip of both components, 20 sub-steps
with a full scan of the edge table in table order, `intercept` (the `d2 > R2` test, `dot >= 0`, the KAPPA2 test), the
count-edges rule (one hit mirrors, more than one reverses), the extra move on `i == 19`, the goal test, drag and clamp only
when the goal was not reached, and the reward. The map's binary32 table (`x0, y0, ex, ey, inv_len2, ux, uy`) and its scalars
(R2, TR2, hstep, TX, TY) are exact input data.

Error bounds. Per env, in float64, as sums of absolute values, the model carries a bound on the distance between its value
and any binary32 evaluation of the same operations: `eP` on the Euclidean norm of the position error, `eV` on that of the
velocity error (constants `C_*` below, each derived where it is defined). Norms rather than components, because the mirror
is a reflection: it keeps the norm of an error vector, where a bound per component would triple at every bounce. Every discrete decision gets a margin the same way: `d2` against `R2`, the sign of
`dot`, the KAPPA2 comparison and the goal test. A decision lies within its bound when its float64 margin is not larger than
the bound; `intercept` is then evaluated in three-valued logic (surely true, surely false, open), so that a decision within its
bound counts only where it can change the result: a ball sliding along a wall has `dot` within its bound of 0, but it is
intercepted either way (`dot >= 0`, or `dot * dot` far below the KAPPA2 side). An env with an open intercept or an open goal
test at any sub-step is AMBIGUOUS: the tested system gives only the final state, so the model cannot follow it through that
sub-step; such envs are excluded from the comparison and reported. The clip, the `t` clamp and the final clamp are
continuous (1-Lipschitz) and are not decisions.

For every env that is not ambiguous, reward and goal are exact and `x, y, vx, vy` lie within the propagated bound. The model
also records the edges that intercept at each sub-step (`hits`: env, sub-step, edge), for the pruning checks of the tests.
float64 rounding (2^-53 relative) is absorbed by the slack of the constants below.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24                       # unit roundoff of binary32

DV = float(np.float32(0.2))          # SPEC §1.3 constants, as the binary32 values both sides embed
VMAX = 2.0
DRAG = float(np.float32(0.995))
KAPPA2 = float.fromhex("0x1.0553bep-14")

# ---- error-bound constants (binary32 evaluation against the float64 value of the same formula)
# One binary32 operation on exact operands errs by at most U |result|; an fma rounds once.
# impulse: vx + DV, one rounding: U |vx'|. The clip is 1-Lipschitz.
C_IMP = 1.0
# move: x' = fma(vx, h, x), y' likewise: eP + h eV plus one rounding of each component, U (|x'| + |y'|).
C_MOVE = 1.0
# closest point b = c - p (Euclidean norm of the error vector). With the binary32 position p32 and the float64 position p64,
# |b(p32) - b(p64)| <= |p32 - p64| <= eP: b is p -> clip-projection(p) - p, the residual of the projection on a segment, which
# is non-expansive (the table's inv_len2 is 1/|e|^2 to 2^-24, a factor 1 + 1e-7 the slack covers).
# Local roundings on p32, per component, with d = p - p0: dx, dy: U |d|; the numerator fma(dy, ey, dx ex): |e| sqrt(2) U |d|
# from dx, dy, plus U |dx ex| + U |num| <= 2 U |e| |d|; the product with inv_len2: U |t|; so
# |e| err(t) <= (sqrt(2) + 2) U |d| + U |e| |t| <= 4.5 U |d| (|e| |t| <= |d| where t is not clamped); cx = fma(ex, t, x0):
# U |cx|; bx = cx - x: U |bx|. Per component U (4.5 |d| + |c| + |b|) with |c|, |b| the component sums, as a Euclidean
# norm sqrt(2) times that: C_B = 1.5 (slack 6 %).
C_B = 1.5
# d2 = fma(by, by, bx bx): |b32|^2 - |b64|^2 <= 2 |b| eb + eb^2, plus U bx^2 + U d2 <= 2 U d2 (C_D2 = 3: slack).
C_D2 = 3.0
# dot = fma(by, vy, bx vx): |b| eV + |v| eb + eb eV, plus U |bx vx| + U |dot| <= 2 U |b| |v| (C_DOT = 3: slack).
C_DOT = 3.0
# vv = fma(vy, vy, vx vx): 2 |v| eV + eV^2 + 2 U vv (C_VV = 3).
C_VV = 3.0
# KAPPA2 test: lhs = dot * dot: 2 |dot| tdot + tdot^2 + U lhs. rhs = (KAPPA2 d2) vv: KAPPA2 (vv td2 + d2 tvv + td2 tvv) plus
# two roundings, 2 U rhs (C_RHS = 3).
C_LHS = 2.0
C_RHS = 3.0
# mirror: v' = 2 (v.u) u - v is the reflection A = 2 u u^T - I, |A| <= 1 + 4 U for the table's |u| = 1 to 2^-24: it carries
# eV to (1 + 4 U) eV. Roundings: p = fma(vy, uy, vx ux), U |vx ux| + U |p| <= 2 U |v|, which 2 p u doubles to 4 U |v|; then
# vx' = fma(2p, ux, -vx) and vy' once each, U (|vx'| + |vy'|) <= 2 U |v| (1 + 4 U). 6 U |v| in all (C_MIR = 8: slack).
C_MIR = 8.0
# goal: gx = x - TX, gy = y - TY (U (|gx| + |gy|)), g2 = fma(gy, gy, gx gx): 2 |g| eG + eG^2 with eG = eP + U (|gx| + |gy|),
# plus U gx^2 + U g2 <= 2 U g2 (C_GOAL = 3: slack).
C_GOAL = 3.0
# drag: vx * DRAG, vy * DRAG: DRAG eV + U (|vx'| + |vy'|). The clamp is 1-Lipschitz.
C_DRAG = 1.0


class PhysResult(dict):
    """x, y, vx, vy (float64), reward, goal, tolerances tx, ty, tvx, tvy, `ambiguous` (bool per env), `hits` (env, sub-step,
    edge) int arrays, `speed` (|v| after the impulse and the clip), `pre` (the pre-step position)."""


def step(pmap_or_table, x, y, vx, vy, action, scalars=None, chunk=1024):
    """One SPEC §1.3 step of every env. pmap_or_table: a PinballMap, or an edge table [n_edges, 8] float32 with `scalars`
    = [R, hstep, R2, TX, TY, TR2] float32. State and action arrays are not modified. Envs are independent: the work is
    done `chunk` envs at a time."""
    if scalars is None:
        E, S = pmap_or_table.edges, pmap_or_table.scalars
    else:
        E, S = pmap_or_table, scalars
    n = len(x)
    a = np.broadcast_to(np.asarray(action, np.int64), (n,))
    parts = [_step(E, S, x[i:i + chunk], y[i:i + chunk], vx[i:i + chunk], vy[i:i + chunk], a[i:i + chunk])
             for i in range(0, max(n, 1), chunk)]
    out = PhysResult()
    for k in parts[0]:
        if k == "hits":
            out[k] = tuple(np.concatenate([p[k][c] + (i * chunk if c == 0 else 0) for i, p in enumerate(parts)]) for c in range(3))
        elif k == "pre":
            out[k] = tuple(np.concatenate([p[k][c] for p in parts]) for c in range(2))
        else:
            out[k] = np.concatenate([p[k] for p in parts])
    return out


def _step(E, S, x, y, vx, vy, action):
    E = np.asarray(E, np.float32).astype(np.float64)
    _, h, R2, TX, TY, TR2 = (float(v) for v in np.asarray(S, np.float32))
    x0, y0, ex_, ey_, il2 = (E[:, k][None, :] for k in range(5))
    n = len(x)
    a = np.asarray(action, np.int64)
    X = np.asarray(x, np.float32).astype(np.float64)
    Y = np.asarray(y, np.float32).astype(np.float64)
    VX = np.asarray(vx, np.float32).astype(np.float64)
    VY = np.asarray(vy, np.float32).astype(np.float64)
    eP = np.zeros(n)

    # impulse (only effect of the action), then clip both components
    dvx = np.where(a == 0, DV, np.where(a == 2, -DV, 0.0))
    dvy = np.where(a == 1, DV, np.where(a == 3, -DV, 0.0))
    VX = VX + dvx
    VY = VY + dvy
    eV = C_IMP * U * (np.abs(dvx) > 0) * np.abs(VX) + C_IMP * U * (np.abs(dvy) > 0) * np.abs(VY)
    VX = np.clip(VX, -VMAX, VMAX)
    VY = np.clip(VY, -VMAX, VMAX)
    speed = np.hypot(VX, VY)

    amb = np.zeros(n, bool)
    goal = np.zeros(n, bool)
    live = np.ones(n, bool)                 # not yet in the goal
    hit_env, hit_sub, hit_edge = [], [], []

    def move(X, Y, eP, m):
        Xn = np.where(m, X + VX * h, X)
        Yn = np.where(m, Y + VY * h, Y)
        return Xn, Yn, np.where(m, eP + h * eV + C_MOVE * U * (np.abs(Xn) + np.abs(Yn)), eP)

    for i in range(20):
        X, Y, eP = move(X, Y, eP, live)
        if E.shape[0]:
            Xc, Yc = X[:, None], Y[:, None]
            dx, dy = Xc - x0, Yc - y0
            t = np.clip((dy * ey_ + dx * ex_) * il2, 0.0, 1.0)
            bx = (x0 + ex_ * t) - Xc
            by = (y0 + ey_ * t) - Yc
            d2 = by * by + bx * bx
            bn = np.sqrt(d2)
            cx, cy = x0 + ex_ * t, y0 + ey_ * t
            M = 4.5 * np.hypot(dx, dy) + np.abs(cx) + np.abs(cy) + np.abs(bx) + np.abs(by)
            eb = eP[:, None] + C_B * U * M
            td2 = 2.0 * bn * eb + eb * eb + C_D2 * U * d2
            eVc = eV[:, None]
            vn = speed[:, None]
            dot = by * VY[:, None] + bx * VX[:, None]
            tdot = bn * eVc + vn * eb + eb * eVc + C_DOT * U * bn * vn
            vv = (VY * VY + VX * VX)[:, None]
            tvv = 2.0 * vn * eVc + eVc * eVc + C_VV * U * vv
            lhs = dot * dot
            rhs = (KAPPA2 * d2) * vv
            tl = 2.0 * np.abs(dot) * tdot + tdot * tdot + C_LHS * U * lhs
            tr = KAPPA2 * (vv * td2 + d2 * tvv + td2 * tvv) + C_RHS * U * rhs
            near = ~(d2 > R2)
            near_lo, near_hi = d2 + td2 <= R2, d2 - td2 <= R2
            tow = dot >= 0
            tow_lo, tow_hi = dot - tdot >= 0, dot + tdot >= 0
            kap = lhs <= rhs
            kap_lo, kap_hi = lhs + tl <= rhs - tr, lhs - tl <= rhs + tr
            hit = near & (tow | kap) & live[:, None]
            hlo = near_lo & (tow_lo | kap_lo)
            hhi = near_hi & (tow_hi | kap_hi)
            amb |= live & np.any(hhi & ~hlo, axis=1)
            nhit = hit.sum(1)
            first = np.argmax(hit, axis=1)
            ee, jj = np.nonzero(hit)
            hit_env.append(ee); hit_sub.append(np.full(len(ee), i)); hit_edge.append(jj)
            one, many = nhit == 1, nhit > 1
            if one.any():
                fux, fuy = E[first, 5], E[first, 6]
                p = VY * fuy + VX * fux
                tp = p + p
                nvx, nvy = tp * fux - VX, tp * fuy - VY
                VX, VY = np.where(one, nvx, VX), np.where(one, nvy, VY)
                eV = np.where(one, (1.0 + 4.0 * U) * eV + C_MIR * U * speed, eV)
                if i == 19:
                    X, Y, eP = move(X, Y, eP, one & live)
            VX, VY = np.where(many, -VX, VX), np.where(many, -VY, VY)
        gx, gy = X - TX, Y - TY
        g2 = gy * gy + gx * gx
        eG = eP + U * (np.abs(gx) + np.abs(gy))
        tg = 2.0 * np.sqrt(g2) * eG + eG * eG + C_GOAL * U * g2
        reach = live & (g2 < TR2)
        amb |= live & ((g2 - tg < TR2) != (g2 + tg < TR2))
        goal |= reach
        live &= ~reach

    # drag and clamp only when the goal was not reached
    nv = ~goal
    VXd, VYd = VX * DRAG, VY * DRAG
    eV = np.where(nv, DRAG * eV + C_DRAG * U * (np.abs(VXd) + np.abs(VYd)), eV)
    VX, VY = np.where(nv, VXd, VX), np.where(nv, VYd, VY)
    X, Y = np.where(nv, np.clip(X, 0.0, 1.0), X), np.where(nv, np.clip(Y, 0.0, 1.0), Y)
    reward = np.where(goal, 10000.0, np.where(a == 4, -1.0, -5.0))
    cat = (lambda L: np.concatenate(L) if L else np.zeros(0, np.int64))
    return PhysResult(x=X, y=Y, vx=VX, vy=VY, reward=reward, goal=goal, tx=eP, ty=eP, tvx=eV, tvy=eV, ambiguous=amb,
                      hits=(cat(hit_env), cat(hit_sub), cat(hit_edge)), speed=speed,
                      pre=(np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)))


def compare(res, x, y, vx, vy, reward, goal, msg=""):
    """Assert that a binary32 result (final x, y, vx, vy, reward, goal) agrees with the model on every env that is not
    ambiguous: reward and goal exactly, the state to the propagated tolerance. Returns the number of ambiguous envs."""
    ok = ~res["ambiguous"]
    g = np.asarray(goal).astype(bool)
    bad = np.nonzero(ok & (g != res["goal"]))[0]
    assert len(bad) == 0, f"{msg} goal: {len(bad)} envs differ, first {bad[:5].tolist()}"
    r = np.asarray(reward).astype(np.float64)
    bad = np.nonzero(ok & (r != res["reward"]))[0]
    assert len(bad) == 0, f"{msg} reward: {len(bad)} envs differ, first {bad[:5].tolist()}"
    for name, got, tol in (("x", x, "tx"), ("y", y, "ty"), ("vx", vx, "tvx"), ("vy", vy, "tvy")):
        e = np.abs(np.asarray(got).astype(np.float64) - res[name])
        bad = np.nonzero(ok & ~(e <= res[tol]))[0]
        assert len(bad) == 0, (f"{msg} {name}: {len(bad)} envs out of tolerance, first {bad[:5].tolist()}: error "
                               f"{e[bad[:5]].tolist()} tolerance {res[tol][bad[:5]].tolist()}")
    return int(np.sum(res["ambiguous"]))


def seg_dist(E, px, py):
    """float64 distance from points (px, py) [n] to every edge of the table E [m, 8]: [n, m]."""
    E = np.asarray(E, np.float32).astype(np.float64)
    dx, dy = px[:, None] - E[None, :, 0], py[:, None] - E[None, :, 1]
    l2 = E[None, :, 2] ** 2 + E[None, :, 3] ** 2
    t = np.clip((dx * E[None, :, 2] + dy * E[None, :, 3]) / l2, 0.0, 1.0)
    return np.hypot(E[None, :, 0] + E[None, :, 2] * t - px[:, None], E[None, :, 1] + E[None, :, 3] * t - py[:, None])
