"""The CPU oracle's Pinball physics against the independent float64 model of SPEC §1.3 (tests/phys64.py).

A seeded sweep over every action, the shipped maps, the crowded synthetic maps and maps of exactly 64 / 65 / 128 / 129 / 256
edges, with random states and states made to sit on the physics' decisions: full speed and clips from outside +-2, balls
touching edges, sliding along them, hitting vertices and corners, hitting on sub-step 19, reaching the goal after a bounce,
and clamps at 0 and 1. Named cases with hand-derived answers follow. The SPEC's pruning argument (SPEC §1.3, last paragraph)
is checked on every edge the model saw intercept."""
import time

import numpy as np
import pytest

import phys64
import skill_chaining_with_graphs_amd as scg
from util import (REFINE_A, REFINE_B, cell_of, cell_reach, CELL_G, dense_map, edge_count_map, edge_hit_state,
                  edge_normals, hub_map, random_states)

f32 = np.float32
SQ8 = float(np.sqrt(f32(8.0)))              # |v| of (2, 2)
# Ambiguous env-steps measured in the sweep below: 349 of 234 315 (0.15 %) over all maps, at most 0.26 % on one map (edges129,
# whose adversarial states crowd round the target and its wall). The bound is per map.
AMB_RATE = 0.005


def _oracle(m):
    import sc_oracle
    from util import HP, SCALE
    return sc_oracle.Oracle(m, SCALE, n_envs=1, n_options=0, seed=0, n_threads=4, **HP)


def open_map():
    """No edges at all, the target straddling the right side of the unit square: only the clamp keeps a ball inside, and a
    ball can reach the goal outside [0, 1] (where the clamp must not act)."""
    return scg.parse_map("ball 0.01\ntarget 1.03 0.5 0.02\nstart 0.5 0.5\n", "open")


def maps():
    out = {name: scg.load_map(name) for name in ("pinball_empty", "pinball_simple", "pinball_maze")}
    out["dense"] = dense_map()
    out["hub12"] = hub_map(12)
    out["hub20"] = hub_map(20)
    for n in (64, 65, 128, 129, 256):
        out[f"edges{n}"] = edge_count_map(n)
    out["open"] = open_map()
    return out


MAPS = maps()
BOUNDARY_EDGES = {64: [63], 65: [63, 64], 128: [63, 64, 127], 129: [127, 128], 256: [63, 64, 127, 128, 255]}


def _unit(rng, n):
    t = rng.uniform(0, 2 * np.pi, n)
    return np.cos(t), np.sin(t)


def adversarial_states(m, rng, n):
    """States made to sit on the decisions of SPEC §1.3 (about n of each family, fewer where they would start inside an
    obstacle). Returns {family: (x, y, vx, vy)} as float32 arrays."""
    R = float(m.radius)
    h = R / 20
    E = m.edges.astype(np.float64)
    fam = {}
    x, y, vx, vy = random_states(m, n, int(rng.integers(1 << 30)), vmax=2.0)
    sgn = np.where(rng.random((2, n)) < 0.5, -1.0, 1.0)
    fam["full_speed"] = (x, y, (2.0 * sgn[0]).astype(f32), (2.0 * sgn[1]).astype(f32))
    big = rng.uniform(2.0, 3.5, (2, n)) * sgn
    fam["clip_outside"] = (x.copy(), y.copy(), big[0].astype(f32), big[1].astype(f32))
    if len(E):
        nrm = edge_normals(m) if _convex(m) else None
        j = rng.integers(0, len(E), n)
        side = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        if nrm is None:
            en = np.stack([E[j, 3], -E[j, 2]], 1) / np.hypot(E[j, 2], E[j, 3])[:, None]
            nn = en * side[:, None]
        else:
            nn = nrm[j]
        along = rng.uniform(0.05, 0.95, n)
        foot = E[j, 0:2] + along[:, None] * E[j, 2:4]
        tang = E[j, 2:4] / np.hypot(E[j, 2], E[j, 3])[:, None]
        # touching: centre at R (1 +- 2 %) from the edge, any direction, any speed
        p = foot + nn * R * rng.uniform(0.98, 1.02, n)[:, None]
        ux_, uy_ = _unit(rng, n)
        s = rng.uniform(0.3, SQ8, n)
        fam["touching"] = (p[:, 0], p[:, 1], ux_ * s, uy_ * s)
        # sliding: overlapping by 1 %, moving along the edge, within +-1 degree of parallel (toward or away)
        p = foot + nn * R * 0.99
        dl = np.radians(rng.uniform(-1.0, 1.0, n))
        dl[: n // 4] = 0.0
        d = tang * np.cos(dl)[:, None] - nn * np.sin(dl)[:, None]
        d *= np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]
        s = rng.uniform(0.3, 2.0, n)
        fam["sliding"] = (p[:, 0], p[:, 1], d[:, 0] * s, d[:, 1] * s)
        # first contact on sub-step 19 (i = 19): head-on, (i + 0.5) sub-steps of travel from contact
        s = rng.uniform(0.5, 2.0, n)
        gap = 19.5 * s * h
        p = foot + nn * (R + gap)[:, None]
        fam["substep19"] = (p[:, 0], p[:, 1], -nn[:, 0] * s, -nn[:, 1] * s)
        # vertices (shared by two edges; the map's concave corners among them): aimed at the vertex from any side
        vtx = E[j, 0:2]
        ux_, uy_ = _unit(rng, n)
        r0 = R * rng.uniform(1.0, 2.0, n)
        s = rng.uniform(0.5, SQ8, n)
        fam["vertex"] = (vtx[:, 0] + ux_ * r0, vtx[:, 1] + uy_ * r0, -ux_ * s, -uy_ * s)
    tx, ty, tr = (float(v) for v in m.target)
    ux_, uy_ = _unit(rng, n)
    r0 = tr + R * rng.uniform(0.0, 3.0, n)
    s = rng.uniform(0.5, SQ8, n)
    fam["near_goal"] = (tx + ux_ * r0, ty + uy_ * r0, -ux_ * s * rng.choice([-1.0, 1.0], n), -uy_ * s)
    # the goal after a bounce: between the target and the wall right of it (the edge-count maps put the target there)
    xg = tx + tr + R * rng.uniform(0.05, 1.0, n)
    fam["goal_bounce"] = (xg, ty + R * rng.uniform(-0.5, 0.5, n), rng.uniform(1.0, 2.0, n), rng.uniform(-0.2, 0.2, n))
    # clamps: at and beyond the sides of the unit square, moving out
    xc = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.003, n), rng.uniform(0.997, 1.0, n))
    yc = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.003, n), rng.uniform(0.997, 1.0, n))
    fam["clamp"] = (xc, yc, np.where(xc < 0.5, -2.0, 2.0), np.where(yc < 0.5, -1.5, 1.5))
    out = {}
    for k, (a, b, c, d) in fam.items():
        a, b = np.asarray(a, f32), np.asarray(b, f32)
        keep = np.array([(k == "clamp" or 0.0 < p < 1.0 and 0.0 < q < 1.0) and not m.inside_obstacle(float(p), float(q))
                         for p, q in zip(a, b)])
        out[k] = (a[keep], b[keep], np.asarray(c, f32)[keep], np.asarray(d, f32)[keep])
    return out


def _convex(m):
    for poly in m.polygons:
        p = poly.astype(np.float64)
        e = np.roll(p, -1, 0) - p
        cr = e[:, 0] * np.roll(e, -1, 0)[:, 1] - e[:, 1] * np.roll(e, -1, 0)[:, 0]
        if not (np.all(cr >= 0) or np.all(cr <= 0)):
            return False
    return True


def boundary_states(m, edges, rng, n_each=16):
    """Balls that hit the given edges head-on at various speeds and points along them."""
    out = []
    for j in edges:
        for k in range(n_each):
            out.append(edge_hit_state(m, j, gap=rng.uniform(0.05, 1.5), speed=rng.uniform(0.5, 2.0),
                                      along=rng.uniform(0.2, 0.8)))
    return tuple(np.array(c, f32) for c in zip(*out))


def check_pruning(m, res, x, y, margin=0.01):
    """SPEC §1.3's pruning argument on every (env, sub-step, edge) the model saw intercept: the edge lies within
    R (1 + 1.05 |v|) of the pre-step position, within the kernel's refined reach R (1.02 + 1.10 |v|) and within the cell-mask
    reach of the ball's cell centre, the last two with a relative margin."""
    env, sub, j = res["hits"]
    if len(env) == 0:
        return 0
    R = float(m.radius)
    E = m.edges.astype(np.float64)
    px, py = np.asarray(x, f32).astype(np.float64)[env], np.asarray(y, f32).astype(np.float64)[env]
    d = _dist_rows(E[j], px, py)
    v = res["speed"][env]
    spec = R * (1.0 + 1.05 * v)
    assert np.all(d <= spec * (1 + 1e-9)), f"an edge intercepted beyond R (1 + 1.05 |v|): excess {np.max(d - spec)}"
    refined = R * (REFINE_A + REFINE_B * v)
    assert np.all(d <= refined * (1 - margin)), f"an intercepted edge within {margin} of the refined reach"
    cx, cy = cell_of(np.asarray(x, f32)[env], np.asarray(y, f32)[env])
    dc = _dist_rows(E[j], (cx + 0.5) / CELL_G, (cy + 0.5) / CELL_G)
    assert np.all(dc <= cell_reach(R) * (1 - margin)), f"an intercepted edge within {margin} of the cell-mask reach"
    return len(env)


def _dist_rows(E, px, py):
    dx, dy = px - E[:, 0], py - E[:, 1]
    t = np.clip((dx * E[:, 2] + dy * E[:, 3]) / (E[:, 2] ** 2 + E[:, 3] ** 2), 0.0, 1.0)
    return np.hypot(E[:, 0] + E[:, 2] * t - px, E[:, 1] + E[:, 3] * t - py)


def run_oracle(orc, x, y, vx, vy, a):
    X, Y, VX, VY = (np.array(v, f32) for v in (x, y, vx, vy))
    r, g = orc.pinball_step(X, Y, VX, VY, np.broadcast_to(np.asarray(a, np.uint8), X.shape).copy())
    return X, Y, VX, VY, r, g


@pytest.mark.parametrize("name", list(MAPS))
def test_oracle_physics_matches_float64_model(name):
    """Every action on random and adversarial states: reward and goal exact, the state within the propagated bound, every
    env not ambiguous; ambiguous envs rare; every intercepted edge inside the pruning bounds."""
    t0 = time.time()
    m = MAPS[name]
    orc = _oracle(m)
    rng = np.random.default_rng(sum(map(ord, name)))
    fam = adversarial_states(m, rng, 400)
    if m.n_edges:
        fam["random"] = random_states(m, 1000, int(rng.integers(1 << 30)), vmax=2.8)
    n_edges = m.n_edges
    if name.startswith("edges"):
        fam["mask_words"] = boundary_states(m, BOUNDARY_EDGES[n_edges], rng)
    n_amb = n_steps = n_hits = n_goal = n_multi = n_sub19 = 0
    for a in range(5):
        for k, (x, y, vx, vy) in fam.items():
            res = phys64.step(m, x, y, vx, vy, np.full(len(x), a))
            X, Y, VX, VY, r, g = run_oracle(orc, x, y, vx, vy, a)
            n_amb += phys64.compare(res, X, Y, VX, VY, r, g, msg=f"{name} a={a} {k}")
            n_steps += len(x)
            n_hits += check_pruning(m, res, x, y)
            n_goal += int(g.sum())
            env, sub, j = res["hits"]
            if len(env):
                n_multi += int(np.sum(np.bincount(env * 20 + sub) > 1))
                n_sub19 += int(np.sum(sub == 19))
            if k == "mask_words":
                for e in BOUNDARY_EDGES[n_edges]:
                    assert np.any(j == e), f"{name}: edge {e} is never hit"
    assert n_amb <= AMB_RATE * n_steps, f"{name}: {n_amb} of {n_steps} env-steps ambiguous"
    if n_edges:
        assert n_multi > 0 and n_sub19 > 0, f"{name}: the states reach no corner ({n_multi}) or no sub-step-19 hit ({n_sub19})"
    print(f"{name}: {n_steps} env-steps, {n_amb} ambiguous, {n_hits} intercepts ({n_multi} multi-edge sub-steps, "
          f"{n_sub19} on sub-step 19), {n_goal} goals, {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------- named edge cases

def step1(m, x, y, vx, vy, a, orc=None):
    """One env through the oracle and the model; asserts that they agree and that the env is not ambiguous. Returns the
    oracle's (x, y, vx, vy, reward, goal) and the model result."""
    orc = orc or _oracle(m)
    x, y, vx, vy = (np.array([v], f32) for v in (x, y, vx, vy))
    res = phys64.step(m, x, y, vx, vy, np.array([a]))
    X, Y, VX, VY, r, g = run_oracle(orc, x, y, vx, vy, a)
    assert not res["ambiguous"][0]
    phys64.compare(res, X, Y, VX, VY, r, g)
    return (float(X[0]), float(Y[0]), float(VX[0]), float(VY[0]), float(r[0]), int(g[0])), res


def _moves(x, v, h, k):
    for _ in range(k):
        x = f32(np.float64(v) * np.float64(h) + np.float64(x))        # fma(v, h, x): exact in float64, rounded once
    return x


def test_sliding_parallel_to_a_wall():
    """Overlapping the right wall (inner face x = 0.99, R = 0.02) and moving straight up: dot = 0 exactly at every sub-step,
    so the wall intercepts 20 times and mirrors (vx, vy) about itself: the velocity is unchanged, and the extra move of
    sub-step 19 makes 21 moves."""
    m = scg.load_map("pinball_empty")
    h = f32(m.scalars[1])
    got, res = step1(m, 0.9705, 0.5, 0.0, 1.0, 4)
    assert got == (float(f32(0.9705)), float(_moves(f32(0.5), f32(1.0), h, 21)), 0.0, float(f32(1.0) * f32(0.995)), -1.0, 0)
    env, sub, j = res["hits"]
    assert sorted(sub.tolist()) == list(range(20)) and len(set(j.tolist())) == 1


def test_moving_away_just_past_kappa_is_not_intercepted():
    """Overlapping the right wall, moving away at 90.55 degrees from the wall normal: cos^2 = 9.2e-5 is above KAPPA2
    (6.2e-5, 90.45 degrees) and below 2 KAPPA2: no intercept, the velocity only drags."""
    m = scg.load_map("pinball_empty")
    ang = np.radians(0.55)
    vx, vy = f32(-np.sin(ang)), f32(np.cos(ang))
    got, res = step1(m, 0.9705, 0.3, vx, vy, 4)
    assert len(res["hits"][0]) == 0
    assert got[2] == float(vx * f32(0.995)) and got[3] == float(vy * f32(0.995))


def test_convex_vertex_reverses():
    """Straight at the corner of a square (x0 + 0.02, y0 + 0.02) along the diagonal: both edges of the corner are at the
    same distance, both intercept in one sub-step, and the velocity is reversed (not mirrored)."""
    m = edge_count_map(64)
    R = float(m.radius)
    c = np.array([0.1 + 0.02, 0.1 + 0.02])
    p = c + np.array([1.0, 1.0]) / np.sqrt(2) * R * 1.5
    got, res = step1(m, p[0], p[1], -1.0, -1.0, 4)
    assert got[2] == float(f32(1.0) * f32(0.995)) and got[3] == float(f32(1.0) * f32(0.995))
    env, sub, j = res["hits"]
    assert len(j) == 2 and sub[0] == sub[1]


def test_concave_corner_reverses():
    m = scg.load_map("pinball_empty")
    got, res = step1(m, 0.9695, 0.9695, 1.0, 1.0, 4)
    assert got[2] == float(f32(-1.0) * f32(0.995)) and got[3] == float(f32(-1.0) * f32(0.995))
    env, sub, j = res["hits"]
    assert len(set(j.tolist())) == 2 and np.bincount(sub).max() == 2


def test_hit_on_substep_19_takes_the_extra_move():
    """Right wall contact at x >= 0.97 (R = 0.02, hstep = 0.001, vx = 1): from 0.9505 the 20th move (i = 19) makes the
    first contact; the mirrored velocity then moves the ball once more, back to about 0.9695."""
    m = scg.load_map("pinball_empty")
    h = f32(m.scalars[1])
    got, res = step1(m, 0.9505, 0.5, 1.0, 0.0, 4)
    x20 = _moves(f32(0.9505), f32(1.0), h, 20)
    assert got[0] == float(_moves(x20, f32(-1.0), h, 1))
    assert got[2] == float(f32(-1.0) * f32(0.995)) and got[3] == 0.0
    env, sub, j = res["hits"]
    assert sub.tolist() == [19]


def test_goal_after_a_bounce_without_drag_or_clamp():
    """edges64: target (0.955, 0.955) r 0.02 beside the right wall (contact at x >= 0.98, R = 0.01, 0.001 per sub-step at
    vx = 2): the ball leaves 0.9765, bounces at i = 3 and enters the target at i = 9; vx = -2 stays undragged."""
    m = edge_count_map(64)
    h = f32(m.scalars[1])
    got, res = step1(m, 0.9765, 0.955, 2.0, 0.0, 4)
    x = _moves(_moves(f32(0.9765), f32(2.0), h, 4), f32(-2.0), h, 6)
    assert got == (float(x), float(f32(0.955)), -2.0, 0.0, 10000.0, 1)
    assert res["hits"][1].tolist() == [3]


def test_goal_outside_the_unit_square_is_not_clamped():
    m = open_map()
    got, res = step1(m, 0.9953, 0.5, 2.0, 0.0, 4)
    assert got[5] == 1 and got[0] > 1.0 and got[2] == 2.0


def test_clamp_at_zero_and_one():
    m = open_map()
    got, _ = step1(m, 0.001, 0.999, -2.0, 2.0, 4)
    assert got[0] == 0.0 and got[1] == 1.0 and got[5] == 0


def test_clip_of_both_components():
    """A thrust along y clips vx as well: (3.5, 0) with ACC_Y becomes (2, 0.2) before the move."""
    m = open_map()
    got, _ = step1(m, 0.3, 0.3, 3.5, 0.0, 1)
    assert got[2] == float(f32(2.0) * f32(0.995)) and got[3] == float(f32(0.2) * f32(0.995))
