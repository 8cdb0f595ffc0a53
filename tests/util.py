"""The tests' rig, host side only (nothing here needs a device; tests/gpu_util.py holds the half that does).

`oracle_block(b)` puts the oracle on its build for another SPEC §5 block size for a `with` body and back on the 256-env build
after it. `make_oracle` is an oracle with the test hyper-parameters HP. `random_states`, `random_env_state`, `entry_state`,
`random_weights`, `crossing_weights` and the classifier layouts (`chain_classifiers`, `wide_chain`, `sibling_tree`) are the
seeded inputs the parity tests share: a test that needs "some running env batch" takes
random_env_state and uploads it with gpu_util.state_to_device. The maps below (dense, hub, edge-count, pocket) and the
restatement of the HIP physics' candidate pruning serve the physics tests."""
import contextlib

import numpy as np

import sc_oracle
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd.core import EnvState, fourier_scale_table

SCALE = fourier_scale_table()
HP = dict(gamma=0.99, alpha=1e-3, epsilon=0.1, r_option_success=100.0, max_episode_steps=60,
          max_option_steps=25)


@contextlib.contextmanager
def oracle_block(block_envs):
    """The oracle built for `block_envs` (64 / 128 / 256) inside the body; the default 256-env build after it, also on an error."""
    sc_oracle.use_block_envs(block_envs)
    try:
        yield block_envs
    finally:
        sc_oracle.use_block_envs(256)


def make_oracle(map_name, n_envs=1, n_options=0, seed=0, env_id_base=0, enabled_mask=0, n_threads=4, **hp):
    m = scg.load_map(map_name)
    kw = dict(HP)
    kw.update(hp)
    return sc_oracle.Oracle(m, SCALE, n_envs=n_envs, n_options=n_options, seed=seed, env_id_base=env_id_base,
                            enabled_mask=enabled_mask, n_threads=n_threads, **kw), m


def random_states(m, n, seed, vmax=2.0, near_walls=True):
    """Collision-free positions (some hugging obstacles) + velocities in [-vmax, vmax]."""
    rng = np.random.default_rng(seed)
    pos = m.sample_free(n, rng, margin=1.05 if near_walls else 2.0)
    v = rng.uniform(-vmax, vmax, (n, 2)).astype(np.float32)
    return pos[:, 0].copy(), pos[:, 1].copy(), v[:, 0].copy(), v[:, 1].copy()


def random_env_state(m, n, n_opt, seed, *, id_lo, id_hi, opt_steps_hi, max_episode_steps):
    """A running env batch as a dict of arrays: random_states' positions / velocities (vmax 1.5), option ids in [id_lo, id_hi]
    (out-of-range ids are part of some tests), option-step counters below opt_steps_hi, episode-step counters below
    max_episode_steps, random qcache. The draws and their order are fixed: tests pin their cases on them."""
    rng = np.random.default_rng(seed)
    x, y, vx, vy = random_states(m, n, seed, vmax=1.5)
    return dict(x=x, y=y, vx=vx, vy=vy,
                option_id=rng.integers(id_lo, id_hi + 1, n).astype(np.int32),
                opt_steps=rng.integers(0, opt_steps_hi, n).astype(np.int32),
                ep_steps=rng.integers(0, max_episode_steps, n).astype(np.int32),
                qcache=rng.standard_normal((5, n)).astype(np.float32))


def disc_weights(cx, cy, radius):
    uc, vc, r = 2 * cx - 1, 2 * cy - 1, 2 * radius
    w = np.zeros(8, np.float32)
    w[:6] = [r * r - uc * uc - vc * vc, 2 * uc, 2 * vc, -1.0, 0.0, -1.0]
    return w


def chain_classifiers(m, n_options):
    """A synthetic skill chain: option 1's initiation set is a disc round the goal, option k's a
    larger disc (so that I_k contains I_(k-1)) — stands in for fitted classifiers."""
    clf = np.zeros((n_options + 1, 8), np.float32)
    tx, ty, _ = m.target
    for k in range(1, n_options + 1):
        clf[k] = disc_weights(tx, ty, 0.18 + 0.17 * (k - 1))
    return clf


def wide_chain(m, n_opt):
    """Nested discs round the goal, of radius 0.3 (option 1) up to 1.05 (the last option): options are entered everywhere."""
    clf = np.zeros((n_opt + 1, 8), np.float32)
    tx, ty, _ = m.target
    for k in range(1, n_opt + 1):
        clf[k] = disc_weights(tx, ty, 0.3 + 0.75 * (k - 1) / max(n_opt - 1, 1))
    return clf


SIBLING_PARENTS = [0, 0, 0, 1, 1, 2]


def sibling_tree(m):
    """(parents, clf [6][8]) of the sibling layout on map `m`: five discs whose initiation sets overlap, so that most states
    have several candidates (SPEC §14). Options 1 and 2 lead to the goal, 3 and 4 into option 1, 5 into option 2; (tx, ty) the
    target, s = +-1 pointing from it towards the map centre."""
    tx, ty = float(m.target[0]), float(m.target[1])
    sx, sy = (1.0 if tx < 0.5 else -1.0), (1.0 if ty < 0.5 else -1.0)
    clf = np.zeros((6, 8), np.float32)
    for k, (cx, cy, r) in enumerate([(tx, ty, 0.30), (tx + 0.10 * sx, ty + 0.10 * sy, 0.35), (0.5, 0.5, 0.45), (tx, 0.5, 0.50),
                                     (0.5, 0.5, 0.75)], start=1):
        clf[k] = disc_weights(cx, cy, r)
    return list(SIBLING_PARENTS), clf


def random_weights(n_vf, seed, std=1e-2):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_vf, 5, 1296)) * std).astype(np.float32)


def crossing_weights(n_vf, seed, noise=0.05):
    """Option weights of the root's scale plus noise: V_o and V_0 cross both ways."""
    W = random_weights(n_vf, seed, std=0.1)
    rng = np.random.default_rng(seed + 1000)
    W[1:] = W[0] + (rng.standard_normal(W[1:].shape) * noise).astype(np.float32)
    return W


def entry_state(m, n, n_opt, seed, run_share, max_episode_steps):
    """Random states; a share of the envs runs a random option, the others none or stay out of one (-k)."""
    rng = np.random.default_rng(seed)
    st = sc_oracle.new_state(n, m)
    st["x"][:], st["y"][:], st["vx"][:], st["vy"][:] = random_states(m, n, seed, vmax=1.5)
    run = rng.random(n) < run_share
    st["option_id"][:] = np.where(run, rng.integers(1, n_opt + 1, n), -rng.integers(0, n_opt + 1, n))
    st["opt_steps"][:] = rng.integers(0, 10, n)
    st["ep_steps"][:] = rng.integers(0, max_episode_steps, n)
    st["qcache"][:] = rng.standard_normal((5, n)).astype(np.float32)
    return st


def oracle_state(st_np, m):
    """sc_oracle.new_state seated with a dict of arrays (random_env_state's)."""
    st = sc_oracle.new_state(len(st_np["x"]), m)
    for f, v in st_np.items():
        st[f][...] = v
    return st


def copy_state(st):
    return {f: np.array(st[f], copy=True) for f in EnvState.FIELDS}


def fourier_reference(x, y, vx, vy):
    """float64 cos(pi c.s_hat) in canonical feature order."""
    s = np.stack([x, y, vx * 0.25 + 0.5, vy * 0.25 + 0.5], 1).astype(np.float64)
    idx = np.arange(1296)
    c = np.stack([(idx // 6 ** (3 - d)) % 6 for d in range(4)], 1).astype(np.float64)
    return np.cos(np.pi * s @ c.T)


def dense_map(n_side=6, size=0.035):
    """A synthetic map with many small square obstacles (16 + 4 n_side^2 edges): exercises the 4-word candidate
    masks (> 128 edges) and lanes with more than three candidate edges (overflow path of the HIP physics)."""
    lines = ["ball 0.015", "target 0.93 0.07 0.03", "start 0.07 0.93",
             "polygon 0.0 0.0 0.0 0.01 1.0 0.01 1.0 0.0", "polygon 0.0 0.0 0.01 0.0 0.01 1.0 0.0 1.0",
             "polygon 0.0 1.0 0.0 0.99 1.0 0.99 1.0 1.0", "polygon 1.0 1.0 0.99 1.0 0.99 0.0 1.0 0.0"]
    for i in range(n_side):
        for j in range(n_side):
            cx, cy = 0.16 + 0.136 * i, 0.16 + 0.136 * j
            lines.append(f"polygon {cx - size} {cy - size} {cx + size} {cy - size} {cx + size} {cy + size} {cx - size} {cy + size}")
    return scg.parse_map("\n".join(lines), "dense_synthetic")


def hub_map(n_spokes=12, r_in=0.035, r_out=0.30, half_width=0.006):
    """Thin spokes radiating from the centre (16 + 4 n_spokes edges): a ball near the hub has a dozen or more edges
    within reach at once — more than the (env, edge) pair form of the HIP physics takes per env (> 8: its per-lane
    loop) — and the balls around it have 3..8 (pair runs of every length, several groups of 64 pairs per wave)."""
    lines = ["ball 0.02", "target 0.9 0.1 0.04", "start 0.5 0.5 0.1 0.9 0.5 0.5",
             "polygon 0.0 0.0 0.0 0.01 1.0 0.01 1.0 0.0", "polygon 0.0 0.0 0.01 0.0 0.01 1.0 0.0 1.0",
             "polygon 0.0 1.0 0.0 0.99 1.0 0.99 1.0 1.0", "polygon 1.0 1.0 0.99 1.0 0.99 0.0 1.0 0.0"]
    for k in range(n_spokes):
        t = 2 * np.pi * (k + 0.5) / n_spokes
        c, s_ = np.cos(t), np.sin(t)
        pts = [(0.5 + r_in * c - half_width * s_, 0.5 + r_in * s_ + half_width * c),
               (0.5 + r_out * c - half_width * s_, 0.5 + r_out * s_ + half_width * c),
               (0.5 + r_out * c + half_width * s_, 0.5 + r_out * s_ - half_width * c),
               (0.5 + r_in * c + half_width * s_, 0.5 + r_in * s_ - half_width * c)]
        lines.append("polygon " + " ".join(f"{px:.6f} {py:.6f}" for px, py in pts))
    return scg.parse_map("\n".join(lines), f"hub_{n_spokes}")


_BORDER = ["polygon 0.0 0.0 0.0 0.01 1.0 0.01 1.0 0.0", "polygon 0.0 0.0 0.01 0.0 0.01 1.0 0.0 1.0",
           "polygon 0.0 1.0 0.0 0.99 1.0 0.99 1.0 1.0", "polygon 1.0 1.0 0.99 1.0 0.99 0.0 1.0 0.0"]


def _poly(pts):
    return "polygon " + " ".join(f"{float(px)!r} {float(py)!r}" for px, py in pts)


def edge_count_map(n_edges, radius=0.01):
    """A synthetic map of exactly `n_edges` edges (16 border edges, then squares on an 8 x 8 grid and, where n_edges - 16 is
    not a multiple of 4, one regular polygon of 5..7 vertices in the last slot). Every obstacle is convex and stands alone,
    so every edge can be hit from outside: the edges at the mask-word boundaries (63 / 64, 127 / 128, 255) included."""
    k = n_edges - 16
    assert 4 <= k <= 240
    q, r = divmod(k, 4)
    sizes = [4] * q if r == 0 else [4] * (q - 1) + [4 + r]
    lines = [f"ball {radius}", "target 0.955 0.955 0.02", "start 0.92 0.08"] + _BORDER
    for s, nv in enumerate(sizes):
        cx, cy = 0.1 + 0.1 * (s % 8), 0.1 + 0.1 * (s // 8)
        ph = np.pi / 4 if nv == 4 else 0.3
        rad = 0.02 * np.sqrt(2) if nv == 4 else 0.025
        lines.append(_poly([(cx + rad * np.cos(ph + 2 * np.pi * i / nv), cy + rad * np.sin(ph + 2 * np.pi * i / nv))
                            for i in range(nv)]))
    m = scg.parse_map("\n".join(lines), f"edges_{n_edges}")
    assert m.n_edges == n_edges
    return m


def edge_normals(m):
    """Unit outward normals [n_edges, 2] (float64) of the convex obstacles of a map: from each polygon's centroid."""
    out = []
    for poly in m.polygons:
        p = poly.astype(np.float64)
        c = p.mean(0)
        for i in range(len(p)):
            a, b = p[i], p[(i + 1) % len(p)]
            e = b - a
            nrm = np.array([e[1], -e[0]]) / np.hypot(*e)
            if np.dot(nrm, (a + b) / 2 - c) < 0:
                nrm = -nrm
            out.append(nrm)
    return np.array(out)


def edge_hit_state(m, j, gap, speed=1.0, along=0.5):
    """A ball at `gap` radii (float64) outside edge j, opposite the point at fraction `along` of the edge, moving head-on into
    it at `speed`: (x, y, vx, vy) float32 scalars."""
    E = m.edges.astype(np.float64)[j]
    nrm = edge_normals(m)[j]
    p = E[0:2] + along * E[2:4] + nrm * float(m.radius) * (1.0 + gap)
    v = -nrm * speed
    return np.float32(p[0]), np.float32(p[1]), np.float32(v[0]), np.float32(v[1])


def pocket_map(pockets, radius=0.02, target=(0.5, 0.5, 0.03), name="pockets"):
    """Pockets of thin triangles round given ball positions. `pockets`: list of (cx, cy, sides), sides a list of
    (angle, distance, half_length) in radians / ball radii: a triangle whose long edge faces (cx, cy) at `distance` along
    `angle`, `half_length` to either side, with its apex behind it (away from the pocket centre, far enough that the two
    short edges are no nearer to the centre than the long edge's endpoints). Used to give a ball an exact number of
    candidate edges of the HIP physics and to place edges that are candidates but can never be intercepted."""
    R = radius
    lines = [f"ball {R}", f"target {target[0]} {target[1]} {target[2]}", f"start {target[0]} {target[1] - 0.1}"] + _BORDER
    for cx, cy, sides in pockets:
        for ang, dist, half in sides:
            c, s = np.cos(ang), np.sin(ang)
            d, hl = dist * R, half * R
            depth = max(0.5 * d, hl * hl / d + 0.2 * R)
            lines.append(_poly([(cx + d * c - hl * s, cy + d * s + hl * c), (cx + (d + depth) * c, cy + (d + depth) * s),
                                (cx + d * c + hl * s, cy + d * s - hl * c)]))
    return scg.parse_map("\n".join(lines), name)


# ---- host restatement of the HIP physics' candidate pruning (an acceleration outside the arithmetic contract, SPEC §1.3 last
# paragraph). Restated from the code, not from the SPEC: the refined reach of pinball_wave_prepare (scg_device.hpp) and the
# cell-mask reach of scg_set_map (scg_kernels.hip). If either changes in the code, change it here.
CELL_G = 32
REFINE_A, REFINE_B = 1.02, 1.10                       # rr = fmaf(1.10f, |v|, 1.02f); candidate if edge_d2 <= R2 rr^2
CELL_VMAX = 2.0 * np.sqrt(2.0) * 1.001                # scg_set_map: vmax of the cell-mask reach
CELL_SLACK = 1.01                                     # ... R (1.02 + 1.10 vmax) * 1.01 + half a cell diagonal + 1e-6
PCAP = 8                                              # candidate edges per env that the (env, edge) pair form takes


def cell_reach(R):
    return float(R) * (REFINE_A + REFINE_B * CELL_VMAX) * CELL_SLACK + 0.5 * np.sqrt(2.0) / CELL_G + 1e-6


def cell_of(x, y):
    """The kernel's cell of a position: (int)(x * 32.0f), clamped to 0..31."""
    cx = np.clip((np.asarray(x, np.float32) * np.float32(CELL_G)).astype(np.int64), 0, CELL_G - 1)
    cy = np.clip((np.asarray(y, np.float32) * np.float32(CELL_G)).astype(np.int64), 0, CELL_G - 1)
    return cx, cy


def kernel_candidates(m, x, y, vx, vy, action, margin=0.0):
    """Candidate-edge mask [n, n_edges] of the HIP physics for pre-step states, in float64: edges of the cell mask (within
    cell_reach of the cell centre) that lie within R (1.02 + 1.10 |v|) of the ball, |v| after the impulse and the clip.
    With margin > 0, also asserts that no edge lies within a factor 1 +- margin of either boundary (so that binary32
    rounding cannot change the count)."""
    from phys64 import DV, VMAX, seg_dist
    a = np.asarray(action)
    vx = np.clip(np.asarray(vx, np.float32).astype(np.float64) + np.where(a == 0, DV, np.where(a == 2, -DV, 0.0)), -VMAX, VMAX)
    vy = np.clip(np.asarray(vy, np.float32).astype(np.float64) + np.where(a == 1, DV, np.where(a == 3, -DV, 0.0)), -VMAX, VMAX)
    R = float(m.radius)
    px, py = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    reach = R * (REFINE_A + REFINE_B * np.hypot(vx, vy))[:, None]
    d = seg_dist(m.edges, px, py)
    cx, cy = cell_of(x, y)
    dc = seg_dist(m.edges, (cx + 0.5) / CELL_G, (cy + 0.5) / CELL_G)
    cr = cell_reach(R)
    if margin > 0:
        assert not np.any(np.abs(d / reach - 1.0) < margin), "a state lies within the margin of the refined reach"
        assert not np.any((d <= reach) & (np.abs(dc / cr - 1.0) < margin)), "a cell centre lies within the margin of the cell-mask reach"
    return (d <= reach) & (dc <= cr)


def pair_groups(counts):
    """The run-pushing rule of pinball_wave_prepare for one wave of 64 envs: envs with 1..PCAP candidates take runs of
    consecutive slots in lane order, and a run that would straddle a group of 64 slots starts the next group. Returns
    (groups, pad slots) of the wave."""
    p, pad = 0, 0
    for c in counts:
        if not 1 <= c <= PCAP:
            continue
        if p // 64 != (p + c - 1) // 64:
            nxt = (p // 64 + 1) * 64
            pad += nxt - p
            p = nxt
        p += c
    return -(-p // 64), pad
