"""Host model of SPEC §16.1 (the feature Gram's pinned order) for the tests: a correctly rounded binary32 fma in numpy and
the two-level chains on the oracle's features.

`fma32(a, b, c)` is fmaf: the product of two binary32 values is exact in binary64 (48 <= 53 bits), TwoSum gives the exact
error of the binary64 sum p + c, the sum is rounded to odd when inexact, and one rounding to binary32 finishes it: correct
because 53 >= 2 * 24 + 2. The plain binary64 expression float32(a * b + c) rounds twice and is not fmaf in general
(tests/test_gram_host.py holds both to libm's fmaf).

`gram(phi, offsets, rows, cols)` and `rhs(phi, yv, offsets)` are §16.1 on phi [n][1296] (the oracle's features): per
segment and slab of SLAB samples one fma chain per entry from +0, the slab sums added in order. A 1296 x 1296 chain costs
seconds per 64 samples, so the model takes index lists.

Whole matrices at size go through the lattice. `lattice_states` draws x, y from {0, 0.5, 1} and vx, vy from {-2, 0, 2}: the
oracle's features of such a state are exactly -1, +-0 or +1 (tests/test_gram_host.py holds that), so a sum of their products over
fewer than 2^24 samples is an integer every partial sum of which is exact: any order gives the float64 matmul, and a chain
that starts at +0 never gives -0. `chain(left, right, offsets, lattice)` is §16.1's two levels for a segment whose slabs are
each a prefix of lattice samples followed by real-valued ones: the slab's P starts as the integer matmul of the prefix (+ 0.0:
+0 where it vanishes), runs the fma32 chain over the tail, and the slab sums are added in order. `lattice_gram` and
`lattice_rhs` are A and b on it (yv integer-valued on the lattice part); tests/cross_gram_model.py's `lattice_cross` is C.

`scalar_targets` is SPEC §16.2 for one env as a plain loop over Trajectory.segments' rule, the yardstick of
valuefit.returns_to_go."""
import numpy as np

SLAB = 1024
NF = 1296


def fma32(a, b, c):
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((np.atleast_1d(s).view(np.uint64).reshape(np.shape(s)) & np.uint64(1)) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return np.asarray(s).astype(np.float32)


def slabs(lo, hi):
    return [(s, min(s + SLAB, hi)) for s in range(lo, hi, SLAB)]


def gram(phi, offsets, rows, cols):
    """A_g[rows][cols] for every segment: float32 [n_seg][len(rows)][len(cols)]."""
    phi = np.asarray(phi, np.float32)
    rows, cols = np.asarray(rows), np.asarray(cols)
    out = np.zeros((len(offsets) - 1, len(rows), len(cols)), np.float32)
    for g in range(len(offsets) - 1):
        for lo, hi in slabs(int(offsets[g]), int(offsets[g + 1])):
            P = np.zeros(out.shape[1:], np.float32)
            for n in range(lo, hi):
                P = fma32(phi[n, rows][:, None], phi[n, cols][None, :], P)
            out[g] = out[g] + P
    return out


def rhs(phi, yv, offsets):
    """b_g, all 1296 entries: float32 [n_seg][1296]."""
    phi, yv = np.asarray(phi, np.float32), np.asarray(yv, np.float32)
    out = np.zeros((len(offsets) - 1, phi.shape[1]), np.float32)
    for g in range(len(offsets) - 1):
        for lo, hi in slabs(int(offsets[g]), int(offsets[g + 1])):
            P = np.zeros(phi.shape[1], np.float32)
            for n in range(lo, hi):
                P = fma32(phi[n], yv[n], P)
            out[g] = out[g] + P
    return out


def chain_bound(phi, offsets):
    """The derived bound on |A_g - float64 Gram| per entry, [n_seg][1296][1296]: (1024 + n_slabs) 2^-24 sum_n |phi_i phi_j| (1 + 2^-10),
    the standard chain bound for each of the two levels; and the float64 Gram itself."""
    p64 = np.asarray(phi, np.float32).astype(np.float64)
    ref, bound = [], []
    for g in range(len(offsets) - 1):
        seg = p64[int(offsets[g]): int(offsets[g + 1])]
        n_slabs = len(slabs(int(offsets[g]), int(offsets[g + 1])))
        ref.append(seg.T @ seg)
        bound.append((SLAB + n_slabs) * 2.0 ** -24 * (np.abs(seg).T @ np.abs(seg)) * (1 + 2.0 ** -10))
    return np.stack(ref), np.stack(bound)


def gram_states(n, seed):
    """The GPU tests' states: seeded uniform positions, velocities in [-2, 2] with the exact corners 0, 1, +-2 among them."""
    rng = np.random.default_rng(seed)
    s = [rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32),
         rng.uniform(-2, 2, n).astype(np.float32), rng.uniform(-2, 2, n).astype(np.float32)]
    corners = np.array([0.0, 1.0, 2.0, -2.0], np.float32)
    for d in (2, 3):
        at = rng.choice(n, min(n, 8), replace=False)
        s[d][at] = corners[rng.integers(0, 4, len(at))]
    return s


def index_set(macro=96, seed=5):
    """48 feature indices: the tile edges 0, 15, 16, 17, 1279, 1280, 1295, both sides of every macro-tile edge (`macro` features a side), a few
    other tile edges, and seeded others."""
    must = {0, 15, 16, 17, 1279, 1280, 1295, 63, 64, 1215, 1216}
    for e in range(macro, NF, macro):
        must |= {e - 1, e}
    rng = np.random.default_rng(seed)
    rest = [int(i) for i in rng.permutation(NF) if int(i) not in must]
    return np.array(sorted(must | set(rest[: 48 - len(must)])), np.int64)


LATTICE_POS, LATTICE_VEL = (0.0, 0.5, 1.0), (-2.0, 0.0, 2.0)


def lattice_states(n, seed):
    """Seeded states on the lattice: positions from {0, 0.5, 1}, velocities from {-2, 0, 2} (features exactly -1, +-0 or +1)."""
    rng = np.random.default_rng(seed)
    pos, vel = np.array(LATTICE_POS, np.float32), np.array(LATTICE_VEL, np.float32)
    return [pos[rng.integers(0, 3, n)], pos[rng.integers(0, 3, n)], vel[rng.integers(0, 3, n)], vel[rng.integers(0, 3, n)]]


def mixed_states(runs, seed):
    """(states, lattice mask) of `runs` = [(count, on the lattice?)] in sample order: lattice_states where the mask is set,
    gram_states elsewhere."""
    lat = np.concatenate([np.full(int(c), bool(on)) for c, on in runs])
    return [np.where(lat, a, b) for a, b in zip(lattice_states(len(lat), seed), gram_states(len(lat), seed + 1))], lat


def chain(left, right, offsets, lattice=None):
    """out[g][i][j] = §16.1's two levels over sum_n left[n][i] right[n][j], float32 [n_seg][I][J], whole matrices. `lattice` [n]
    marks the samples whose operands are integer-valued: in every slab they must come first; the slab's P starts as their
    float64 matmul (exact: asserted integers, absolute sums below 2^24; + 0.0 makes a vanishing sum +0 as the chain from +0
    does) and then runs the fma32 chain over the others. Without `lattice` this is the plain chain."""
    left, right = np.asarray(left, np.float32), np.asarray(right, np.float32)
    lat = np.zeros(len(left), bool) if lattice is None else np.asarray(lattice, bool)
    out = np.zeros((len(offsets) - 1, left.shape[1], right.shape[1]), np.float32)
    for g in range(len(offsets) - 1):
        for lo, hi in slabs(int(offsets[g]), int(offsets[g + 1])):
            k = hi if lat[lo:hi].all() else lo + int(np.argmin(lat[lo:hi]))
            assert not lat[k:hi].any(), "the lattice samples of a slab must be its prefix"
            l64, r64 = left[lo:k].astype(np.float64), right[lo:k].astype(np.float64)
            assert np.all(l64 == np.rint(l64)) and np.all(r64 == np.rint(r64)), "lattice operands must be integers"
            if k > lo:
                assert np.abs(l64).sum(axis=0).max() * np.abs(r64).max() < 2.0 ** 24
            P = (l64.T @ r64 + 0.0).astype(np.float32)
            for n in range(k, hi):
                P = fma32(left[n][:, None], right[n][None, :], P)
            out[g] = out[g] + P
    return out


def lattice_gram(phi, offsets, lattice=None, rows=None, cols=None):
    """A_g of `chain`, whole (rows / cols None) or on index lists."""
    phi = np.asarray(phi, np.float32)
    return chain(phi if rows is None else phi[:, rows], phi if cols is None else phi[:, cols], offsets, lattice)


def lattice_rhs(phi, yv, offsets, lattice=None):
    """b_g of `chain`, all 1296 entries; yv integer-valued where `lattice` is set."""
    return chain(phi, np.asarray(yv, np.float32)[:, None], offsets, lattice)[:, :, 0]


def scalar_targets(reward, vf, term, gamma, r_succ):
    """§16.2 for one env, a plain loop: (g, y) per row; row 0 (the begin row) gets 0. The executions are Trajectory.segments'
    runs: a run ends before a row of another vf, after a row with term != 0 and with the env's last row (a one-episode record
    holds its done row last). Every row of a run of an option that ends in SUCCESS gets the bonus, discounted to the run's end."""
    L = len(reward)
    g, y = [0.0] * (L + 1), [0.0] * L
    for j in range(L - 1, 0, -1):
        g[j] = float(reward[j]) + gamma * g[j + 1]
    start = 0
    for j in range(L):
        if j + 1 == L or vf[j + 1] != vf[j] or term[j] != 0:
            for i in range(max(start, 1), j + 1):
                y[i] = g[i]
                if vf[i] >= 1 and term[j] == 1:             # SCG_TRIAL_SUCCESS
                    y[i] += gamma ** (j - i) * r_succ
            start = j + 1
    return g[:L], y
