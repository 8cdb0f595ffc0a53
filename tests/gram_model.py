"""Host model of SPEC §16.1 (the feature Gram's pinned order) for the tests: a correctly rounded binary32 fma in numpy and
the two-level chains on the oracle's features.

`fma32(a, b, c)` is fmaf: the product of two binary32 values is exact in binary64 (48 <= 53 bits), TwoSum gives the exact
error of the binary64 sum p + c, the sum is rounded to odd when inexact, and one rounding to binary32 finishes it: correct
because 53 >= 2 * 24 + 2. The plain binary64 expression float32(a * b + c) rounds twice and is not fmaf in general
(tests/test_gram_host.py holds both to libm's fmaf).

`gram(phi, offsets, rows, cols)` and `rhs(phi, yv, offsets)` are §16.1 on phi [n][1296] (the oracle's features): per
segment and slab of SLAB samples one fma chain per entry from +0, the slab sums added in order. A 1296 x 1296 chain costs
seconds per 64 samples, so the model takes index lists.

`scalar_targets` is SPEC §16.2 for one env as a plain loop, the yardstick of valuefit.returns_to_go."""
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


def scalar_targets(reward, vf, term, gamma, r_succ):
    """§16.2 for one env, a plain loop: (g, y) per row; row 0 (the begin row) gets 0."""
    L = len(reward)
    g, y = [0.0] * (L + 1), [0.0] * L
    for j in range(L - 1, 0, -1):
        g[j] = float(reward[j]) + gamma * g[j + 1]
    for j in range(1, L):
        y[j] = g[j]
        if vf[j] >= 1:
            tau = j
            while tau + 1 < L and vf[tau + 1] == vf[j]:
                tau += 1
            if term[tau] == 1:                              # SCG_TRIAL_SUCCESS
                y[j] += gamma ** (tau - j) * r_succ
    return g[:L], y
