"""The random draws of SPEC §2 at any 64-bit run identity (host only).

A few lines on top of ref64.philox4x32_10 / ref64.mulhi32 (pinned by the published vectors), independent of the oracle and of
the kernels: how the three 64-bit quantities — the seed, the step counter t and the global env id g = env_id_base + e — are split
into the 32-bit words of Philox4x32-10. Python ints in, no float64 on the way (2^53 would silently round a 64-bit counter).

WIDE_T / WIDE_SEED / wide_bases(n) are the grid the wide-identity tests share: values that put non-zero bits into every upper
word, and env ids that cross bit 31 and the 2^32 wrap inside one batch (and inside one block of it)."""
import numpy as np

from ref64 import mulhi32, philox4x32_10

M32 = 0xFFFFFFFF

WIDE_T = (5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 40, 2 ** 63, 2 ** 64 - 1)
WIDE_SEED = (3, 2 ** 32 - 1, 2 ** 32 + 3, 2 ** 63 + 3, 2 ** 64 - 1)


def wide_bases(n):
    """env_id_base values for n envs: ids cross bit 31 / the 2^32 wrap in the middle of the batch."""
    return (0, 2 ** 31 - n // 2, 2 ** 32 - n // 2, 2 ** 32, 2 ** 40 + 3)


def grid(n):
    """(seed, env_id_base, t) triples: every value of each axis with the other two at a wide value, and at a small one."""
    small = (WIDE_SEED[0], 0, WIDE_T[0])
    wide = (2 ** 63 + 3, 2 ** 32 - n // 2, 2 ** 32 + 5)
    out = []
    for other in (wide, small):
        out += [(s, other[1], other[2]) for s in WIDE_SEED]
        out += [(other[0], b, other[2]) for b in wide_bases(n)]
        out += [(other[0], other[1], t) for t in WIDE_T]
    return list(dict.fromkeys(out))


def words(seed, t):
    """(c1, c2, k0, k1) of SPEC §2 for a seed and a step counter, both taken mod 2^64."""
    seed, t = int(seed) % 2 ** 64, int(t) % 2 ** 64
    return t & M32, t >> 32, seed & M32, seed >> 32


def draws(g, seed, t, n_starts):
    """For global env ids g (Python ints, any sign) and scalars seed, t: (explore_u float64 — exact, a multiple of 2^-24 —,
    a_rand, start), each an array over g. c0 = g mod 2^32 (two's complement for a negative g)."""
    c0 = np.array([int(v) % 2 ** 32 for v in g], np.uint64)
    c1, c2, k0, k1 = words(seed, t)
    n = len(c0)
    u0, u1, u2, _ = philox4x32_10(c0, np.full(n, c1, np.uint64), np.full(n, c2, np.uint64), np.zeros(n, np.uint64), k0, k1)
    explore_u = (u0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return explore_u, mulhi32(u1, 5), mulhi32(u2, n_starts)


def draws_batch(env_id_base, n, seed, t, n_starts):
    """draws() for the n envs of a shard at env_id_base."""
    return draws([int(env_id_base) + e for e in range(n)], seed, t, n_starts)


def seven_start_map():
    """An empty synthetic map with 7 distinct start positions (not a power of two: mulhi32 is really exercised), all far from
    the goal in the opposite corner."""
    import skill_chaining_with_graphs_amd as scg
    from util import _BORDER
    starts = " ".join(f"{0.1 + 0.1 * i:.2f} {0.15 + 0.05 * (i % 3):.2f}" for i in range(7))
    m = scg.parse_map("\n".join(["ball 0.02", "target 0.9 0.9 0.04", "start " + starts] + _BORDER), "seven_starts")
    assert len(m.starts) == 7 and len({(float(x), float(y)) for x, y in m.starts}) == 7
    return m
