"""Host model of SPEC §22.1 (the weighted feature Gram) for the tests: the operands u = fl32(rw * phi) and t = fl32(rw * Y), one
binary32 multiply each (numpy's float32 product: round to nearest, subnormals kept), and then tests/gram_model.py's chains on
them, unchanged: `gram` / `rhs` on index lists, `chain` for whole matrices. Nothing of §16.1's order is spelt again here."""
import numpy as np

import gram_model as GM


def operands(phi, rw, Y=None):
    """(u [n][F], t [n][C] or None): every feature, and every target of Y [C][n], times the sample's root weight."""
    phi, rw = np.asarray(phi, np.float32), np.asarray(rw, np.float32)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        u = (rw[:, None] * phi).astype(np.float32)
        t = None if Y is None else (rw[:, None] * np.asarray(Y, np.float32).T).astype(np.float32)
    return u, t


def gram(phi, rw, offsets, rows, cols):
    """A_g[rows][cols] of the weighted Gram: gram_model.gram on u."""
    return GM.gram(operands(phi, rw)[0], offsets, rows, cols)


def rhs(phi, rw, Y, offsets):
    """B_g[c], all entries, float32 [n_seg][C][F]: gram_model.rhs on (u, t_c) per target."""
    u, t = operands(phi, rw, Y)
    return np.stack([GM.rhs(u, t[:, c], offsets) for c in range(t.shape[1])], axis=1)


def whole(phi, rw, Y, offsets, lattice=None):
    """(A [n_seg][F][F], B [n_seg][C][F]) whole, by gram_model.chain: `lattice` marks the samples whose u and t are integers."""
    u, t = operands(phi, rw, Y)
    return GM.chain(u, u, offsets, lattice), np.swapaxes(GM.chain(u, t, offsets, lattice), 1, 2)


def prefix_chain(left, right, ns):
    """{n: the one-segment chain over sum_{m < n} left[m][i] right[m][j], float32 [I][J]} for every n of `ns`, from ONE pass over
    the samples: a one-segment result at n samples is a prefix of the pass at max(ns). The GPU tests tie it to gram_model.gram and
    gram_model.rhs, which it must equal by bits."""
    left, right = np.asarray(left, np.float32), np.asarray(right, np.float32)
    out, tot, P = {}, np.zeros((left.shape[1], right.shape[1]), np.float32), None
    for n in range(max(ns)):
        if n % GM.SLAB == 0:
            P = np.zeros_like(tot)
        P = GM.fma32(left[n][:, None], right[n][None, :], P)
        if (n + 1) % GM.SLAB == 0:
            tot = tot + P
        if n + 1 in ns:
            out[n + 1] = tot.copy() if (n + 1) % GM.SLAB == 0 else tot + P
    return out


def prefix_rhs(phi, rw, Y, ns):
    """{n: rhs(phi[:n], rw[:n], Y[:, :n], [0, n])[0]}, float32 [C][F]."""
    u, t = operands(phi, rw, Y)
    return {n: v.T.copy() for n, v in prefix_chain(u, t, ns).items()}


def prefix_gram(phi, rw, ns, rows, cols):
    """{n: gram(phi[:n], rw[:n], [0, n], rows, cols)[0]}."""
    u = operands(phi, rw)[0]
    return prefix_chain(u[:, rows], u[:, cols], ns)


def no_subnormal_partial_sum(phi, rw, Y, offsets, rows, cols):
    """Does every partial sum of the chains of A[rows][cols] and of all of B, and every operand, stay normal or exactly 0? The
    power-of-two identities (rw = 2 gives 4 A) hold by bits only then."""
    u, t = operands(phi, rw, Y)
    tiny = np.finfo(np.float32).tiny
    ok = lambda v: bool(np.all((v == 0) | (np.abs(v) >= tiny)))
    good = ok(u) and (t is None or ok(t))
    for g in range(len(offsets) - 1):
        for lo, hi in GM.slabs(int(offsets[g]), int(offsets[g + 1])):
            P = np.zeros((len(rows), len(cols)), np.float32)
            Q = None if t is None else np.zeros((t.shape[1], u.shape[1]), np.float32)
            for n in range(lo, hi):
                P = GM.fma32(u[n, rows][:, None], u[n, cols][None, :], P)
                good = good and ok(P)
                if t is not None:
                    Q = GM.fma32(u[n][None, :], t[n][:, None], Q)
                    good = good and ok(Q)
    return good
