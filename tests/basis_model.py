"""Host model of SPEC §18 (the Fourier basis of order p in {3, 5, 7}) for the tests: numpy binary32 on gram_model.fma32.

`features(order, x, y, vx, vy)` is §18.1 operation for operation — §3's sincospi, the power chain, the AB / CD rows, the final
fma — with P1 = order + 1 in the place of 6; every product and sum is a binary32 numpy operation, every fused step is fma32. At
order 5 it is the oracle's `features` by bits (tests/test_basis_host.py). `embed(q, p)` is the index map of the order-q features
into order p's; `values(order, phi, V)` is §18.3's two-level chain on given features; `edge_states()` are finite states at
binary32's edges. The Gram of order p needs no model of its own: gram_model's `gram`, `chain`, `lattice_gram` and `lattice_rhs`
take features of any width."""
import numpy as np

from gram_model import fma32

ORDERS = (3, 5, 7)
S = [np.float32(float.fromhex(h)) for h in ("0x1.921fb6p+1", "-0x1.4abbcep+2", "0x1.466bc6p+1", "-0x1.32d2ccp-1", "0x1.507834p-4")]
C = [np.float32(float.fromhex(h)) for h in ("-0x1.3bd3ccp+2", "0x1.03c1f0p+2", "-0x1.55d3c8p+0", "0x1.e1f506p-3", "-0x1.a6d1f2p-6")]


def num_features(order):
    assert order in ORDERS
    return (order + 1) ** 4


def sincospi(t):
    """SPEC §3's sincospi on a binary32 array: (cos, sin) of pi t."""
    t = np.atleast_1d(np.asarray(t, np.float32))
    with np.errstate(all="ignore"):
        n = np.rint(t + t)
        r = fma32(n, np.float32(-0.5), t)
        z = r * r
        sp = fma32(z, S[4], S[3])
        for k in (2, 1, 0):
            sp = fma32(z, sp, S[k])
        sp = sp * r
        cp = fma32(z, C[4], C[3])
        for k in (2, 1, 0):
            cp = fma32(z, cp, C[k])
        cp = fma32(z, cp, np.float32(1.0))
        small = np.isfinite(n) & (np.abs(n) < 2.0 ** 31)
        q = np.where(small, np.where(small, n, 0).astype(np.int64) & 3, 0)
    c = np.where(q == 0, cp, np.where(q == 1, -sp, np.where(q == 2, -cp, sp)))
    s = np.where(q == 0, sp, np.where(q == 1, cp, np.where(q == 2, -sp, -cp)))
    return c.astype(np.float32), s.astype(np.float32)


def cmul(a, b):
    (ar, ai), (br, bi) = a, b
    with np.errstate(all="ignore"):
        return fma32(-ai, bi, ar * br), fma32(ar, bi, ai * br)


def tables(order, x, y, vx, vy):
    """(AB, CD) of §18.1: each a pair (re, im) of float32 [P2][n]."""
    P1 = order + 1
    x, y, vx, vy = (np.atleast_1d(np.asarray(v, np.float32)) for v in (x, y, vx, vy))
    sh = [x, y, fma32(vx, np.float32(0.25), np.float32(0.5)), fma32(vy, np.float32(0.25), np.float32(0.5))]
    z1 = [sincospi(v) for v in sh]
    one = (np.ones_like(x), np.zeros_like(x))

    def table(zrow, zcol):                                   # entry c_row P1 + c_col = Z_col^c_col times Z_row^1, c_row times
        pw = [one, zcol]
        for _ in range(2, P1):
            pw.append(cmul(pw[-1], zcol))
        ent = list(pw)
        for c in range(1, P1):
            ent += [cmul(ent[(c - 1) * P1 + j], zrow) for j in range(P1)]
        return np.stack([e[0] for e in ent]), np.stack([e[1] for e in ent])

    return table(z1[0], z1[1]), table(z1[2], z1[3])


def features(order, x, y, vx, vy, idx=None):
    """phi float32 [n][F], f = c12 P2 + c34: fma(-AB[c12].im, CD[c34].im, AB[c12].re CD[c34].re); with `idx` only those features, [n][len(idx)]."""
    (abr, abi), (cdr, cdi) = tables(order, x, y, vx, vy)
    if idx is not None:
        P2 = (order + 1) ** 2
        a, c = np.asarray(idx) // P2, np.asarray(idx) % P2
        with np.errstate(all="ignore"):
            return np.ascontiguousarray(fma32(-abi[a], cdi[c], abr[a] * cdr[c]).T)
    with np.errstate(all="ignore"):
        phi = fma32(-abi[:, None, :], cdi[None, :, :], abr[:, None, :] * cdr[None, :, :])      # [c12][c34][n]
    return np.ascontiguousarray(phi.reshape(num_features(order), -1).T)


def coefficients(order):
    P1 = order + 1
    f = np.arange(P1 ** 4)
    return np.stack([(f // P1 ** (3 - d)) % P1 for d in range(4)], 1)


def embed(q, p):
    """The order-p index of every order-q feature (q <= p), in order q's feature order."""
    c = coefficients(q)
    P1 = p + 1
    return ((c[:, 0] * P1 + c[:, 1]) * P1 + c[:, 2]) * P1 + c[:, 3]


def values(order, phi, V):
    """§18.3: out float32 [m][n]; out = +0; per c12 ascending T = +0, T = fma(V[r][c12 P2 + c34], phi_f, T) over c34 ascending, out = out + T."""
    P2 = (order + 1) ** 2
    phi, V = np.asarray(phi, np.float32), np.asarray(V, np.float32)
    out = np.zeros((V.shape[0], phi.shape[0]), np.float32)
    for c12 in range(P2):
        T = np.zeros_like(out)
        for c34 in range(P2):
            f = c12 * P2 + c34
            T = fma32(V[:, f][:, None], phi[:, f][None, :], T)
        with np.errstate(all="ignore"):
            out = out + T
    return out


def edge_states():
    """Finite states at binary32's edges: the 16 grid corners, -0.0, subnormals of both signs, positions outside [0, 1], velocities
    outside [-2, 2], and 2^24 + 2 and 1e30 in each coordinate in turn."""
    c = [(x, y, vx, vy) for x in (0.0, 1.0) for y in (0.0, 1.0) for vx in (-2.0, 2.0) for vy in (-2.0, 2.0)]
    sub = 1e-41
    c += [(-0.0,) * 4, (sub,) * 4, (-sub,) * 4, (-0.25, 1.5, 2.8, -2.8), (1.5, -0.25, -8.0, 8.0)]
    for v in (2.0 ** 24 + 2, 1e30):
        for d in range(4):
            t = [0.25, 0.75, 0.5, -1.0]
            t[d] = v
            c.append(tuple(t))
    out = np.array(c, np.float32)
    return [np.ascontiguousarray(out[:, d]) for d in range(4)]
