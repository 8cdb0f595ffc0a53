"""Host model of SPEC §23.1 / §23.2 for the tests. `terms(orc, z, label)` is §23.1: p from the oracle's sigmoid (SPEC §6's, one
binary32 operation at a time), then e = l - p, q = 1 - p, s = p q and rw = sqrt(s) as numpy binary32 operations (each correctly
rounded). `hessian` is weighted_gram_model.gram on the order's phi (the operands u = fl32(rw phi) on gram_model's chains), `gradient`
gram_model.rhs on the UNWEIGHTED phi against e. Nothing of §16.1's order is spelt again here.

`Float64Gram` is what initfit.irls_fit's `gram=` takes on the host: materialised float64 features, the logistic terms and the two
moments in float64 — the reference the device path is held to, not a model of its bits."""
import numpy as np

import gram_model as GM
import weighted_gram_model as WM

SATURATION = [0.0, -0.0, 87.0, -87.0, 88.0, -88.0, np.inf, -np.inf, np.nan, 2.0 ** -140, -2.0 ** -140]
P_FLOOR = float.fromhex("0x1.666d0ep-126")                            # sigmoid of a NaN and of every z <= -87


def sigmoid(orc, z):
    """The oracle's sigmoid on a binary32 array: one call per distinct bit pattern."""
    z = np.ascontiguousarray(z, np.float32).reshape(-1)
    bits, inv = np.unique(z.view(np.uint32), return_inverse=True)
    vals = np.array([orc.sigmoid(float(v)) for v in bits.view(np.float32)], np.float32)
    return vals[inv]


def terms(orc, z, label):
    """(p, rw, e) float32 [n] of §23.1."""
    p = sigmoid(orc, z)
    l = np.where(np.asarray(label).reshape(-1) != 0, np.float32(1), np.float32(0)).astype(np.float32)
    e = (l - p).astype(np.float32)
    q = (np.float32(1) - p).astype(np.float32)
    s = (p * q).astype(np.float32)
    return p, np.sqrt(s).astype(np.float32), e


def hessian(phi, rw, offsets, rows, cols):
    """H_g[rows][cols]: §22.1's operands on `phi` (features of any order, [n][F]), §16.1's chains."""
    return WM.gram(phi, rw, offsets, rows, cols)


def gradient(phi, e, offsets):
    """grad_g, all F entries: gram_model.rhs on the unweighted phi."""
    return GM.rhs(phi, e, offsets)


class Float64Gram:
    """irls_fit's `gram=` on the host: phi float64 [n][F] materialised; values(w) = phi w (float64, no binary32 anywhere),
    hessian_gradient(z) = (phi^T diag(p (1 - p)) phi, phi^T (l - p))."""

    def __init__(self, phi, label):
        self.phi = np.asarray(phi, np.float64)
        self.l = (np.asarray(label).reshape(-1) != 0).astype(np.float64)

    def values(self, w):
        return self.phi @ np.asarray(w, np.float64)

    def hessian_gradient(self, z):
        z = np.asarray(z, np.float64)
        p = np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))
        return (self.phi * (p * (1.0 - p))[:, None]).T @ self.phi, self.phi.T @ (self.l - p)


# ---------------------------------------------------------------------------------------------------- SPEC §23.3's test problems

def problem(name, n=4096, seed=11):
    """(states [4][n] float32, labels bool [n]) of the fit tests' three problems: "bernoulli" — labels drawn from sigmoid(w* . phi)
    of a known order-3 row —, "disc" — inside a disc in position — and "vx" — vx > 0, vx uniform in [-2, 2): invisible to a
    position classifier."""
    import basis_model as BM
    rng = np.random.default_rng(seed)
    s = [rng.uniform(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32),
         rng.uniform(-2, 2, n).astype(np.float32), rng.uniform(-2, 2, n).astype(np.float32)]
    if name == "bernoulli":
        w = np.zeros(256)
        c = BM.coefficients(3)
        low = np.flatnonzero(c.sum(1) <= 2)
        w[low] = rng.normal(0, 1.0, len(low)) / np.maximum(1.0, np.sqrt((c[low] ** 2).sum(1)))
        z = BM.features(3, *s).astype(np.float64) @ w
        lab = rng.uniform(0, 1, n) < 1.0 / (1.0 + np.exp(-z))
    elif name == "disc":
        lab = (s[0] - 0.4) ** 2 + (s[1] - 0.55) ** 2 < 0.3 ** 2
    elif name == "vx":
        lab = s[2] > 0
    else:
        raise ValueError(name)
    return s, lab
