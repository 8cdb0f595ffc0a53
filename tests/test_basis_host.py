"""SPEC §18's host model (tests/basis_model.py), without a GPU: at order 5 it is the oracle's `features` by bits, the orders
embed into one another by bits, lattice states give exactly -1, +-0 or +1 at order 7, `values` is the pinned two-level chain,
and the binding knows the orders."""
import numpy as np
import pytest

import basis_model as BM
import gram_model as GM
from bits import assert_bits_equal
from util import make_oracle


@pytest.fixture(scope="module")
def states():
    return GM.gram_states(300, 11)


@pytest.fixture(scope="module")
def phis(states):
    return {p: BM.features(p, *states) for p in BM.ORDERS}


def test_order_five_is_the_oracles_features_by_bits(states, phis):
    orc, _ = make_oracle("pinball_simple")
    assert phis[5].shape == (300, 1296)
    assert_bits_equal(phis[5], orc.features(*states), msg="order 5 on gram_states:")
    e = BM.edge_states()
    assert_bits_equal(BM.features(5, *e), orc.features(*e), msg="order 5 on the finite edge states:")


def test_sincospi_is_the_oracles_by_bits():
    orc, _ = make_oracle("pinball_simple")
    t = np.concatenate([np.linspace(-3, 3, 241), [0.125, 1e-41, -1e-41, 2.0 ** 24 + 2, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31]]).astype(np.float32)
    c, s = BM.sincospi(t)
    want = np.array([orc.sincospi(float(v)) for v in t], np.float32)
    assert_bits_equal(c, want[:, 0], msg="cos:")
    assert_bits_equal(s, want[:, 1], msg="sin:")


@pytest.mark.parametrize("q,p", [(3, 5), (5, 7), (3, 7)])
def test_a_lower_order_embeds_by_bits(phis, q, p):
    idx = BM.embed(q, p)
    assert len(idx) == BM.num_features(q) and len(set(idx.tolist())) == len(idx) and idx[0] == 0 and idx.max() < BM.num_features(p)
    assert np.array_equal(BM.coefficients(p)[idx], BM.coefficients(q))
    assert_bits_equal(phis[p][:, idx], phis[q], msg=f"order {q} inside order {p}:")
    e = BM.edge_states()
    assert_bits_equal(BM.features(p, *e)[:, idx], BM.features(q, *e), msg=f"order {q} inside order {p}, edge states:")


def test_embedding_composes():
    assert np.array_equal(BM.embed(5, 7)[BM.embed(3, 5)], BM.embed(3, 7))
    assert np.array_equal(BM.embed(5, 5), np.arange(1296))


@pytest.mark.parametrize("order", BM.ORDERS)
def test_lattice_states_give_exact_features(order):
    phi = BM.features(order, *GM.lattice_states(500, 3))
    assert phi.shape == (500, BM.num_features(order))
    assert np.isin(phi, [-1.0, 0.0, 1.0]).all() and (phi == -1).any() and (phi == 0).any()
    assert np.all(phi[:, 0] == 1)


def test_features_are_the_cosines(states, phis):
    """Against float64 cos(pi c . s^): the model is the basis it claims to be (sincospi is accurate to 3e-7, up to 14 chained products)."""
    sh = np.stack([states[0], states[1], states[2] * 0.25 + 0.5, states[3] * 0.25 + 0.5], 1).astype(np.float64)
    for p in BM.ORDERS:
        want = np.cos(np.pi * sh @ BM.coefficients(p).T.astype(np.float64))
        assert np.abs(phis[p] - want).max() < 2e-5, p


@pytest.mark.parametrize("order", BM.ORDERS)
def test_values_follow_the_pinned_two_level_chain(order, phis):
    """Against a scalar loop of SPEC §18.3 with libm-checked fma32 on a few samples, and against float64 on all of them."""
    rng = np.random.default_rng(order)
    F, P2 = BM.num_features(order), (order + 1) ** 2
    V = rng.standard_normal((3, F)).astype(np.float32)
    V[0, :5] = [0.0, -0.0, 1e-41, 1e30, -1e30]
    phi = phis[order][:40]
    got = BM.values(order, phi, V)
    assert got.shape == (3, 40) and got.dtype == np.float32
    for r, n in ((0, 0), (1, 7), (2, 39)):
        out = np.float32(0.0)
        for c12 in range(P2):
            T = np.float32(0.0)
            for c34 in range(P2):
                T = GM.fma32(V[r, c12 * P2 + c34], phi[n, c12 * P2 + c34], T).reshape(())[()]
            out = np.float32(out + T)
        assert_bits_equal(got[r, n:n + 1], np.array([out], np.float32), msg=f"order {order}, row {r}, sample {n}:")
    ref = V[1:].astype(np.float64) @ phi.astype(np.float64).T
    # the standard chain bound of the two levels: (P2 + P2) roundings of 2^-24 on sum |V phi|
    bound = 2 * P2 * 2.0 ** -24 * 1.01 * (np.abs(V[1:]).astype(np.float64) @ np.abs(phi).astype(np.float64).T)
    assert np.all(np.abs(got[1:] - ref) <= bound)
    # a vanishing sum is +0: the chain starts at +0 and -0 + +0 = +0
    z = BM.values(order, phi[:2], np.full((1, F), -0.0, np.float32))
    assert_bits_equal(z, np.zeros((1, 2), np.float32), msg="all -0 weights:")


def test_binding_knows_the_orders(pkg):
    from skill_chaining_with_graphs_amd import _lib
    from skill_chaining_with_graphs_amd.core import fourier_scale_table
    assert _lib.BASIS_ORDERS == BM.ORDERS == (3, 5, 7)
    assert [_lib.basis_features(p) for p in BM.ORDERS] == [256, 1296, 4096]
    with pytest.raises(_lib.ScgError):
        _lib.basis_features(4)
    for name in ("scg_basis_features", "scg_basis_gram", "scg_basis_values"):
        assert name in pkg.EXPORTED_SYMBOLS
    for q, p in ((3, 5), (5, 7)):
        assert np.array_equal(fourier_scale_table(p)[BM.embed(q, p)], fourier_scale_table(q))
