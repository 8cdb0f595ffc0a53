"""SPEC §16 on the host: the yardsticks of tests/test_gpu_gram.py and test_gpu_value_fit.py are themselves held to something —
gram_model.fma32 to libm's fmaf, the lattice shortcut of whole matrices (gram_model.chain) to the plain chains, valuefit.returns_to_go
to a scalar loop and to hand-made records whose bonus is known exactly, valuefit.ridge_solve to its normal equations."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import gram_model as GM
from bits import assert_bits_equal
from util import SCALE, make_oracle
from skill_chaining_with_graphs_amd import valuefit

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def libm_fmaf(a, b, c):
    return np.array([_libm.fmaf(float(u), float(v), float(w)) for u, v, w in zip(a, b, c)], np.float32)


def f32_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def test_fma32_is_fmaf_on_random_triples():
    rng = np.random.default_rng(0)
    n = 60000
    a, b, c = (rng.standard_normal(n).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, n).astype(np.float32) for _ in range(3))
    c[::3] = -(a[::3] * b[::3])                                      # cancellation: the sum's low bits decide
    assert_bits_equal(GM.fma32(a, b, c), libm_fmaf(a, b, c), msg="fma32 on random triples:")


def midpoint_cases(rng, n):
    """a b + c within 2^-30 (relative) of a binary32 midpoint: p = a b exact in binary64, m the midpoint of the two binary32
    neighbours of p, c = float32(m - p) and the same c one unit in its last place either side (by bit pattern)."""
    a = (rng.integers(2 ** 23, 2 ** 24, n)).astype(np.float32) * np.float32(2.0) ** rng.integers(-30, 8, n).astype(np.float32)
    b = (rng.integers(2 ** 23, 2 ** 24, n) | 1).astype(np.float32) * np.float32(2.0) ** rng.integers(-30, 8, n).astype(np.float32)
    p = a.astype(np.float64) * b.astype(np.float64)
    lo = p.astype(np.float32)
    lo = np.where(lo.astype(np.float64) > p, np.nextafter(lo, np.float32(-np.inf)), lo)
    m = (lo.astype(np.float64) + np.nextafter(lo, np.float32(np.inf)).astype(np.float64)) / 2
    c = (m - p).astype(np.float32)
    out = []
    for d in (-1, 0, 1):
        cb = (c.view(np.uint32).astype(np.int64) + d).astype(np.uint32).view(np.float32)
        out.append((a, b, cb))
    near = np.abs((p + c.astype(np.float64)) - m) <= 2.0 ** -30 * np.abs(m)
    assert near.all()
    return out


def test_fma32_is_fmaf_next_to_midpoints_where_the_binary64_expression_is_not():
    rng = np.random.default_rng(1)
    naive_wrong = 0
    for a, b, c in midpoint_cases(rng, 4000):
        want = libm_fmaf(a, b, c)
        assert_bits_equal(GM.fma32(a, b, c), want, msg="fma32 next to a midpoint:")
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        naive_wrong += int(np.sum(naive.view(np.uint32) != want.view(np.uint32)))
    assert naive_wrong > 0, "the cases do not separate fmaf from the twice-rounded binary64 expression"


def test_fma32_subnormal_results_and_signed_zeros():
    rng = np.random.default_rng(2)
    n = 4000
    a = rng.standard_normal(n).astype(np.float32) * np.float32(2.0 ** -70)
    b = rng.standard_normal(n).astype(np.float32) * np.float32(2.0 ** -65)
    c = f32_bits(rng.integers(0, 2 ** 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31))      # subnormals of both signs
    got = GM.fma32(a, b, c)
    assert_bits_equal(got, libm_fmaf(a, b, c), msg="fma32, subnormal results:")
    assert np.any((np.abs(got) < np.float32(2.0 ** -126)) & (got != 0))
    z, nz, one = np.float32(0.0), np.float32(-0.0), np.float32(1.5)
    tri = [(z, one, z), (z, one, nz), (nz, one, nz), (nz, one, z), (z, z, z), (nz, z, nz), (one, one, -one * one), (-one, one, one * one),
           (nz, nz, nz), (z, nz, z), (np.float32(2.0 ** -100), np.float32(2.0 ** -100), z), (np.float32(-2.0 ** -100), np.float32(2.0 ** -100), z),
           (np.float32(-2.0 ** -100), np.float32(2.0 ** -100), nz)]
    a, b, c = (np.array(v, np.float32) for v in zip(*tri))
    assert_bits_equal(GM.fma32(a, b, c), libm_fmaf(a, b, c), msg="fma32, signed zeros:")


# ---------------------------------------------------------------------------------------------------- §16.1's model

@pytest.fixture(scope="module")
def phi_small():
    orc, _ = make_oracle("pinball_simple")
    s = GM.gram_states(1100, 11)
    return orc.features(*s)


def test_model_gram_is_symmetric_by_bits_and_inside_the_chain_bound(phi_small):
    idx = GM.index_set()
    off = [0, 3, 3, 1100]                                            # a short, an empty and a two-slab segment
    A = GM.gram(phi_small, off, idx, idx)
    assert A.shape == (3, 48, 48) and np.array_equal(A.view(np.uint32), A.transpose(0, 2, 1).view(np.uint32))
    assert not A[1].any() and not np.signbit(A[1]).any()
    ref, bound = GM.chain_bound(phi_small, off)
    sub = np.ix_(range(3), idx, idx)
    assert np.all(np.abs(A.astype(np.float64) - ref[sub]) <= bound[sub])
    assert A[2][0, 0] == 1097 and A[0][0, 0] == 3                    # phi_0 = 1


def test_model_rhs_chain(phi_small):
    yv = np.random.default_rng(3).standard_normal(1100).astype(np.float32)
    b = GM.rhs(phi_small, yv, [0, 5, 1100])
    ref = phi_small[5:].astype(np.float64).T @ yv[5:].astype(np.float64)
    bound = (GM.SLAB + 2) * 2.0 ** -24 * (np.abs(phi_small[5:].astype(np.float64)).T @ np.abs(yv[5:].astype(np.float64))) * (1 + 2.0 ** -10)
    assert np.all(np.abs(b[1] - ref) <= bound)
    want0 = np.float32(0)
    for v in yv[:5]:
        want0 = GM.fma32(np.float32(1), v, want0)
    assert b[0][0] == want0


# ---------------------------------------------------------------------------------------------------- the lattice shortcut

def test_lattice_features_are_exactly_minus_one_zero_or_one():
    orc, _ = make_oracle("pinball_simple")
    pos, vel = np.array(GM.LATTICE_POS, np.float32), np.array(GM.LATTICE_VEL, np.float32)
    g = np.stack(np.meshgrid(pos, pos, vel, vel, indexing="ij"), -1).reshape(-1, 4)      # all 81 lattice states
    phi = orc.features(*(np.ascontiguousarray(g[:, d]) for d in range(4)))
    assert phi.shape == (81, NF) and np.isin(phi, [-1.0, 0.0, 1.0]).all()
    assert np.all(phi[:, 0] == 1) and {-1.0, 0.0, 1.0} == set(np.unique(phi))
    drawn = orc.features(*GM.lattice_states(500, 4))
    assert np.isin(drawn, [-1.0, 0.0, 1.0]).all() and len(np.unique(drawn, axis=0)) > 70           # the draw reaches most of the 81


# a segment of two slabs whose real-valued samples lie on both sides of the slab edge (950 lattice + 74 real | 40 real: gram's
# chunk edge at 960 and the slab edge at 1024 are inside real samples), an empty one, and 28 lattice + 9 real samples (the cross
# kernel's chunk edge at 32 inside the tail); the first two samples belong to no segment
MIXED_RUNS = [(2, False), (950, True), (114, False), (28, True), (9, False), (3, True)]
MIXED_OFF = [2, 1066, 1066, 1103]


def test_lattice_shortcut_equals_the_plain_chains_on_the_index_set():
    orc, _ = make_oracle("pinball_simple")
    s, lat = GM.mixed_states(MIXED_RUNS, 40)
    assert len(lat) == 1106 and lat.sum() == 981 and not lat[1100:1103].any()
    phi = orc.features(*s)
    idx = GM.index_set()
    yv = np.random.default_rng(41).standard_normal(len(lat)).astype(np.float32)
    yv[lat] = np.random.default_rng(42).integers(-3, 4, int(lat.sum())).astype(np.float32)
    assert_bits_equal(GM.lattice_gram(phi, MIXED_OFF, lat, idx, idx), GM.gram(phi, MIXED_OFF, idx, idx), msg="A by the shortcut:")
    assert_bits_equal(GM.lattice_rhs(phi, yv, MIXED_OFF, lat), GM.rhs(phi, yv, MIXED_OFF), msg="b by the shortcut:")
    assert_bits_equal(GM.lattice_gram(phi, MIXED_OFF, None, idx, idx), GM.gram(phi, MIXED_OFF, idx, idx), msg="A without a mask:")
    with pytest.raises(AssertionError):                              # a lattice sample behind a real one in its slab
        GM.lattice_gram(phi, [0, 1103], lat, idx[:2], idx[:2])
    with pytest.raises(AssertionError):                              # a real sample marked as a lattice one
        GM.lattice_gram(phi, [0, 2], np.ones(len(lat), bool), idx[:2], idx[:2])


def test_whole_matrix_of_one_sample_is_the_rounded_product():
    """One sample a segment: the chain from +0 is one fma, float32(float64(phi_i) float64(phi_j)) with -0 turned into +0."""
    orc, _ = make_oracle("pinball_simple")
    s = GM.gram_states(3, 6)
    s[2][1], s[3][1] = 0.0, 2.0                                      # a corner velocity: features that are exactly +-0 and +-1
    phi = orc.features(*s)
    A = GM.lattice_gram(phi, [0, 1, 2, 3])
    p = phi.astype(np.float64)
    want = (p[:, :, None] * p[:, None, :]).astype(np.float32) + np.float32(0)
    assert A.shape == (3, NF, NF) and (phi[1] == 0).any()
    assert_bits_equal(A, want, msg="one-sample A:")
    assert_bits_equal(A[:, 0, :], phi + np.float32(0), msg="row 0 of a one-sample A:")


# ---------------------------------------------------------------------------------------------------- §16.2: returns_to_go

SUCCESS, EPISODE_END, LEFT, TIMEOUT = 1, 2, 3, 4
scalar_targets = GM.scalar_targets


def episode(steps):
    """[(reward, vf, term)] of the steps -> the env's rows with the begin row in front."""
    return [(0.0, 0, 0)] + list(steps)


HAND = {
    "success mid-episode": episode([(-1, 0, 0), (-5, 1, 0), (-1, 1, 0), (-5, 1, SUCCESS), (-1, 0, 0), (10000, 0, 0)]),
    "left initiation": episode([(-5, 2, 0), (-5, 2, LEFT), (-1, 0, 0), (-1, 0, 0)]),
    "cut by the episode's end (time limit)": episode([(-1, 0, 0), (-5, 1, 0), (-5, 1, 0), (-5, 1, EPISODE_END)]),
    "two runs of one option apart": episode([(-5, 1, 0), (-5, 1, SUCCESS), (-1, 0, 0), (-5, 1, 0), (-1, 1, LEFT), (-1, 0, 0)]),
    "goal ending inside an option": episode([(-5, 1, 0), (10000, 1, SUCCESS)]),
    "option timeout then another option": episode([(-5, 2, 0), (-5, 2, TIMEOUT), (-5, 1, 0), (-5, 1, SUCCESS), (-1, 0, 0)]),
    "len 1": episode([]),
    "len 2": episode([(10000, 0, 0)]),
    "len 2 in an option": episode([(-5, 1, SUCCESS)]),
}


@pytest.mark.parametrize("gamma,r_succ", [(0.99, 100.0), (0.9, 0.0), (1.0, -7.5)])
def test_returns_to_go_equals_the_scalar_loop(gamma, r_succ):
    envs = list(HAND.values())
    off = np.concatenate([[0], np.cumsum([len(e) for e in envs])]).astype(np.int64)
    flat = {"offsets": off, "reward": np.array([r for e in envs for r, _, _ in e], np.float32),
            "vf": np.array([v for e in envs for _, v, _ in e], np.uint8), "term": np.array([t for e in envs for _, _, t in e], np.uint8)}
    got = valuefit.returns_to_go(flat, gamma, r_succ)
    assert got["g"].dtype == np.float64 and np.array_equal(got["offsets"], off)
    for i, (name, e) in enumerate(HAND.items()):
        g, y = scalar_targets(*zip(*e), gamma, r_succ)
        sl = slice(off[i], off[i + 1])
        assert np.allclose(got["g"][sl], g, rtol=1e-14, atol=0), name
        assert np.allclose(got["y"][sl], y, rtol=1e-13, atol=0), name
        assert list(got["sample"][sl]) == [False] + [True] * (len(e) - 1), name
    # the cases say what they are meant to: the bonus reaches the first run of "two runs" and not its second, nor a run that did not succeed
    g, y = scalar_targets(*zip(*HAND["two runs of one option apart"]), 0.99, 100.0)
    assert y[1] - g[1] == pytest.approx(99.0) and y[2] - g[2] == 100.0 and y[4] == g[4] and y[5] == g[5]
    g, y = scalar_targets(*zip(*HAND["left initiation"]), 0.99, 100.0)
    assert y == g


# Executions inside one run of a vf (SPEC §16.2's tau): (vf, term) per step and the bonus each row must get at gamma = 0.5,
# r_option_success = 100, the begin row in front. A power of 0.5 times 100 is exact, so with rewards of 0 y IS the bonus.
INTERRUPTED = 5
EXECUTIONS = {
    "a timeout inside the initiation set, entered again at once, then success":
        ([(0, 0), (1, 0), (1, TIMEOUT), (1, 0), (1, SUCCESS), (0, 0), (0, 0)], [0, 0, 0, 0, 50, 100, 0, 0]),
    "timeout, timeout, success":
        ([(2, 0), (2, TIMEOUT), (2, TIMEOUT), (2, 0), (2, 0), (2, SUCCESS)], [0, 0, 0, 0, 25, 50, 100]),
    "an interrupted run that is entered again":
        ([(1, 0), (1, INTERRUPTED), (1, 0), (1, SUCCESS), (0, 0)], [0, 0, 0, 50, 100, 0]),
    "option 1 followed directly by option 2":
        ([(1, 0), (1, SUCCESS), (2, 0), (2, 0), (2, SUCCESS), (1, 0), (1, LEFT)], [0, 50, 100, 25, 50, 100, 0, 0]),
    "a success followed by a run that the record's end cuts":
        ([(1, SUCCESS), (1, 0), (1, 0)], [0, 100, 0, 0]),
    "the episode ends inside an execution":
        ([(0, 0), (2, 0), (2, TIMEOUT), (2, 0), (2, EPISODE_END)], [0, 0, 0, 0, 0, 0]),
    "a begin row only": ([], [0]),
}


def exec_flat(rewards=None):
    envs = [[(0, 0)] + steps for steps, _ in EXECUTIONS.values()]
    off = np.concatenate([[0], np.cumsum([len(e) for e in envs])]).astype(np.int64)
    flat = {"offsets": off, "vf": np.array([v for e in envs for v, _ in e], np.uint8), "term": np.array([t for e in envs for _, t in e], np.uint8)}
    flat["reward"] = np.zeros(int(off[-1]), np.float32) if rewards is None else rewards(int(off[-1]))
    return flat


def test_the_bonus_goes_to_the_execution_that_succeeded():
    flat = exec_flat()
    got = valuefit.returns_to_go(flat, 0.5, 100.0)
    off = flat["offsets"]
    for i, (name, (steps, bonus)) in enumerate(EXECUTIONS.items()):
        sl = slice(off[i], off[i + 1])
        assert got["y"][sl].tolist() == [float(v) for v in bonus], name
        assert not got["g"][sl].any(), name
        g, y = scalar_targets(flat["reward"][sl], flat["vf"][sl], flat["term"][sl], 0.5, 100.0)
        assert y == [float(v) for v in bonus] and not any(g), name
    # the issue's record by itself, and no envs at all
    one = {"offsets": np.array([0, 7]), "reward": np.zeros(7, np.float32), "vf": np.array([0, 1, 1, 1, 1, 0, 0], np.uint8),
           "term": np.array([0, 0, 4, 0, 1, 0, 0], np.uint8)}
    assert valuefit.returns_to_go(one, 0.5, 100.0)["y"].tolist() == [0, 0, 0, 50, 100, 0, 0]
    none = valuefit.returns_to_go({"offsets": np.zeros(1, np.int64), "reward": np.zeros(0, np.float32), "vf": np.zeros(0, np.uint8),
                                   "term": np.zeros(0, np.uint8)}, 0.5, 100.0)
    assert all(len(none[k]) == 0 for k in ("g", "y", "sample")) and none["y"].dtype == np.float64 and none["offsets"].tolist() == [0]


@pytest.mark.parametrize("gamma,r_succ", [(0.99, 100.0), (float(np.float32(0.99)), 100.0), (1.0, -7.5)])
def test_executions_with_rewards_equal_the_scalar_loop_by_bits(gamma, r_succ):
    flat = exec_flat(lambda n: np.random.default_rng(7).choice(np.array([-1, -5, 10000], np.float32), n))
    got = valuefit.returns_to_go(flat, gamma, r_succ)
    off = flat["offsets"]
    for i, name in enumerate(EXECUTIONS):
        sl = slice(off[i], off[i + 1])
        g, y = scalar_targets(flat["reward"][sl], flat["vf"][sl], flat["term"][sl], gamma, r_succ)
        assert np.array_equal(got["g"][sl], g) and np.array_equal(got["y"][sl], y), name
        assert (np.asarray(y) != np.asarray(g)).sum() == np.count_nonzero(EXECUTIONS[name][1]), name


# ---------------------------------------------------------------------------------------------------- §16.3: ridge_solve

NF = 1296
RESIDUAL_RATIO_MEASURED = 1.513e-4     # the largest of the 20 systems below as first measured (profiles/r22_value_fit_checks.txt)
RESIDUAL_RATIO_BOUND = 8 * RESIDUAL_RATIO_MEASURED


def ridge_system(seed, n_rows=300):
    rng = np.random.default_rng(seed)
    A, b, n = np.zeros((5, NF, NF), np.float32), np.zeros((5, NF), np.float32), np.zeros(5, np.int64)
    for a in range(5):
        m = n_rows * (a + 1)
        X = (rng.standard_normal((m, NF)) * SCALE[None, :]).astype(np.float32)
        X[:, 0] = 1
        G = X.astype(np.float64).T @ X.astype(np.float64)
        A[a] = np.tril(G).astype(np.float32) + np.tril(G, -1).astype(np.float32).T
        b[a] = (X.astype(np.float64).T @ rng.standard_normal(m) * 100).astype(np.float32)
        n[a] = m
    return A, b, n


def residual_ratio(A, b, n, ridge, delta):
    out = []
    for a in range(len(n)):
        M = A[a].astype(np.float64) + np.diag(ridge * max(int(n[a]), 1) / SCALE.astype(np.float64) ** 2)
        res = np.linalg.norm(M @ delta[a] - b[a].astype(np.float64))
        out.append(res / (np.finfo(np.float64).eps * NF * (np.linalg.norm(M) * np.linalg.norm(delta[a]) + np.linalg.norm(b[a].astype(np.float64)))))
    return max(out)


def test_ridge_solve_satisfies_its_normal_equations():
    worst = 0.0
    for seed in range(4):                                            # 4 x 5 actions = 20 systems
        A, b, n = ridge_system(seed)
        delta = valuefit.ridge_solve(A, b, n, 1e-3, SCALE)
        assert delta.dtype == np.float64 and np.isfinite(delta).all()
        worst = max(worst, residual_ratio(A, b, n, 1e-3, delta))
    print(f"ridge_solve: largest residual ratio over 20 systems {worst:.4g} (bound {RESIDUAL_RATIO_BOUND:.4g})")
    assert worst <= RESIDUAL_RATIO_BOUND


def test_ridge_solve_empty_action_triangles_and_penalty():
    A, b, n = ridge_system(9, n_rows=100)
    n[2] = 0
    delta = valuefit.ridge_solve(A, b, n, 1e-3, SCALE)
    assert not delta[2].any() and delta[[0, 1, 3, 4]].any(axis=1).all()
    assert np.array_equal(A, A.transpose(0, 2, 1))
    assert np.array_equal(valuefit.ridge_solve(A.transpose(0, 2, 1).copy(), b, n, 1e-3, SCALE), delta)      # either triangle of a symmetric A
    up = A.copy()
    up[:, np.triu_indices(NF, 1)[0], np.triu_indices(NF, 1)[1]] = 7.0      # only the lower triangle is read
    assert np.array_equal(valuefit.ridge_solve(up, b, n, 1e-3, SCALE), delta)
    # no data at all: Delta_f = b_f scale_f^2 / (ridge n); feature 0 (scale 1) is penalised with ridge n
    Z = np.zeros((1, NF, NF), np.float32)
    bb = np.ones((1, NF), np.float32)
    d = valuefit.ridge_solve(Z, bb, [50], 0.5, SCALE)
    assert d[0, 0] == pytest.approx(1 / (0.5 * 50), rel=1e-15)
    assert np.allclose(d[0], SCALE.astype(np.float64) ** 2 / (0.5 * 50), rtol=1e-14, atol=0)
