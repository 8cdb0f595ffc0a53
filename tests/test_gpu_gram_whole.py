"""scg_feature_gram and scg_feature_cross_gram (SPEC §16.1, §17.1) over the WHOLE 1296 x 1296 matrix, by bits, and at the sizes the
kernels were written for. tests/test_gpu_gram.py and test_gpu_cross_gram.py compare bits on 48 x 48 indices; here every entry of A,
b and C is pinned:

- small segments of real-valued states against the plain fma32 chain (both kernels' chunk edges, ragged tails, an empty segment);
- segments whose slabs are a prefix of lattice samples and a tail of real-valued ones (tests/gram_model.py's `chain`): the exact
  integer prefix makes three slabs affordable, and every entry's bits still depend on the slab restart and on the order of the tail;
- pure lattice segments at n near 40 000 (33 slabs in one segment, 25 segments), against the float64 integer product;
- 64 single-sample segments (SCG_GRAM_MAX_SEGMENTS) over states at binary32's edges, against the rounded product of the device's
  own scg_fourier_features;
- scg_fourier_features past its grid of 8192 workgroups, against the oracle.

Every comparison is by bits (a NaN matches a NaN of any payload where one is expected) or of exact integers."""
import gc

import numpy as np
import pytest
import torch

import cross_gram_model as CM
import gram_model as GM
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd.core import ScgContext
from bits import assert_bits_equal
from gpu_util import dev
from util import HP, make_oracle

pytestmark = pytest.mark.gpu

NF = 1296
BUILDS = (256, 64)


@pytest.fixture(scope="module", autouse=True)
def cached_blocks_go_back():
    """64 segments of A are a 430 MB block: torch's cached blocks are handed back when the module is done, so that later modules find
    the allocator as they would without this one (tests/test_gpu_robustness.py counts on a 64 MiB request getting a segment of its own)."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def rig():
    orc, m = make_oracle("pinball_simple")
    ctx = {b: ScgContext(64, 0, m, device=0, block_envs=b, **HP) for b in BUILDS}
    yield dict(orc=orc, ctx=ctx)
    for c in ctx.values():
        c.close()


def same_bits(got, want, msg, allow_nan=False):
    """assert_bits_equal, with the common case (no difference) decided by one comparison of the words."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        assert_bits_equal(got, want, allow_nan=allow_nan, msg=msg)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def mixed_yv(lat, seed):
    """yv: integers in [-3, 3] on the lattice samples, seeded normal values with +-0, a subnormal and +-1e30 among them elsewhere."""
    rng = np.random.default_rng(seed)
    yv = rng.standard_normal(len(lat)).astype(np.float32)
    real = np.nonzero(~lat)[0]
    edge = np.array([0.0, -0.0, 1e-41, 1e30, -1e30], np.float32)
    yv[real[: len(edge)]] = edge[: len(real)]
    yv[lat] = rng.integers(-3, 4, int(lat.sum())).astype(np.float32)
    return yv


# ---------------------------------------------------------------------------------------------------- 1. small real-valued segments

def test_gram_of_small_real_segments_whole_matrix_by_bits(rig):
    """Sizes 3, 0, 66 from sample 1: gram's 64-sample chunk edge and a ragged tail of 2 (padded to 4)."""
    off, n = [1, 4, 4, 70], 71
    s = GM.gram_states(n, 61)
    yv = mixed_yv(np.zeros(n, bool), 62)
    phi = rig["orc"].features(*s)
    A, b = rig["ctx"][256].feature_gram([dev(v) for v in s], off, dev(yv))
    same_bits(host(A), GM.lattice_gram(phi, off), "A, every entry:")
    same_bits(host(b), GM.lattice_rhs(phi, yv, off), "b:")
    assert [float(v) for v in host(A)[:, 0, 0]] == [3, 0, 66]


def test_cross_gram_of_small_real_segments_whole_matrix_by_bits(rig):
    """Sizes 3, 0, 37 from sample 1: the cross kernel's 32-sample chunk edge and a tail of 5 (padded to 8)."""
    off, n = [1, 4, 4, 41], 42
    s, s2 = GM.gram_states(n, 63), GM.gram_states(n, 64)
    Cm = host(rig["ctx"][256].feature_cross_gram([dev(v) for v in s], [dev(v) for v in s2], off))
    same_bits(Cm, CM.lattice_cross(rig["orc"].features(*s), rig["orc"].features(*s2), off), "C, every entry:")
    assert [float(v) for v in Cm[:, 0, 0]] == [3, 0, 37] and not np.array_equal(Cm[2], Cm[2].T)


# ---------------------------------------------------------------------------------------------------- 2. lattice prefix + real tail

# sample 0 belongs to no segment; 1024 + 1024 lattice + 5 real samples (three slabs, the last ragged and all real); empty; 60 lattice +
# 9 real (the tail crosses gram's chunk edge at 64); empty; 28 lattice + 9 real (the tail crosses the cross kernel's chunk edge at 32)
MIXED_RUNS = [(1, False), (2048, True), (5, False), (60, True), (9, False), (28, True), (9, False), (2, True)]
MIXED_OFF = [1, 2054, 2054, 2123, 2123, 2160]


@pytest.fixture(scope="module")
def mixed(rig):
    (s, lat), (s2, lat2) = GM.mixed_states(MIXED_RUNS, 70), GM.mixed_states(MIXED_RUNS, 80)
    assert len(lat) == 2162 and np.array_equal(lat, lat2)
    return dict(s=s, s2=s2, lat=lat, yv=mixed_yv(lat, 72), phi=rig["orc"].features(*s), phi2=rig["orc"].features(*s2),
                sd=[dev(v) for v in s], sd2=[dev(v) for v in s2], want={})


def mixed_want(mixed, what):
    """The model's A, b or C of the mixed layout, computed once (23 whole-matrix fma32 steps each for A and C)."""
    w = mixed["want"]
    if what not in w:
        if what == "A":
            w["A"] = GM.lattice_gram(mixed["phi"], MIXED_OFF, mixed["lat"])
        elif what == "b":
            w["b"] = GM.lattice_rhs(mixed["phi"], mixed["yv"], MIXED_OFF, mixed["lat"])
        else:
            w["C"] = CM.lattice_cross(mixed["phi"], mixed["phi2"], MIXED_OFF, mixed["lat"])
    return w[what]


@pytest.mark.parametrize("build", BUILDS)
def test_gram_of_lattice_prefix_and_real_tail_whole_matrix_by_bits(rig, mixed, build):
    A, b = rig["ctx"][build].feature_gram(mixed["sd"], MIXED_OFF, dev(mixed["yv"]))
    A, b = host(A), host(b)
    same_bits(A, mixed_want(mixed, "A"), f"A, every entry, {build}-env build:")
    same_bits(b, mixed_want(mixed, "b"), f"b, {build}-env build:")
    assert [float(v) for v in A[:, 0, 0]] == [2053, 0, 69, 0, 37]


@pytest.mark.parametrize("build", BUILDS)
def test_cross_gram_of_lattice_prefix_and_real_tail_whole_matrix_by_bits(rig, mixed, build):
    Cm = host(rig["ctx"][build].feature_cross_gram(mixed["sd"], mixed["sd2"], MIXED_OFF))
    same_bits(Cm, mixed_want(mixed, "C"), f"C, every entry, {build}-env build:")
    assert [float(v) for v in Cm[:, 0, 0]] == [2053, 0, 69, 0, 37] and not np.array_equal(Cm[0], Cm[0].T)


# ---------------------------------------------------------------------------------------------------- 3. pure lattice at size

# 33 000 samples = 32 slabs + 232, then 24 uneven segments (six empty, three longer than a slab, one of exactly two slabs), from sample 3
SIZES_25 = [33000, 0, 1, 1100, 3, 0, 64, 5, 0, 33, 2100, 4, 0, 65, 7, 31, 0, 1024, 2, 150, 0, 63, 2048, 37, 12]
OFF_25 = [3] + [3 + int(v) for v in np.cumsum(SIZES_25)]
N_LATTICE = OFF_25[-1] + 8


@pytest.fixture(scope="module")
def lattice(rig):
    """s and s2 drawn independently and unevenly (s2 keeps to a part of the lattice), their features, integer yv."""
    assert len(SIZES_25) == 25 and SIZES_25.count(0) == 6 and 39000 < N_LATTICE < 41000 and 33000 == 32 * 1024 + 232
    s, s2 = GM.lattice_states(N_LATTICE, 90), GM.lattice_states(N_LATTICE, 91)
    rng = np.random.default_rng(92)
    s2[0] = np.where(rng.random(N_LATTICE) < 0.6, np.float32(0.5), s2[0])          # uneven: x2 = 0.5 on most samples ...
    s2[3] = np.where(rng.random(N_LATTICE) < 0.5, np.float32(2.0), s2[3])          # ... and vy2 = 2 on half of them
    yv = rng.integers(-3, 4, N_LATTICE).astype(np.float32)
    phi, phi2 = rig["orc"].features(*s), rig["orc"].features(*s2)
    assert np.isin(phi, [-1.0, 0.0, 1.0]).all() and np.isin(phi2, [-1.0, 0.0, 1.0]).all()
    return dict(sd=[dev(v) for v in s], sd2=[dev(v) for v in s2], yv=yv, p=phi.astype(np.float64), q=phi2.astype(np.float64))


def test_gram_of_forty_thousand_lattice_samples_is_the_integer_product(rig, lattice):
    A, b = rig["ctx"][256].feature_gram(lattice["sd"], OFF_25, dev(lattice["yv"]))
    A, b = host(A), host(b)
    y64 = lattice["yv"].astype(np.float64)
    for g in range(25):
        lo, hi = OFF_25[g], OFF_25[g + 1]
        p = lattice["p"][lo:hi]
        same_bits(A[g], (p.T @ p + 0.0).astype(np.float32), f"A of segment {g} ({hi - lo} samples):")
        same_bits(b[g], (p.T @ y64[lo:hi] + 0.0).astype(np.float32), f"b of segment {g} ({hi - lo} samples):")
        assert A[g][0, 0] == hi - lo
    assert np.abs(A[0]).max() == 33000 and np.abs(b[0]).max() > 0


def test_cross_gram_of_forty_thousand_lattice_samples_is_the_integer_product(rig, lattice):
    Cm = host(rig["ctx"][256].feature_cross_gram(lattice["sd"], lattice["sd2"], OFF_25))
    for g in range(25):
        lo, hi = OFF_25[g], OFF_25[g + 1]
        same_bits(Cm[g], (lattice["p"][lo:hi].T @ lattice["q"][lo:hi] + 0.0).astype(np.float32), f"C of segment {g} ({hi - lo} samples):")
        assert Cm[g][0, 0] == hi - lo
    for g in (0, 3, 10):
        assert not np.array_equal(Cm[g], Cm[g].T), g


# ---------------------------------------------------------------------------------------------------- 4., 5. edge states, the grid

N_FEATURES_RUNS = (8192, 8193, 20000)        # scg_fourier_features' grid is min(n, 8192) workgroups: one pass, a second pass of one, 2.4 passes


@pytest.fixture(scope="module")
def real20k(rig):
    s = GM.gram_states(max(N_FEATURES_RUNS), 71)
    return dict(s=s, phi=rig["orc"].features(*s))


@pytest.mark.parametrize("n", N_FEATURES_RUNS)
def test_features_past_the_grid_equal_the_oracle_by_bits(rig, real20k, n):
    got = host(rig["ctx"][256].features([dev(v[:n]) for v in real20k["s"]]))
    same_bits(got, real20k["phi"][:n], f"scg_fourier_features, n = {n}:")


def edge_states(fill):
    """64 states: the 16 grid corners; -0.0, subnormals of both signs, positions -0.25 and 1.5, velocities +-2.8 and +-8; 2^24 + 2, 1e30,
    +-inf and NaN in each coordinate in turn; `fill`'s first states up to 64."""
    c = [(x, y, vx, vy) for x in (0.0, 1.0) for y in (0.0, 1.0) for vx in (-2.0, 2.0) for vy in (-2.0, 2.0)]
    sub = 1e-41
    c += [(-0.0,) * 4, (sub,) * 4, (-sub,) * 4, (-0.25, 1.5, 2.8, -2.8), (1.5, -0.25, -8.0, 8.0)]
    for v in (2.0 ** 24 + 2, 1e30, np.inf, -np.inf, np.nan):
        for d in range(4):
            t = [0.25, 0.75, 0.5, -1.0]
            t[d] = v
            c.append(tuple(t))
    out = np.array(c, np.float32)
    k = _lib.GRAM_MAX_SEGMENTS - len(out)
    assert k > 0
    out = np.concatenate([out, np.stack([f[:k] for f in fill], 1)])
    return [np.ascontiguousarray(out[:, d]) for d in range(4)]


@pytest.fixture(scope="module")
def edges(rig, real20k):
    s = edge_states(real20k["s"])
    n = len(s[0])
    assert n == 64 == _lib.GRAM_MAX_SEGMENTS
    finite = np.all([np.isfinite(v) for v in s], axis=0)
    assert 0 < (~finite).sum() == 12 and float(np.float32(2.0 ** 24 + 2)) == 2.0 ** 24 + 2
    sd = [dev(v) for v in s]
    phi = host(rig["ctx"][256].features(sd))
    return dict(s=s, sd=sd, phi=phi, finite=finite, off=list(range(n + 1)))


def test_edge_state_features_equal_the_oracle_where_the_state_is_finite(rig, edges):
    f = edges["finite"]
    want = rig["orc"].features(*[np.ascontiguousarray(v[f]) for v in edges["s"]])
    same_bits(edges["phi"][f], want, "features of the finite edge states:")
    assert np.all(edges["phi"][:, 0] == 1)                            # phi_0 = 1 whatever the state
    assert np.isnan(edges["phi"][~f]).any(axis=1).all() and not np.isnan(edges["phi"][f]).any()


def one_sample_products(rig, edges, left, right, got, name):
    """Segment g holds sample g alone: every entry is fma(left_i, right_j, +0) = the product rounded once (a -0 becomes +0); NaN
    wherever the product is NaN."""
    for g in range(len(left)):
        with np.errstate(invalid="ignore"):
            want = (left[g].astype(np.float64)[:, None] * right[g].astype(np.float64)[None, :]).astype(np.float32) + np.float32(0)
        same_bits(host(got[g]), want, f"{name} of the one-sample segment {g}, state {[float(v[g]) for v in edges['s']]}:", allow_nan=True)


def test_gram_of_sixty_four_single_sample_segments_of_edge_states(rig, edges):
    A = rig["ctx"][256].feature_gram(edges["sd"], edges["off"])
    assert A.shape == (64, NF, NF)
    one_sample_products(rig, edges, edges["phi"], edges["phi"], A, "A")
    same_bits(host(A[:, 0, :]), edges["phi"] + np.float32(0), "row 0 of every A_g against phi + 0:", allow_nan=True)


def test_cross_gram_of_sixty_four_single_sample_segments_of_edge_states(rig, edges):
    sd2 = [torch.roll(t, 7) for t in edges["sd"]]
    phi2 = np.roll(edges["phi"], 7, axis=0)
    Cm = rig["ctx"][256].feature_cross_gram(edges["sd"], sd2, edges["off"])
    assert Cm.shape == (64, NF, NF)
    one_sample_products(rig, edges, edges["phi"], phi2, Cm, "C")
    same_bits(host(Cm[:, 0, :]), phi2 + np.float32(0), "row 0 of every C_g against phi(s2) + 0:", allow_nan=True)
