"""SPEC §18 on the GPU: scg_basis_features, scg_basis_gram and scg_basis_values at the orders 3, 5 and 7, by bits or as exact integers.

- order 3 (256 features, 16 tiles: the small shape with every tiling edge — three macro-tiles a side, the last one short): whole A
  and b of small real-valued segments and of a three-slab segment against the plain fma32 chain, both block builds; features and
  values against tests/basis_model.py at the sample counts where the kernels' loops turn;
- order 5: basis_gram and basis_features are feature_gram and features by bits;
- order 7 (4096 features, 256 tiles, 43 macro-tiles a side, the last of 4 tiles): the embedding 3 in 5 in 7 by bits; a 48-index
  set outside the embedded block against the model; whole matrices on lattice prefixes with real tails and on 33 000 lattice
  samples; single-sample segments of edge states;
- the refusals, with sentinel-filled outputs."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import basis_model as BM
import gram_model as GM
from skill_chaining_with_graphs_amd.core import ScgContext
from bits import assert_bits_equal
from gpu_util import dev
from util import HP, make_oracle

pytestmark = pytest.mark.gpu

BUILDS = (256, 64)
F = {p: BM.num_features(p) for p in BM.ORDERS}


@pytest.fixture(scope="module", autouse=True)
def cached_blocks_go_back():
    """Five segments of order 7's A are a 336 MB block: torch's cached blocks are handed back when the module is done, so that later
    modules find the allocator as they would without this one (tests/test_gpu_gram_whole.py does the same)."""
    yield
    torch._C._cuda_clearCublasWorkspaces()               # (the float64 reference product of the 33 000-sample test left a BLAS workspace)
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
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        assert_bits_equal(got, want, allow_nan=allow_nan, msg=msg)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def real_yv(n, seed):
    yv = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    yv[:5] = np.array([0.0, -0.0, 1e-41, 1e30, -1e30], np.float32)[:n]
    return yv


# ---------------------------------------------------------------------------------------------------- order 3: whole matrices

# sample 0 in no segment; 3 samples; empty; 66 (the 64-sample chunk edge, a ragged tail of 2); 2053 (three slabs, the last ragged)
OFF_3 = [1, 4, 4, 70, 2123]


@pytest.fixture(scope="module")
def small3():
    n = OFF_3[-1] + 1
    s, yv = GM.gram_states(n, 31), real_yv(n, 32)
    phi = BM.features(3, *s)
    return dict(s=s, sd=[dev(v) for v in s], yv=yv, phi=phi, A=GM.chain(phi, phi, OFF_3), b=GM.lattice_rhs(phi, yv, OFF_3))


@pytest.mark.parametrize("build", BUILDS)
def test_order_three_gram_whole_matrix_by_bits(rig, small3, build):
    A, b = rig["ctx"][build].basis_gram(3, small3["sd"], OFF_3, dev(small3["yv"]))
    A, b = host(A), host(b)
    assert A.shape == (4, 256, 256) and b.shape == (4, 256)
    same_bits(A, small3["A"], f"A of order 3, every entry, {build}-env build:")
    same_bits(b, small3["b"], f"b of order 3, {build}-env build:")
    assert [float(v) for v in A[:, 0, 0]] == [3, 0, 66, 2053]
    assert np.array_equal(A.view(np.uint32), np.ascontiguousarray(A.transpose(0, 2, 1)).view(np.uint32))
    A2 = host(rig["ctx"][build].basis_gram(3, small3["sd"], OFF_3))              # without yv: the other instantiation
    same_bits(A2, small3["A"], f"A of order 3 without b, {build}-env build:")


N_SMALL = (1, 63, 64, 65, 8193)          # one sample; either side of a wavefront; past the features grid of 8192 workgroups


@pytest.fixture(scope="module")
def real3():
    s = GM.gram_states(max(N_SMALL), 33)
    rng = np.random.default_rng(34)
    V = rng.standard_normal((8, 256)).astype(np.float32)
    V[0, :5] = [0.0, -0.0, 1e-41, 1e30, -1e30]
    phi = BM.features(3, *s)
    return dict(s=s, phi=phi, V=V, want={m: BM.values(3, phi, V[:m]) for m in (1, 5, 8)})


@pytest.mark.parametrize("n", N_SMALL)
def test_order_three_features_equal_the_model_by_bits(rig, real3, n):
    got = host(rig["ctx"][256].basis_features(3, [dev(v[:n]) for v in real3["s"]]))
    assert got.shape == (n, 256)
    same_bits(got, real3["phi"][:n], f"basis_features, order 3, n = {n}:")


@pytest.mark.parametrize("m", (1, 5, 8))
@pytest.mark.parametrize("n", N_SMALL)
def test_order_three_values_equal_the_model_by_bits(rig, real3, n, m):
    got = host(rig["ctx"][256].basis_values(3, [dev(v[:n]) for v in real3["s"]], dev(real3["V"][:m])))
    assert got.shape == (m, n)
    same_bits(got, real3["want"][m][:, :n], f"basis_values, order 3, n = {n}, m = {m}:")


@pytest.mark.parametrize("order", (5, 7))
def test_values_of_the_other_orders_equal_the_model_by_bits(rig, order):
    """n = 67: eight groups of 8 samples and a group of 3; m = 5, the fit's shape."""
    s = GM.gram_states(67, 35 + order)
    V = np.random.default_rng(36).standard_normal((5, F[order])).astype(np.float32)
    got = host(rig["ctx"][256].basis_values(order, [dev(v) for v in s], dev(V)))
    same_bits(got, BM.values(order, BM.features(order, *s), V), f"basis_values, order {order}:")


def test_order_seven_features_equal_the_model_by_bits_and_index_in_64_bits(rig):
    s = GM.gram_states(65, 37)
    same_bits(host(rig["ctx"][256].basis_features(7, [dev(v) for v in s])), BM.features(7, *s), "basis_features, order 7:")
    # n F past 2^31: the last rows' element index needs 64 bits (8.6 GB of phi; only its ends are looked at)
    n = 2 ** 19 + 3
    big = GM.gram_states(n, 38)
    phi = rig["ctx"][256].basis_features(7, [dev(v) for v in big])
    tail = np.arange(n - 5, n)
    got = host(torch.cat([phi[:2], phi[n - 5:]]))
    del phi
    torch.cuda.empty_cache()
    at = np.concatenate([[0, 1], tail])
    same_bits(got, BM.features(7, *[v[at] for v in big]), "basis_features, order 7, rows either side of element 2^31:")


# ---------------------------------------------------------------------------------------------------- order 5: the existing kernels

MIXED_RUNS = [(1, False), (2048, True), (5, False), (60, True), (9, False), (28, True), (9, False), (2, True)]     # test_gpu_gram_whole.py's layout
MIXED_OFF = [1, 2054, 2054, 2123, 2123, 2160]


def test_order_five_is_feature_gram_and_features_by_bits(rig):
    s, lat = GM.mixed_states(MIXED_RUNS, 70)
    assert len(lat) == 2162
    sd, yv = [dev(v) for v in s], dev(real_yv(2162, 41))
    ctx = rig["ctx"][256]
    A, b = ctx.basis_gram(5, sd, MIXED_OFF, yv)
    A0, b0 = ctx.feature_gram(sd, MIXED_OFF, yv)
    assert A.shape == (5, 1296, 1296)
    same_bits(host(A), host(A0), "basis_gram(5) against feature_gram, A:")
    same_bits(host(b), host(b0), "basis_gram(5) against feature_gram, b:")
    same_bits(host(ctx.basis_gram(5, sd, MIXED_OFF)), host(A0), "basis_gram(5) without b:")
    same_bits(host(ctx.basis_features(5, sd)), host(ctx.features(sd)), "basis_features(5) against features:")
    same_bits(host(ctx.basis_features(5, sd)), rig["orc"].features(*s), "basis_features(5) against the oracle:")


# ---------------------------------------------------------------------------------------------------- order 7

def index_set_7(seed=7):
    """48 indices of order 7: 0, the tile edge 15 / 16, both sides of six 96-feature macro-tile edges, 4031 / 4032 (the short last
    macro-tile), 4095, and seeded features with some c in {6, 7} (outside the embedded order-5 block)."""
    must = {0, 15, 16, 4031, 4032, 4095}
    for e in (96, 192, 2016, 2112, 3840, 3936):
        must |= {e - 1, e}
    outside = np.nonzero((BM.coefficients(7) >= 6).any(axis=1))[0]
    rest = [int(i) for i in np.random.default_rng(seed).permutation(outside) if int(i) not in must]
    idx = np.array(sorted(must | set(rest[: 48 - len(must)])), np.int64)
    assert len(idx) == 48 and len(np.intersect1d(idx, BM.embed(5, 7))) <= 8
    return idx


@pytest.fixture(scope="module")
def real7(rig):
    """2162 real-valued samples in the mixed layout's offsets, at all three orders, from the 256-env build."""
    s = GM.gram_states(2162, 51)
    sd, yv = [dev(v) for v in s], real_yv(2162, 52)
    ctx = rig["ctx"][256]
    out = {p: tuple(host(t) for t in ctx.basis_gram(p, sd, MIXED_OFF, dev(yv))) for p in BM.ORDERS}
    return dict(s=s, sd=sd, yv=yv, out=out)


def test_order_seven_holds_order_five_and_order_five_holds_order_three_by_bits(real7):
    for q, p in ((5, 7), (3, 5), (3, 7)):
        e = BM.embed(q, p)
        (Ap, bp), (Aq, bq) = real7["out"][p], real7["out"][q]
        same_bits(Ap[:, e][:, :, e], Aq, f"A of order {p} at the embedded indices against order {q}:")
        same_bits(bp[:, e], bq, f"b of order {p} at the embedded indices against order {q}:")
    A7 = real7["out"][7][0]
    assert A7.shape == (5, 4096, 4096) and [float(v) for v in A7[:, 0, 0]] == [2053, 0, 69, 0, 37]
    for g in range(5):
        assert np.array_equal(A7[g].view(np.uint32), np.ascontiguousarray(A7[g].T).view(np.uint32)), g


def test_order_seven_outside_the_embedded_block_equals_the_model_by_bits(real7):
    idx = index_set_7()
    phi = BM.features(7, *real7["s"], idx=idx)
    loc = np.arange(len(idx))
    A7, b7 = real7["out"][7]
    same_bits(A7[:, idx][:, :, idx], GM.gram(phi, MIXED_OFF, loc, loc), "A of order 7 on the 48-index set:")
    same_bits(b7[:, idx], GM.rhs(phi, real7["yv"], MIXED_OFF), "b of order 7 on the 48-index set:")


# sample 0 in no segment; 1030 lattice + 2 real (two slabs: 1024 lattice, then 6 lattice and the 2 real); empty; 62 lattice + 3 real (the
# tail crosses the 64-sample chunk edge)
RUNS_7 = [(1, False), (1030, True), (2, False), (62, True), (3, False), (2, True)]
OFF_7 = [1, 1033, 1033, 1098]


WANT_7 = {}                  # the model's A and b of that layout, computed once for both builds (five whole-matrix fma32 steps)


@pytest.mark.parametrize("build", BUILDS)
def test_order_seven_lattice_prefix_and_real_tail_whole_matrix_by_bits(rig, build):
    want7 = WANT_7
    s, lat = GM.mixed_states(RUNS_7, 53)
    rng = np.random.default_rng(54)
    yv = np.where(lat, rng.integers(-3, 4, len(lat)), rng.standard_normal(len(lat))).astype(np.float32)
    if not want7:
        phi = BM.features(7, *s)
        want7["A"], want7["b"] = GM.lattice_gram(phi, OFF_7, lat), GM.lattice_rhs(phi, yv, OFF_7, lat)
    A, b = rig["ctx"][build].basis_gram(7, [dev(v) for v in s], OFF_7, dev(yv))
    A, b = host(A), host(b)
    same_bits(A, want7["A"], f"A of order 7, every entry, {build}-env build:")
    same_bits(b, want7["b"], f"b of order 7, {build}-env build:")
    assert [float(v) for v in A[:, 0, 0]] == [1032, 0, 65]


def test_order_seven_gram_of_33000_lattice_samples_is_the_integer_product(rig):
    """32 slabs + 232 samples in one segment. The features of a lattice state are exactly -1, 0 or 1, so phi = AB.re CD.re - AB.im CD.im
    and the Gram are exact in float64 in any order: the reference is formed from the model's tables by a float64 product."""
    n, lo = 33000 + 5, 3
    s = GM.lattice_states(n, 55)
    yv = np.random.default_rng(56).integers(-3, 4, n).astype(np.float32)
    (abr, abi), (cdr, cdi) = BM.tables(7, *s)
    assert all(np.isin(t, [-1.0, 0.0, 1.0]).all() for t in (abr, abi, cdr, cdi))
    t64 = lambda a: torch.from_numpy(a[:, lo:lo + 33000].astype(np.float64)).cuda()
    P = (t64(abr)[:, None, :] * t64(cdr)[None, :, :] - t64(abi)[:, None, :] * t64(cdi)[None, :, :]).reshape(4096, 33000)
    assert bool(((P == 0) | (P.abs() == 1)).all())
    wantA = (P @ P.T + 0.0).float()
    wantb = (P @ torch.from_numpy(yv[lo:lo + 33000].astype(np.float64)).cuda() + 0.0).float()
    del P
    A, b = rig["ctx"][256].basis_gram(7, [dev(v) for v in s], [lo, lo + 33000], dev(yv))
    torch.cuda.synchronize()
    assert torch.equal(A[0].view(torch.int32), wantA.view(torch.int32)), "A of 33 000 lattice samples, order 7"
    assert torch.equal(b[0].view(torch.int32), wantb.view(torch.int32)), "b of 33 000 lattice samples, order 7"
    assert float(A[0, 0, 0]) == 33000 and float(A[0].abs().max()) == 33000 and float(b.abs().max()) > 0


def test_order_seven_single_sample_segments_of_edge_states(rig):
    """Segment g holds sample g alone: every entry is fma(phi_i, phi_j, +0), the product rounded once (a -0 becomes +0), NaN where
    the product is NaN; phi is the device's own basis_features."""
    st = np.array([(1.0, 0.0, -2.0, 2.0), (-0.0, -0.0, -0.0, -0.0), (1e-41, -1e-41, 1e-41, -1e-41), (0.25, 2.0 ** 24 + 2, 0.5, -1.0),
                   (0.25, 0.75, np.nan, -1.0)], np.float32)
    sd = [dev(np.ascontiguousarray(st[:, d])) for d in range(4)]
    ctx = rig["ctx"][256]
    phi = host(ctx.basis_features(7, sd))
    assert np.all(phi[:, 0] == 1) and np.isnan(phi[4]).any() and not np.isnan(phi[:4]).any()
    A = host(ctx.basis_gram(7, sd, list(range(6))))
    assert A.shape == (5, 4096, 4096)
    for g in range(5):
        with np.errstate(invalid="ignore"):
            want = (phi[g].astype(np.float64)[:, None] * phi[g].astype(np.float64)[None, :]).astype(np.float32) + np.float32(0)
        same_bits(A[g], want, f"A of the one-sample segment {g}, state {st[g].tolist()}:", allow_nan=True)


# ---------------------------------------------------------------------------------------------------- refusals

FILL = -12345.5


def test_refusals_leave_the_outputs_untouched(rig):
    ctx = rig["ctx"][256]
    lib, raw = ctx.lib, ctx._ctx
    n = 70
    s = [dev(v) for v in GM.gram_states(n, 61)]
    yv, V = dev(real_yv(n, 62)), dev(np.ones((8, 256), np.float32))
    off = np.array([0, n], np.int64)
    A, b = torch.full((256 * 256,), FILL, device=s[0].device), torch.full((256,), FILL, device=s[0].device)
    phi, out = torch.full((n * 256,), FILL, device=s[0].device), torch.full((8 * n,), FILL, device=s[0].device)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    sp, offp, stream = [p(t) for t in s], off.ctypes.data_as(C.c_void_p), ctx._stream()

    def refused(rc, name, what):
        torch.cuda.synchronize()
        assert rc == -1, what
        assert name.encode() in lib.scg_last_error(raw), what
        for t in (A, b, phi, out):
            assert bool(torch.all(t == FILL)), what

    for order in (4, 9, 0, -1, 6, 2):
        refused(lib.scg_basis_features(raw, order, C.c_int64(n), *sp, p(phi), stream), "scg_basis_features", f"order {order}")
        refused(lib.scg_basis_gram(raw, order, C.c_int64(n), *sp, p(yv), 1, offp, p(A), p(b), stream), "scg_basis_gram", f"order {order}")
        refused(lib.scg_basis_values(raw, order, C.c_int64(n), *sp, p(V), 1, p(out), stream), "scg_basis_values", f"order {order}")
        assert b"order" in lib.scg_last_error(raw)
    refused(lib.scg_basis_gram(raw, 3, C.c_int64(n), *sp, p(yv), 1, offp, p(A), None, stream), "scg_basis_gram", "yv without b")
    refused(lib.scg_basis_gram(raw, 3, C.c_int64(n), *sp, None, 1, offp, p(A), p(b), stream), "scg_basis_gram", "b without yv")
    refused(lib.scg_basis_gram(raw, 3, C.c_int64(n), *sp, p(yv), 0, offp, p(A), p(b), stream), "scg_basis_gram", "n_seg = 0")
    refused(lib.scg_basis_gram(raw, 3, C.c_int64(-1), *sp, p(yv), 1, offp, p(A), p(b), stream), "scg_basis_gram", "n < 0")
    for m in (0, 9, -1):
        refused(lib.scg_basis_values(raw, 3, C.c_int64(n), *sp, p(V), m, p(out), stream), "scg_basis_values", f"m = {m}")
    refused(lib.scg_basis_values(raw, 3, C.c_int64(n), *sp, None, 1, p(out), stream), "scg_basis_values", "null V")
    refused(lib.scg_basis_features(raw, 3, C.c_int64(n), *sp, None, stream), "scg_basis_features", "null phi")
    # the order is looked at before the arrays: a bad order with a null array names the order
    assert lib.scg_basis_gram(raw, 4, C.c_int64(n), None, *sp[1:], p(yv), 1, offp, p(A), p(b), stream) == -1
    assert b"order" in lib.scg_last_error(raw)
    # and the accepted calls write what they should: the same buffers, order 3
    assert lib.scg_basis_gram(raw, 3, C.c_int64(n), *sp, p(yv), 1, offp, p(A), p(b), stream) == 0
    assert lib.scg_basis_values(raw, 3, C.c_int64(n), *sp, p(V), 8, p(out), stream) == 0
    torch.cuda.synchronize()
    assert float(A[0]) == n and not bool(torch.any(b == FILL)) and not bool(torch.any(out == FILL))
    with pytest.raises(Exception, match="order"):
        ctx.basis_gram(4, s, [0, n])
    with pytest.raises(Exception, match="1 <= m <= 8"):
        ctx.basis_values(3, s, dev(np.ones((9, 256), np.float32)))
