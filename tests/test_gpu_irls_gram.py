"""scg_basis_gram_irls (SPEC §23.2) against the host model of tests/irls_gram_model.py, bit for bit: at the orders 3, 5 and 7 on an
index set for every n, segmentation and block build, with rw and e the logistic terms of real logits (saturated ones among them, +-0
weights at chunk and slab edges); at order 3 over the whole 256 x 256 matrix on lattice states; the identities of §23.2 on the device
(order 5's H is scg_feature_gram_weighted's A, grad is scg_basis_gram's b whatever rw holds, H ignores e, unit weights, the embedded
sub-blocks, symmetry); segments made only of edge weights; the write set; the refusals in their sequence.

The shapes are tests/test_gpu_weighted_gram.py's. The one-segment models are computed once per order, in one pass over the 2049
samples (weighted_gram_model.prefix_chain)."""
import ctypes as C

import numpy as np
import pytest
import torch

import basis_model as BM
import gram_model as GM
import irls_gram_model as IM
import weighted_gram_model as WM
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd.core import ScgContext
from bits import assert_bits_equal
from gpu_util import dev
from util import HP, make_oracle

pytestmark = pytest.mark.gpu

N = 2049
NS = [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049]
SEGMENTATIONS = {                                                     # tests/test_gpu_gram.py's five
    "five segments, starts off the multiples of 4": [0, 5, 410, 411, 1437, 2049],
    "a segment across the array's slab edge": [1000, 1050],
    "slabs are cut per segment": [3, 1030, 2049],
    "an empty segment in the middle and one at the end": [0, 700, 700, 1300, 1300],
    "samples outside every segment": [7, 1000, 2001],
}
BUILDS = (256, 128, 64)
ORDERS = (3, 5, 7)
TINY = np.finfo(np.float32).tiny
FEATURES = {3: 256, 5: 1296, 7: 4096}


def index_set(order):
    """Feature indices of order `order`: both sides of the tile and macro-tile (96) edges at both ends, and seeded others."""
    F = FEATURES[order]
    if order == 5:
        return GM.index_set()
    must = {0, 15, 16, 17, 95, 96, 97, 191, 192, F - 17, F - 16, F - 1, 96 * ((F - 1) // 96) - 1, 96 * ((F - 1) // 96)}
    rest = [int(i) for i in np.random.default_rng(5 + order).permutation(F) if int(i) not in must]
    return np.array(sorted(must | set(rest[: 36 - len(must)])), np.int64)


def same_bits(got, want, msg, allow_nan=False):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        assert_bits_equal(got, want, allow_nan=allow_nan, msg=msg)


@pytest.fixture(scope="module")
def data():
    s = GM.gram_states(N, 21)
    orc, m = make_oracle("pinball_simple")
    rng = np.random.default_rng(47)
    z = rng.normal(0, 6, N).astype(np.float32)
    z[rng.choice(N, 80, replace=False)] = rng.choice(np.array([90, 100, -95, -200, 87, -87], np.float32), 80)      # saturated both ways
    z[[0, 2, 63, 64, 1023, 1024]] = [88, 120, 95, 1e9, 87.5, np.inf]                                              # p = 1, rw = +0 at the edges
    label = rng.integers(0, 2, N).astype(np.uint8)
    _, rw, e = IM.terms(orc, z, label)
    assert not rw[[0, 2, 63, 64, 1023, 1024]].any() and (rw == 0).sum() >= 30 and (rw > 0.4).sum() > 50
    rw[[2, 1024]] = -0.0                                              # ... and of both signs
    rw2 = rng.uniform(0.0, 0.5, N).astype(np.float32)                 # other weights and other residuals, for the independence checks
    e2 = rng.uniform(-1, 1, N).astype(np.float32)
    idx = {p: index_set(p) for p in ORDERS}
    phi = {p: (orc.features(*s)[:, idx[5]] if p == 5 else BM.features(p, *s, idx=idx[p])) for p in ORDERS}      # on the index sets
    ctx = {b: ScgContext(64, 0, m, device=0, block_envs=b, **HP) for b in BUILDS}
    model = {}
    for p in ORDERS:
        u = WM.operands(phi[p], rw)[0]
        model[p] = dict(H=WM.prefix_chain(u, u, set(NS)), g=WM.prefix_chain(phi[p], e[:, None], set(NS)))
    yield dict(s=s, rw=rw, e=e, idx=idx, phi=phi, ctx=ctx, orc=orc, model=model, sd=[dev(v) for v in s], rwd=dev(rw), ed=dev(e),
               rw2d=dev(rw2), e2d=dev(e2), one=dev(np.ones(N, np.float32)))
    for c in ctx.values():
        c.close()


def run(data, order, offsets, n=N, build=256, rw=None, e=None):
    s = [t[:n].contiguous() for t in data["sd"]]
    rwd = (data["rwd"] if rw is None else rw)[:n].contiguous()
    ed = (data["ed"] if e is None else e)[:n].contiguous()
    H, g = data["ctx"][build].basis_gram_irls(order, s, offsets, rwd, ed)
    torch.cuda.synchronize()
    F = FEATURES[order]
    assert H.shape == (len(offsets) - 1, F, F) and g.shape == (len(offsets) - 1, F)
    return H.cpu().numpy(), g.cpu().numpy()


def plain(data, order, offsets, n=N, yv=None):
    s = [t[:n].contiguous() for t in data["sd"]]
    A, b = data["ctx"][256].basis_gram(order, s, offsets, (data["ed"] if yv is None else yv)[:n].contiguous())
    torch.cuda.synchronize()
    return A.cpu().numpy(), b.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- 1. the model

def test_the_one_pass_model_is_the_models_chains(data):
    for p, n in ((3, 1025), (7, 5)):
        idx, phi = data["idx"][p], data["phi"][p]
        cols = np.arange(len(idx))
        same_bits(data["model"][p]["H"][n], IM.hessian(phi[:n], data["rw"][:n], [0, n], cols, cols)[0], f"H, order {p}, n {n}:")
        same_bits(data["model"][p]["g"][n][:, 0], IM.gradient(phi[:n], data["e"][:n], [0, n])[0], f"grad, order {p}, n {n}:")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n", NS)
def test_one_segment_equals_the_model_by_bits(data, order, n):
    idx = data["idx"][order]
    H, g = run(data, order, [0, n], n)
    same_bits(H[0][np.ix_(idx, idx)], data["model"][order]["H"][n], f"order {order} n {n}: H on the index set against the model:")
    same_bits(g[0][idx], data["model"][order]["g"][n][:, 0], f"order {order} n {n}: grad on the index set against the model:")
    same_bits(H[0], H[0].T, f"order {order} n {n}: H against its transpose:")
    # phi_0 = 1: H[0][0] is the sum of p (1 - p) and grad[0] the sum of e, within the chains' bound and the operands' rounding
    w = data["rw"][:n].astype(np.float64) ** 2
    assert H[0][0, 0] == pytest.approx(w.sum(), rel=2.0 ** -13, abs=1e-30)
    assert g[0][0] == pytest.approx(data["e"][:n].astype(np.float64).sum(), abs=2.0 ** -13 * np.abs(data["e"][:n]).sum() + 1e-30)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", list(SEGMENTATIONS))
def test_segmentations_equal_the_model_by_bits(data, order, name):
    off, idx, phi = SEGMENTATIONS[name], data["idx"][order], data["phi"][order]
    cols = np.arange(len(idx))
    H, g = run(data, order, off)
    same_bits(H[:, idx][:, :, idx], IM.hessian(phi, data["rw"], off, cols, cols), f"order {order}, {name}: H on the index set:")
    same_bits(g[:, idx], IM.gradient(phi, data["e"], off), f"order {order}, {name}: grad on the index set:")
    for k in range(len(off) - 1):
        same_bits(H[k], H[k].T, f"order {order}, {name}: H[{k}] against its transpose:")
        if off[k + 1] == off[k]:                                      # an empty segment: all +0
            assert not H[k].view(np.uint32).any() and not g[k].view(np.uint32).any()


@pytest.mark.parametrize("order", ORDERS)
def test_same_bits_from_every_block_build(data, order):
    off = SEGMENTATIONS["five segments, starts off the multiples of 4"]
    want = run(data, order, off, build=256)
    for b in (64, 128):
        assert data["ctx"][b].block_envs == b
        got = run(data, order, off, build=b)
        same_bits(got[0], want[0], f"order {order}: H, {b}-env build:")
        same_bits(got[1], want[1], f"order {order}: grad, {b}-env build:")


# ---------------------------------------------------------------------------------------------------- 2. the whole matrix, order 3

MIXED_RUNS = [(1, False), (1100, True), (5, False), (60, True), (9, False), (2, True)]      # tests/test_gpu_weighted_gram.py's
MIXED_OFF = [1, 1106, 1106, 1175]


@pytest.mark.parametrize("build", (256, 64))
def test_whole_matrix_at_order_3_on_lattice_states_by_bits(data, build):
    s, lat = GM.mixed_states(MIXED_RUNS, 70)
    n = len(lat)
    rng = np.random.default_rng(73)
    rw = rng.uniform(0.0, 0.5, n).astype(np.float32)
    rw[lat] = rng.integers(0, 3, int(lat.sum())).astype(np.float32)   # {0, 1, 2}: u stays an integer
    e = rng.uniform(-1, 1, n).astype(np.float32)
    e[lat] = rng.integers(-1, 2, int(lat.sum())).astype(np.float32)
    if "whole" not in data:                                           # (the model once for both builds)
        phi = BM.features(3, *s)
        assert np.all(np.isin(phi[lat], (-1.0, 0.0, 1.0)))            # the lattice holds at order 3 as at order 5
        u = WM.operands(phi, rw)[0]
        data["whole"] = GM.chain(u, u, MIXED_OFF, lat), GM.lattice_rhs(phi, e, MIXED_OFF, lat)
    wantH, wantg = data["whole"]
    H, g = data["ctx"][build].basis_gram_irls(3, [dev(v) for v in s], MIXED_OFF, dev(rw), dev(e))
    torch.cuda.synchronize()
    H, g = H.cpu().numpy(), g.cpu().numpy()
    same_bits(H, wantH, f"H, every entry, {build}-env build:")
    same_bits(g, wantg, f"grad, every entry, {build}-env build:")
    assert not H[1].view(np.uint32).any() and not g[1].view(np.uint32).any() and H[0][0, 0] > 1000


# ---------------------------------------------------------------------------------------------------- 3. the identities, on the device

@pytest.mark.parametrize("order", ORDERS)
def test_grad_ignores_rw_and_H_ignores_e(data, order):
    """A right-hand side formed from the weighted operand, or a weight on e, would show here."""
    for name, off in (("one segment", [0, N]), ("three", SEGMENTATIONS["slabs are cut per segment"])):
        H, g = run(data, order, off)
        _, b = plain(data, order, off)
        same_bits(g, b, f"order {order}, {name}: grad against scg_basis_gram's b for yv = e:")
        H2, g2 = run(data, order, off, rw=data["rw2d"])
        same_bits(g2, g, f"order {order}, {name}: grad under other weights:")
        assert not np.array_equal(H2, H)
        H3, g3 = run(data, order, off, e=data["e2d"])
        same_bits(H3, H, f"order {order}, {name}: H beside another e:")
        _, b3 = plain(data, order, off, yv=data["e2d"])
        same_bits(g3, b3, f"order {order}, {name}: grad for the other e against scg_basis_gram's b:")
        H0, g0 = run(data, order, off, rw=dev(np.zeros(N, np.float32)))                  # no weight at all: H = +0, grad as ever
        assert not H0.view(np.uint32).any()
        same_bits(g0, g, f"order {order}, {name}: grad under zero weights:")


@pytest.mark.parametrize("order", ORDERS)
def test_unit_weights_give_scg_basis_grams_bits(data, order):
    for n in (5, 1025, N):
        A, b = plain(data, order, [0, n], n)
        H, g = run(data, order, [0, n], n, rw=data["one"])
        same_bits(H, A, f"order {order}, n {n}: H under unit weights against scg_basis_gram's A:")
        same_bits(g, b, f"order {order}, n {n}: grad against scg_basis_gram's b:")


@pytest.mark.parametrize("name", list(SEGMENTATIONS))
def test_order_5_H_is_scg_feature_gram_weighteds_A(data, name):
    off = SEGMENTATIONS[name]
    H, _ = run(data, 5, off)
    A, _ = data["ctx"][256].feature_gram_weighted(data["sd"], off, data["rwd"])
    torch.cuda.synchronize()
    same_bits(H, A.cpu().numpy(), f"{name}: H against scg_feature_gram_weighted's A:")


def test_a_lower_order_is_the_embedded_sub_block(data):
    off = [3, 1030, 2049]
    out = {p: run(data, p, off) for p in ORDERS}
    for q, p in ((3, 5), (3, 7), (5, 7)):
        emb = BM.embed(q, p)
        same_bits(out[q][0], out[p][0][:, emb][:, :, emb], f"order {q}'s H in order {p}'s:")
        same_bits(out[q][1], out[p][1][:, emb], f"order {q}'s grad in order {p}'s:")


def test_a_zero_weight_masks_no_nan_and_a_bad_e_spoils_grad_only(data):
    off = [3, 1030, 2049]
    H, g = run(data, 3, off)
    bad_e = data["ed"].clone()
    bad_e[1500] = float("inf")
    Hb, gb = run(data, 3, off, e=bad_e)
    same_bits(Hb, H, "H beside an infinite e:")
    same_bits(gb[0], g[0], "grad of the other segment:")
    assert not np.isfinite(gb[1]).all()
    s = [t.clone() for t in data["sd"]]
    s[2][1023] = float("nan")                                         # sample 1023 has rw = +0: 0 * NaN is NaN
    assert data["rw"][1023] == 0
    Hn, gn = data["ctx"][256].basis_gram_irls(3, s, off, data["rwd"], data["ed"])
    torch.cuda.synchronize()
    assert np.isnan(Hn[0].cpu().numpy()).any()
    same_bits(Hn[1].cpu().numpy(), H[1], "H of the other segment:")


# ---------------------------------------------------------------------------------------------------- 4. edge weights

EDGE_RW = [0.0, -0.0, -1.0, 2.0 ** -140, 2.0 ** -70, 2.0 ** 60]


def test_segments_of_edge_weights_equal_the_model_by_bits(data):
    """Three segments made only of edge weights (tests/test_gpu_weighted_gram.py's): all six; all but 2^60; the tiny and zero ones
    alone, where H itself is a sum of subnormal products. Segment 1's e is subnormal: grad is a sum of subnormal products there."""
    n, off = 36, [0, 12, 27, 36]
    rw = np.array((EDGE_RW * 2) + (EDGE_RW[:5] * 3) + [2.0 ** -70, 2.0 ** -140, 0.0, -0.0, 2.0 ** -70, 2.0 ** -70, 2.0 ** -140, 2.0 ** -70,
                                                       2.0 ** -70], np.float32)
    assert len(rw) == n and rw[3] != 0 and abs(rw[3]) < TINY
    rng = np.random.default_rng(43)
    e = rng.uniform(-1, 1, n).astype(np.float32)
    e[12:27] = (e[12:27] * np.float32(1e-41)).astype(np.float32)
    assert np.all(np.abs(e[12:27]) < TINY) and np.any(e[12:27] != 0)
    s = [v[:n] for v in data["s"]]
    phi = BM.features(3, *s)
    u = WM.operands(phi, rw)[0]
    wantH, wantg = GM.chain(u, u, off), GM.chain(phi, e[:, None], off)[:, :, 0]
    # the case bites: with subnormal products flushed, stored bits differ
    flushed = np.where(np.abs(e) < TINY, np.float32(0), e)
    assert not np.array_equal(GM.chain(phi, flushed[:, None], off)[1].view(np.uint32), wantg[:, :, None][1].view(np.uint32))
    assert np.any((wantg[1] != 0) & (np.abs(wantg[1]) < TINY))
    assert np.any((wantH[2] != 0) & (np.abs(wantH[2]) < TINY)) and np.abs(wantH[2]).max() < 2.0 ** -130
    assert np.isfinite(wantH).all() and wantH[0].max() > 2.0 ** 119
    for build in (256, 64):
        H, g = data["ctx"][build].basis_gram_irls(3, [t[:n].contiguous() for t in data["sd"]], off, dev(rw), dev(e))
        torch.cuda.synchronize()
        same_bits(H.cpu().numpy(), wantH, f"H, every entry, {build}-env build:")
        same_bits(g.cpu().numpy(), wantg, f"grad, every entry, {build}-env build:")


# ---------------------------------------------------------------------------------------------------- 5. write set, refusals

GUARD = 4099                  # floats either side (odd: the outputs sit at a 4-byte-aligned address only)
FILL = -12345.5


def raw_call(ctx, order, n, s, rw, e, offsets, H, g, n_seg=None):
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64)
    p = lambda t: C.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    rc = ctx.lib.scg_basis_gram_irls(ctx._ctx, order, C.c_int64(n), *[p(t) for t in s], p(rw), p(e),
                                     len(off) - 1 if n_seg is None else n_seg,
                                     None if off is None else off.ctypes.data_as(C.c_void_p), p(H), p(g), ctx._stream())
    torch.cuda.synchronize()
    return rc


def guarded(n_seg, F):
    bufH = torch.full((2 * GUARD + n_seg * F * F,), FILL, dtype=torch.float32, device="cuda:0")
    bufg = torch.full((2 * GUARD + n_seg * F,), FILL, dtype=torch.float32, device="cuda:0")
    return bufH, bufg, bufH.data_ptr() + 4 * GUARD, bufg.data_ptr() + 4 * GUARD


@pytest.mark.parametrize("order", ORDERS)
def test_writes_H_and_grad_only_and_keeps_its_inputs(data, order):
    ctx, off, F = data["ctx"][256], [2, 900, 900, 2040], FEATURES[order]
    bufH, bufg, pH, pg = guarded(3, F)
    s = [t.clone() for t in data["sd"]]
    rwd, ed = data["rwd"].clone(), data["ed"].clone()
    assert raw_call(ctx, order, N, s, rwd, ed, off, pH, pg) == 0
    for buf, body in ((bufH, 3 * F * F), (bufg, 3 * F)):
        h = buf.cpu().numpy()
        assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + body:] == FILL)
        assert not np.any(h[GUARD: GUARD + body] == FILL)             # fully overwritten, the empty segment too
    H, g = run(data, order, off)
    same_bits(bufH.cpu().numpy()[GUARD: GUARD + 3 * F * F].reshape(3, F, F), H, "H at an odd address:")
    same_bits(bufg.cpu().numpy()[GUARD: GUARD + 3 * F].reshape(3, F), g, "grad at an odd address:")
    for t, w in zip(s + [rwd, ed], data["sd"] + [data["rwd"], data["ed"]]):
        assert torch.equal(t.view(torch.int32), w.view(torch.int32))


def test_refusals_in_their_sequence_write_nothing_and_n_zero_zeroes(data):
    ctx, F = data["ctx"][256], 256
    bufH, bufg, pH, pg = guarded(1, F)
    s, rwd, ed = data["sd"], data["rwd"], data["ed"]
    base = dict(order=3, n=N, s=s, rw=rwd, e=ed, offsets=[0, N], H=pH, g=pg)
    bad_order, null_rw, neg_n, seg0 = dict(order=4), dict(rw=None), dict(n=-1), dict(offsets=[0])
    leave, decr = dict(offsets=[0, N + 1]), dict(offsets=[0, 9, 5])
    # every refusal alone, and beside the NEXT one of the sequence: the earlier one's message is the one reported
    cases = [
        ("order must be", bad_order), ("order must be", dict(order=0)), ("order must be", dict(order=6)), ("order must be", dict(bad_order, **null_rw)),
        ("null array", null_rw), ("null array", dict(e=None)), ("null array", dict(s=[None] + s[1:])), ("null array", dict(s=s[:3] + [None])),
        ("null array", dict(H=None)), ("null array", dict(g=None)), ("null array", dict(offsets=None, n_seg=1)), ("null array", dict(null_rw, **neg_n)),
        ("n must be", neg_n), ("n must be", dict(neg_n, **seg0)),
        ("n_seg", seg0), ("n_seg", dict(offsets=list(range(66)))), ("n_seg", dict(offsets=[5] * 65 + [N + 1])),
        ("leave", leave), ("leave", dict(offsets=[-1, N])), ("leave", dict(offsets=[0, 9, 5, N + 1])),
        ("decrease", decr),
    ]
    for want, kw in cases:
        a = dict(base, **kw)
        name = f"{want}: {sorted(kw)}"
        assert raw_call(ctx, a["order"], a["n"], a["s"], a["rw"], a["e"], a["offsets"], a["H"], a["g"], a.get("n_seg")) == -1, name
        err = ctx.lib.scg_last_error(ctx._ctx)
        assert b"scg_basis_gram_irls" in err and want.encode() in err, (name, err)
        assert torch.all(bufH == FILL) and torch.all(bufg == FILL), name
    assert ctx.lib.scg_basis_gram_irls(None, 4, C.c_int64(0), *([None] * 6), 1, None, None, None, None) == -1
    assert b"null ctx" in ctx.lib.scg_last_error(None)
    for n, off in ((0, [0, 0]), (N, [7, 7])):                         # n = 0, and every segment empty: zeroed, nothing else
        bufH.fill_(FILL), bufg.fill_(FILL)
        assert raw_call(ctx, 3, n, s, rwd, ed, off, pH, pg) == 0
        hH, hg = bufH.cpu().numpy(), bufg.cpu().numpy()
        assert not hH[GUARD: GUARD + F * F].view(np.uint32).any() and not hg[GUARD: GUARD + F].view(np.uint32).any()
        assert np.all(hH[:GUARD] == FILL) and np.all(hH[GUARD + F * F:] == FILL)
        assert np.all(hg[:GUARD] == FILL) and np.all(hg[GUARD + F:] == FILL)
    H, g = ctx.basis_gram_irls(5, [t[:0] for t in s], [0, 0, 0], rwd[:0], ed[:0])      # ... and through the wrapper, from empty tensors
    assert H.shape == (2, 1296, 1296) and g.shape == (2, 1296)
    assert not H.cpu().numpy().view(np.uint32).any() and not g.cpu().numpy().view(np.uint32).any()
    for bad in (rwd[:5].contiguous(), rwd.cpu(), rwd.double(), rwd[::2], None):
        with pytest.raises(scg.ScgError):
            ctx.basis_gram_irls(3, s, [0, N], bad, ed)
        with pytest.raises(scg.ScgError):
            ctx.basis_gram_irls(3, s, [0, N], rwd, bad)
    with pytest.raises(scg.ScgError):
        ctx.basis_gram_irls(4, s, [0, N], rwd, ed)
    with pytest.raises(scg.ScgError):
        ctx.basis_gram_irls(3, s, [0, N + 1], rwd, ed)
