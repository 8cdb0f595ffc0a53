"""scg_feature_gram_weighted (SPEC §22.1) against the host model of tests/weighted_gram_model.py, bit for bit: on an index set for
every n, target count, segmentation and block build; over the whole matrix on lattice states with lattice weights; the three
identities the definition implies (unit weights against both unweighted entry points, a uniform 2, a zero-weight tail across a slab
edge); segments made only of edge weights, where a flushed subnormal product would change a stored bit; a target's independence of
its neighbours; the write set; the refusals in their sequence.

The shapes are tests/test_gpu_gram_targets.py's. The one-segment models of all 16 targets and of A on the index set are computed
once, in one pass over the 2049 samples (weighted_gram_model.prefix_chain, tied to gram_model.gram / rhs below)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gram_model as GM
import weighted_gram_model as WM
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd.core import ScgContext
from bits import assert_bits_equal
from gpu_util import dev
from util import HP, make_oracle

pytestmark = pytest.mark.gpu

NF = 1296
N = 2049
T = _lib.GRAM_MAX_TARGETS
NS = [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049]
SEGMENTATIONS = {                                                     # tests/test_gpu_gram.py's five
    "five segments, starts off the multiples of 4": [0, 5, 410, 411, 1437, 2049],
    "a segment across the array's slab edge": [1000, 1050],
    "slabs are cut per segment": [3, 1030, 2049],
    "an empty segment in the middle and one at the end": [0, 700, 700, 1300, 1300],
    "samples outside every segment": [7, 1000, 2001],
}
BUILDS = (256, 128, 64)
TINY = np.finfo(np.float32).tiny


def same_bits(got, want, msg, allow_nan=False):
    """assert_bits_equal, with the common case (no difference) decided by one comparison of the words."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        assert_bits_equal(got, want, allow_nan=allow_nan, msg=msg)


@pytest.fixture(scope="module")
def data():
    s = GM.gram_states(N, 21)
    orc, m = make_oracle("pinball_simple")
    phi = orc.features(*s)
    rng = np.random.default_rng(41)
    rw = rng.uniform(0.25, 4.0, N).astype(np.float32)
    rw[rng.choice(N, 60, replace=False)] = 0.0                        # exact zeros ...
    rw[[0, 2, 1023, 1024]] = [0.0, -0.0, 0.0, -0.0]                   # ... at the edges of chunks and slabs too
    rw[rng.choice(N, 500, replace=False)] *= -1.0                     # negative roots: the same weight
    Y = rng.standard_normal((T, N)).astype(np.float32)
    idx = GM.index_set()
    ctx = {b: ScgContext(64, 0, m, device=0, block_envs=b, **HP) for b in BUILDS}
    model = dict(A=WM.prefix_gram(phi, rw, set(NS), idx, idx), B=WM.prefix_rhs(phi, rw, Y, set(NS)))
    yield dict(s=s, phi=phi, rw=rw, Y=Y, idx=idx, ctx=ctx, orc=orc, sd=[dev(v) for v in s], rwd=dev(rw), Yd=dev(Y), model=model,
               one=dev(np.ones(N, np.float32)))
    for c in ctx.values():
        c.close()


def run(data, offsets, n=N, n_tgt=5, build=256, rw=None, Y=None):
    s = [t[:n].contiguous() for t in data["sd"]]
    rwd = (data["rwd"] if rw is None else rw)[:n].contiguous()
    Yd = None if n_tgt == 0 else (data["Yd"] if Y is None else Y)[:n_tgt, :n].contiguous()
    A, B = data["ctx"][build].feature_gram_weighted(s, offsets, rwd, Yd)
    torch.cuda.synchronize()
    assert A.shape == (len(offsets) - 1, NF, NF)
    assert B is None if n_tgt == 0 else B.shape == (len(offsets) - 1, n_tgt, NF)
    return A.cpu().numpy(), None if B is None else B.cpu().numpy()


def unweighted(data, offsets, n=N, n_tgt=5):
    s = [t[:n].contiguous() for t in data["sd"]]
    A, B = data["ctx"][256].feature_gram_targets(s, offsets, data["Yd"][:n_tgt, :n].contiguous())
    torch.cuda.synchronize()
    return A.cpu().numpy(), B.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- 1. the model

def test_the_one_pass_model_is_gram_models_chains(data):
    phi, rw, Y, idx = data["phi"], data["rw"], data["Y"], data["idx"]
    for n, c in ((1025, 3), (5, 0)):
        same_bits(data["model"]["B"][n][c], WM.rhs(phi[:n], rw[:n], Y[c:c + 1, :n], [0, n])[0, 0], f"B, n {n} column {c}:")
        same_bits(data["model"]["A"][n], WM.gram(phi[:n], rw[:n], [0, n], idx, idx)[0], f"A, n {n}:")


@pytest.mark.parametrize("n", NS)
def test_one_segment_equals_the_model_by_bits_for_every_target_count(data, n):
    idx = data["idx"]
    A0 = None
    for n_tgt in (0, 1, 5, 16):
        A, B = run(data, [0, n], n, n_tgt)
        same_bits(A[0][np.ix_(idx, idx)], data["model"]["A"][n], f"n {n} n_tgt {n_tgt}: A on the index set against the model:")
        same_bits(A[0], A[0].T, f"n {n} n_tgt {n_tgt}: A against its transpose:")
        A0 = A if A0 is None else A0
        same_bits(A, A0, f"n {n}: A with {n_tgt} targets against A alone:")
        if n_tgt:
            same_bits(B[0], data["model"]["B"][n][:n_tgt], f"n {n} n_tgt {n_tgt}: B against the model:")
    w = data["rw"][:n].astype(np.float64) ** 2
    # phi_0 = 1: A[0][0] is the sum of the weights, within the chain's bound (1024 + 3) 2^-24 and the operands' rounding 2^-22 < 2^-13
    assert A0[0][0, 0] == pytest.approx(w.sum(), rel=2.0 ** -13, abs=1e-30)


@pytest.mark.parametrize("name", list(SEGMENTATIONS))
def test_segmentations_equal_the_model_by_bits(data, name):
    off, idx = SEGMENTATIONS[name], data["idx"]
    A, B = run(data, off)
    same_bits(A[:, idx][:, :, idx], WM.gram(data["phi"], data["rw"], off, idx, idx), f"{name}: A on the index set against the model:")
    same_bits(B, WM.rhs(data["phi"], data["rw"], data["Y"][:5], off), f"{name}: B against the model:")
    A0, _ = run(data, off, n_tgt=0)
    same_bits(A0, A, f"{name}: A alone against A with targets:")
    for g in range(len(off) - 1):
        same_bits(A[g], A[g].T, f"{name}: A[{g}] against its transpose:")
        if off[g + 1] == off[g]:                                      # an empty segment: all +0
            assert not A[g].view(np.uint32).any() and not B[g].view(np.uint32).any()


def test_same_bits_from_every_block_build(data):
    off = SEGMENTATIONS["five segments, starts off the multiples of 4"]
    for n_tgt in (0, 5):
        want = run(data, off, n_tgt=n_tgt, build=256)
        for b in (64, 128):
            assert data["ctx"][b].block_envs == b
            got = run(data, off, n_tgt=n_tgt, build=b)
            same_bits(got[0], want[0], f"A, {b}-env build, {n_tgt} targets:")
            if n_tgt:
                same_bits(got[1], want[1], f"B, {b}-env build:")


# ---------------------------------------------------------------------------------------------------- 2. the whole matrix

# sample 0 belongs to no segment; 1100 lattice samples (a slab and 76) with 5 real ones behind; an empty segment; 60 lattice + 9 real
# (the tail crosses the kernel's chunk edge at 64)
MIXED_RUNS = [(1, False), (1100, True), (5, False), (60, True), (9, False), (2, True)]
MIXED_OFF = [1, 1106, 1106, 1175]


@pytest.mark.parametrize("build", (256, 64))
def test_whole_matrix_on_lattice_states_with_lattice_weights_by_bits(data, build):
    s, lat = GM.mixed_states(MIXED_RUNS, 70)
    n = len(lat)
    rng = np.random.default_rng(73)
    rw = rng.uniform(-4.0, 4.0, n).astype(np.float32)
    rw[lat] = rng.integers(0, 3, int(lat.sum())).astype(np.float32)   # {0, 1, 2}: u stays an integer
    Y = rng.standard_normal((3, n)).astype(np.float32)
    Y[:, lat] = rng.integers(-3, 4, (3, int(lat.sum()))).astype(np.float32)
    phi = data["orc"].features(*s)
    if "whole" not in data:                                           # (the model once for both builds)
        data["whole"] = WM.whole(phi, rw, Y, MIXED_OFF, lat)
    wantA, wantB = data["whole"]
    A, B = data["ctx"][build].feature_gram_weighted([dev(v) for v in s], MIXED_OFF, dev(rw), dev(Y))
    torch.cuda.synchronize()
    A, B = A.cpu().numpy(), B.cpu().numpy()
    same_bits(A, wantA, f"A, every entry, {build}-env build:")
    same_bits(B, wantB, f"B, every entry, {build}-env build:")
    for g in range(3):
        same_bits(A[g], A[g].T, f"A[{g}] against its transpose:")
    assert not A[1].view(np.uint32).any() and not B[1].view(np.uint32).any() and A[0][0, 0] > 1000


# ---------------------------------------------------------------------------------------------------- 3. the identities

@pytest.mark.parametrize("n", NS)
def test_unit_weights_give_the_unweighted_entry_points_bits(data, n):
    wantA, wantB = unweighted(data, [0, n], n)
    A, B = run(data, [0, n], n, 5, rw=data["one"])
    same_bits(A, wantA, f"n {n}: A against scg_feature_gram_targets':")
    same_bits(B, wantB, f"n {n}: B against scg_feature_gram_targets':")
    A0, _ = run(data, [0, n], n, 0, rw=data["one"])
    plain = data["ctx"][256].feature_gram([t[:n].contiguous() for t in data["sd"]], [0, n])
    torch.cuda.synchronize()
    same_bits(A0, plain.cpu().numpy(), f"n {n}: A alone against scg_feature_gram's:")


@pytest.mark.parametrize("name", list(SEGMENTATIONS))
def test_unit_weights_give_the_unweighted_bits_on_every_segmentation(data, name):
    off = SEGMENTATIONS[name]
    wantA, wantB = unweighted(data, off, n_tgt=16)
    A, B = run(data, off, n_tgt=16, rw=data["one"])
    same_bits(A, wantA, f"{name}: A:")
    same_bits(B, wantB, f"{name}: B:")


def test_uniform_two_gives_four_times_the_unweighted_bits(data):
    off, idx = SEGMENTATIONS["slabs are cut per segment"], data["idx"]
    # on the CPU first: no operand and no partial sum of the compared entries is subnormal, so scaling by 4 commutes with every rounding
    assert WM.no_subnormal_partial_sum(data["phi"], np.ones(N, np.float32), data["Y"][:5], off, idx, idx)
    wantA, wantB = unweighted(data, off)
    A, B = run(data, off, rw=dev(np.full(N, 2.0, np.float32)))
    same_bits(A[:, idx][:, :, idx], np.float32(4) * wantA[:, idx][:, :, idx], "A on the index set against 4 A:")
    same_bits(B, np.float32(4) * wantB, "B against 4 B:")
    Am, Bm = run(data, off, rw=dev(np.full(N, -2.0, np.float32)))     # the sign of the root does not matter here: (-2 a)(-2 b) = 4 a b
    same_bits(Am[:, idx][:, :, idx], A[:, idx][:, :, idx], "A under -2 against A under 2:")
    same_bits(Bm, B, "B under -2 against B under 2:")


@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_a_zero_weight_tail_gives_the_shortened_segments_bits(data, zero):
    """Segment 0 = samples 3 .. 1029 has its slab edge at sample 1027: the zero tail 1020 .. 1029 lies across it."""
    rw = np.ones(N, np.float32)
    rw[1020:1030] = zero
    rw[2040:] = zero
    A, B = run(data, [3, 1030, 2049], rw=dev(rw))
    for g, short in enumerate(([3, 1020], [1030, 2040])):
        wantA, wantB = unweighted(data, short)
        same_bits(A[g], wantA[0], f"A[{g}] against the segment {short}:")
        same_bits(B[g], wantB[0], f"B[{g}] against the segment {short}:")
    assert A[0][0, 0] == 1017 and A[1][0, 0] == 1010


# ---------------------------------------------------------------------------------------------------- 4. edge weights

EDGE_RW = [0.0, -0.0, -1.0, 2.0 ** -140, 2.0 ** -70, 2.0 ** 60]


def test_segments_of_edge_weights_equal_the_model_by_bits(data):
    """Three segments made only of the edge weights: all six; all but 2^60, where the subnormal t = -1 * Y of target 1 decides B's
    stored bits; and the tiny and zero ones alone, where A itself is a sum of subnormal products."""
    n, off = 36, [0, 12, 27, 36]
    rw = np.array((EDGE_RW * 2) + (EDGE_RW[:5] * 3) + [2.0 ** -70, 2.0 ** -140, 0.0, -0.0, 2.0 ** -70, 2.0 ** -70, 2.0 ** -140, 2.0 ** -70,
                                                       2.0 ** -70], np.float32)
    assert len(rw) == n and rw[3] != 0 and abs(rw[3]) < TINY
    rng = np.random.default_rng(43)
    Y = rng.standard_normal((3, n)).astype(np.float32)
    Y[1] = (Y[1] * np.float32(1e-41)).astype(np.float32)              # subnormal targets
    Y[2] = Y[2] * np.float32(1e-30)
    assert np.all(np.abs(Y[1]) < TINY) and np.any(Y[1] != 0)
    phi = data["phi"][:n]
    wantA, wantB = WM.whole(phi, rw, Y, off)
    # the case bites: with the products t flushed, stored bits of B differ; and segment 2's A is made of subnormal sums
    u, t = WM.operands(phi, rw, Y)
    flushed = np.where(np.abs(t) < TINY, np.float32(0), t)
    assert not np.array_equal(GM.chain(u, flushed, off)[1].view(np.uint32), GM.chain(u, t, off)[1].view(np.uint32))
    assert np.any((wantB[1, 1] != 0) & (np.abs(wantB[1, 1]) < TINY))
    assert np.any((wantA[2] != 0) & (np.abs(wantA[2]) < TINY)) and np.abs(wantA[2]).max() < 2.0 ** -130
    assert np.isfinite(wantA).all() and np.isfinite(wantB).all() and wantA[0].max() > 2.0 ** 119
    for build in (256, 64):
        A, B = data["ctx"][build].feature_gram_weighted([t_[:n].contiguous() for t_ in data["sd"]], off, dev(rw), dev(Y))
        torch.cuda.synchronize()
        same_bits(A.cpu().numpy(), wantA, f"A, every entry, {build}-env build:")
        same_bits(B.cpu().numpy(), wantB, f"B, every entry, {build}-env build:")


# ---------------------------------------------------------------------------------------------------- 5. independence, write set

def test_a_target_does_not_depend_on_its_neighbours(data):
    off = [3, 1030, 2049]
    A16, B16 = run(data, off, n_tgt=16)
    for c in (0, 7, 15):                                              # target c alone: n_tgt = 1 with Y[c] as the one row
        A1, B1 = run(data, off, n_tgt=1, Y=data["Yd"][c:c + 1])
        same_bits(B1[:, 0], B16[:, c], f"target {c} alone against the same among 16:")
        same_bits(A1, A16, f"A beside target {c} alone against A beside 16:")
    A5, B5 = run(data, off)
    same_bits(B5, B16[:, :5], "targets 0 .. 4 against the same among 16:")
    bad = data["Yd"].clone()
    bad[1] = float("nan")
    bad[3, [0, 1500]] = float("inf")
    Ab, Bb = run(data, off, Y=bad)
    same_bits(Ab, A5, "A beside a NaN and an inf target:")
    for c in (0, 2, 4):
        same_bits(Bb[:, c], B5[:, c], f"target {c} beside a NaN and an inf target:")
    assert np.isnan(Bb[:, 1]).all()
    # a zero weight masks nothing: sample 1023 has rw = +0 and lies in segment 0, and 0 * inf is NaN
    bad2 = data["Yd"].clone()
    bad2[2, 1023] = float("inf")
    assert data["rw"][1023] == 0
    _, Bz = run(data, off, Y=bad2)
    assert np.isnan(Bz[0, 2]).all() and not np.isnan(Bz[1, 2]).any()
    for c in (0, 1, 3, 4):
        same_bits(Bz[:, c], B5[:, c], f"target {c} beside a target with an inf under a zero weight:")


GUARD = 4099                  # floats either side (odd: the outputs sit at a 4-byte-aligned address only)
FILL = -12345.5


def raw_call(ctx, n, s, rw, Y, n_tgt, offsets, A, B, n_seg=None):
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64)
    p = lambda t: C.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    rc = ctx.lib.scg_feature_gram_weighted(ctx._ctx, C.c_int64(n), *[p(t) for t in s], p(rw), p(Y), n_tgt,
                                           len(off) - 1 if n_seg is None else n_seg,
                                           None if off is None else off.ctypes.data_as(C.c_void_p), p(A), p(B), ctx._stream())
    torch.cuda.synchronize()
    return rc


def guarded(n_seg, room):
    """A and a B buffer with room for `room` targets a segment, both between guard bands, all on the sentinel."""
    bufA = torch.full((2 * GUARD + n_seg * NF * NF,), FILL, dtype=torch.float32, device="cuda:0")
    bufB = torch.full((2 * GUARD + n_seg * room * NF,), FILL, dtype=torch.float32, device="cuda:0")
    return bufA, bufB, bufA.data_ptr() + 4 * GUARD, bufB.data_ptr() + 4 * GUARD


@pytest.mark.parametrize("n_tgt", [0, 1, 5])
def test_writes_A_and_n_tgt_rows_of_B_only_and_keeps_its_inputs(data, n_tgt):
    ctx, off = data["ctx"][256], [2, 900, 900, 2040]
    bufA, bufB, pA, pB = guarded(3, T)
    s = [t.clone() for t in data["sd"]]
    rwd = data["rwd"].clone()
    Yd = data["Yd"][:max(n_tgt, 1)].clone()
    assert raw_call(ctx, N, s, rwd, Yd if n_tgt else None, n_tgt, off, pA, pB if n_tgt else None) == 0
    for buf, body in ((bufA, 3 * NF * NF), (bufB, 3 * n_tgt * NF)):
        h = buf.cpu().numpy()
        assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + body:] == FILL)
        assert not np.any(h[GUARD: GUARD + body] == FILL)             # fully overwritten, the empty segment too
    A, B = run(data, off, n_tgt=n_tgt)
    same_bits(bufA.cpu().numpy()[GUARD: GUARD + 3 * NF * NF].reshape(3, NF, NF), A, "A at an odd address:")
    if n_tgt:
        same_bits(bufB.cpu().numpy()[GUARD: GUARD + 3 * n_tgt * NF].reshape(3, n_tgt, NF), B, "B at an odd address:")
    for t, w in zip(s + [rwd, Yd], data["sd"] + [data["rwd"], data["Yd"][:max(n_tgt, 1)]]):
        assert torch.equal(t.view(torch.int32), w.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 6. refusals

def test_refusals_in_their_sequence_write_nothing_and_n_zero_zeroes(data):
    ctx = data["ctx"][256]
    bufA, bufB, pA, pB = guarded(1, T)
    s, rwd, Yd = data["sd"], data["rwd"], data["Yd"][:5].contiguous()
    base = dict(n=N, s=s, rw=rwd, Y=Yd, n_tgt=5, offsets=[0, N], A=pA, B=pB)
    # every refusal alone, and beside the NEXT one of the sequence: the earlier one's message is the one reported
    null_rw, neg_n, seg0 = dict(rw=None), dict(n=-1), dict(offsets=[0])
    leave, decr = dict(offsets=[0, N + 1]), dict(offsets=[0, 9, 5])
    cases = [
        ("null array", null_rw), ("null array", dict(s=[None] + s[1:])), ("null array", dict(A=None)),
        ("null array", dict(offsets=None, n_seg=1)), ("null array", dict(null_rw, **neg_n)),
        ("n must be", dict(neg_n, offsets=[0, 0])), ("n must be", dict(neg_n, **seg0)),
        ("n_seg", seg0), ("n_seg", dict(offsets=list(range(66)))), ("n_seg", dict(offsets=[5] * 65 + [N + 1])),
        ("leave", leave), ("leave", dict(offsets=[-1, N])), ("leave", dict(offsets=[0, 9, 5, N + 1])),
        ("decrease", decr), ("decrease", dict(decr, n_tgt=17)),
        ("n_tgt out of range", dict(n_tgt=17)), ("n_tgt out of range", dict(n_tgt=-1)), ("n_tgt out of range", dict(n_tgt=17, Y=None, B=None)),
        ("n_tgt = 0", dict(n_tgt=0)), ("n_tgt = 0", dict(n_tgt=0, Y=None)), ("n_tgt = 0", dict(n_tgt=0, B=None)),
        ("n_tgt >= 1", dict(Y=None)), ("n_tgt >= 1", dict(B=None)), ("n_tgt >= 1", dict(n_tgt=1, Y=None, B=None)),
    ]
    for want, kw in cases:
        a = dict(base, **kw)
        name = f"{want}: {sorted(kw)}"
        assert raw_call(ctx, a["n"], a["s"], a["rw"], a["Y"], a["n_tgt"], a["offsets"], a["A"], a["B"], a.get("n_seg")) == -1, name
        err = ctx.lib.scg_last_error(ctx._ctx)
        assert b"scg_feature_gram_weighted" in err and want.encode() in err, (name, err)
        assert torch.all(bufA == FILL) and torch.all(bufB == FILL), name
    assert ctx.lib.scg_feature_gram_weighted(None, 0, *([None] * 6), 0, 1, None, None, None, None) == -1
    assert b"null ctx" in ctx.lib.scg_last_error(None)
    for n, off in ((0, [0, 0]), (N, [7, 7])):                         # n = 0, and every segment empty: zeroed, nothing else
        bufA.fill_(FILL), bufB.fill_(FILL)
        assert raw_call(ctx, n, s, rwd, Yd, 5, off, pA, pB) == 0
        hA, hB = bufA.cpu().numpy(), bufB.cpu().numpy()
        assert not hA[GUARD: GUARD + NF * NF].view(np.uint32).any() and not hB[GUARD: GUARD + 5 * NF].view(np.uint32).any()
        assert np.all(hA[:GUARD] == FILL) and np.all(hA[GUARD + NF * NF:] == FILL)
        assert np.all(hB[:GUARD] == FILL) and np.all(hB[GUARD + 5 * NF:] == FILL)
    A, B = ctx.feature_gram_weighted([t[:0] for t in s], [0, 0, 0], rwd[:0], Yd[:, :0])      # ... and through the wrapper, from empty tensors
    assert A.shape == (2, NF, NF) and B.shape == (2, 5, NF)
    assert not A.cpu().numpy().view(np.uint32).any() and not B.cpu().numpy().view(np.uint32).any()
    A, B = ctx.feature_gram_weighted([t[:0] for t in s], [0, 0], rwd[:0])
    assert B is None and not A.cpu().numpy().view(np.uint32).any()
    for bad in (Yd[:, :5].contiguous(), Yd[0], torch.zeros((17, N), dtype=torch.float32, device="cuda:0"), Yd.cpu(), Yd.double()):
        with pytest.raises(scg.ScgError):
            ctx.feature_gram_weighted(s, [0, N], rwd, bad)
    for bad in (rwd[:5].contiguous(), rwd.cpu(), rwd.double(), rwd[::2], None):
        with pytest.raises(scg.ScgError):
            ctx.feature_gram_weighted(s, [0, N], bad, Yd)
    with pytest.raises(scg.ScgError):
        ctx.feature_gram_weighted(s, [0, N + 1], rwd, Yd)
