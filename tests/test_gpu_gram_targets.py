"""scg_feature_gram_targets (SPEC §20.1): A and every B[g][c] equal scg_feature_gram's A and its b for yv = Y[c], and the host
model of tests/gram_model.py, bit for bit, for every n_tgt, segmentation and block build; a target does not depend on its
neighbours; the write set is A and n_seg * n_tgt * 1296 floats of B; the refusals.

The model of all 16 targets is computed once, in one pass over the 2049 samples (`prefix_rhs`: §16.1's two levels with the 16
targets side by side, read off at every n the tests use): a one-segment B at n samples is a prefix of that pass. It is tied to
gram_model.rhs, the model the single-yv tests use, on one column."""
import ctypes as C

import numpy as np
import pytest
import torch

import gram_model as GM
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
EDGE_AT = [0, 2, 4, 1023, 1024, 2048]
EDGE_VALUES = np.array([0.0, -0.0, 1e-41, 1e30, -1e30, 1e-41], np.float32)


def rhs_multi(phi, Y, offsets):
    """gram_model.rhs for the targets Y [C][n] side by side: float32 [n_seg][C][1296]."""
    phi, Y = np.asarray(phi, np.float32), np.asarray(Y, np.float32)
    out = np.zeros((len(offsets) - 1, Y.shape[0], phi.shape[1]), np.float32)
    for g in range(len(offsets) - 1):
        for lo, hi in GM.slabs(int(offsets[g]), int(offsets[g + 1])):
            P = np.zeros(out.shape[1:], np.float32)
            for n in range(lo, hi):
                P = GM.fma32(phi[n][None, :], Y[:, n][:, None], P)
            out[g] = out[g] + P
    return out


def prefix_rhs(phi, Y, ns):
    """{n: rhs_multi(phi[:n], Y[:, :n], [0, n])[0]} for every n of `ns` from one pass over the samples."""
    out, tot, P = {}, np.zeros((Y.shape[0], phi.shape[1]), np.float32), None
    for n in range(max(ns)):
        if n % GM.SLAB == 0:
            P = np.zeros_like(tot)
        P = GM.fma32(phi[n][None, :], Y[:, n][:, None], P)
        if (n + 1) % GM.SLAB == 0:
            tot = tot + P
        if n + 1 in ns:
            out[n + 1] = tot.copy() if (n + 1) % GM.SLAB == 0 else tot + P
    return out


@pytest.fixture(scope="module")
def data():
    s = GM.gram_states(N, 21)
    orc, m = make_oracle("pinball_simple")
    phi = orc.features(*s)
    Y = np.random.default_rng(23).standard_normal((T, N)).astype(np.float32)
    for c in range(5):                                                # +-0, a subnormal, +-1e30: placed differently per column
        Y[c, EDGE_AT] = np.roll(EDGE_VALUES, c)
    ctx = {b: ScgContext(64, 0, m, device=0, block_envs=b, **HP) for b in (256, 64, 128)}
    model = prefix_rhs(phi, Y, set(NS))
    yield dict(s=s, phi=phi, Y=Y, ctx=ctx, sd=[dev(v) for v in s], Yd=dev(Y), model=model)
    for c in ctx.values():
        c.close()


def run(data, offsets, n=N, n_tgt=5, build=256, Y=None):
    s = [t[:n].contiguous() for t in data["sd"]]
    Yd = (data["Yd"] if Y is None else Y)[:n_tgt, :n].contiguous()
    A, B = data["ctx"][build].feature_gram_targets(s, offsets, Yd)
    torch.cuda.synchronize()
    assert A.shape == (len(offsets) - 1, NF, NF) and B.shape == (len(offsets) - 1, n_tgt, NF)
    return A.cpu().numpy(), B.cpu().numpy()


def single(data, offsets, n, c, Y=None):
    """scg_feature_gram on the same states with yv = Y[c]."""
    s = [t[:n].contiguous() for t in data["sd"]]
    A, b = data["ctx"][256].feature_gram(s, offsets, (data["Yd"] if Y is None else Y)[c, :n].contiguous())
    torch.cuda.synchronize()
    return A.cpu().numpy(), b.cpu().numpy()


def check_one_segment(data, n, n_tgt):
    A, B = run(data, [0, n], n, n_tgt)
    for c in range(n_tgt):
        A1, b1 = single(data, [0, n], n, c)
        if c == 0:
            assert_bits_equal(A, A1, msg=f"n {n} n_tgt {n_tgt}: A against scg_feature_gram's:")
        assert_bits_equal(B[0][c], b1[0], msg=f"n {n} n_tgt {n_tgt}: B[0][{c}] against scg_feature_gram's b:")
        assert_bits_equal(B[0][c], data["model"][n][c], msg=f"n {n} n_tgt {n_tgt}: B[0][{c}] against the model:")
    assert A[0][0, 0] == n
    return A, B


def test_the_one_pass_model_is_gram_models_rhs(data):
    for n, c in ((1025, 3), (5, 0)):
        assert_bits_equal(data["model"][n][c], GM.rhs(data["phi"][:n], data["Y"][c, :n], [0, n])[0], msg=f"n {n} column {c}:")


@pytest.mark.parametrize("n", NS)
def test_five_targets_equal_feature_gram_and_the_model_by_bits(data, n):
    check_one_segment(data, n, 5)


@pytest.mark.parametrize("n_tgt", [1, 2, 15, 16])
def test_every_target_count_equals_feature_gram_and_the_model_by_bits(data, n_tgt):
    check_one_segment(data, 1025, n_tgt)


@pytest.mark.parametrize("name", list(SEGMENTATIONS))
def test_segmentations_equal_the_model_by_bits(data, name):
    off = SEGMENTATIONS[name]
    A, B = run(data, off)
    want = rhs_multi(data["phi"], data["Y"][:5], off)
    A1 = None
    for c in range(5):
        A1, b1 = single(data, off, N, c)
        for g in range(len(off) - 1):
            assert_bits_equal(B[g][c], want[g][c], msg=f"{name}: B[{g}][{c}] against the model:")
            assert_bits_equal(B[g][c], b1[g], msg=f"{name}: B[{g}][{c}] against scg_feature_gram's b:")
    assert_bits_equal(A, A1, msg=f"{name}: A against scg_feature_gram's:")
    for g in range(len(off) - 1):
        assert A[g][0, 0] == off[g + 1] - off[g]
        if off[g + 1] == off[g]:                                      # an empty segment: all +0
            assert not A[g].view(np.uint32).any() and not B[g].view(np.uint32).any()


def test_a_target_does_not_depend_on_its_neighbours(data):
    off = [3, 1030, 2049]
    A16, B16 = run(data, off, n_tgt=16)
    A2, B2 = run(data, off, n_tgt=2)
    assert_bits_equal(B2, B16[:, :2], msg="targets 0, 1 alone against the same among 16:")
    assert_bits_equal(A2, A16, msg="A with 2 against 16 targets:")
    A5, B5 = run(data, off)
    assert_bits_equal(B5, B16[:, :5], msg="targets 0 .. 4 against the same among 16:")
    bad = data["Yd"].clone()
    bad[1] = float("nan")
    bad[3, [0, 1500]] = float("inf")
    Ab, Bb = run(data, off, Y=bad)
    assert_bits_equal(Ab, A5, msg="A beside a NaN and an inf target:")
    for c in (0, 2, 4):
        assert_bits_equal(Bb[:, c], B5[:, c], msg=f"target {c} beside a NaN and an inf target:")


def test_same_bits_from_every_block_build(data):
    off = SEGMENTATIONS["five segments, starts off the multiples of 4"]
    want = run(data, off, build=256)
    for b in (64, 128):
        assert data["ctx"][b].block_envs == b
        got = run(data, off, build=b)
        assert_bits_equal(got[0], want[0], msg=f"A, {b}-env build:")
        assert_bits_equal(got[1], want[1], msg=f"B, {b}-env build:")


# ---------------------------------------------------------------------------------------------------- write set and refusals

GUARD = 4099                  # floats either side (odd: the outputs sit at a 4-byte-aligned address only)
FILL = -12345.5


def raw_call(ctx, n, s, Y, n_tgt, offsets, A, B, n_seg=None):
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64)
    p = lambda t: C.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    rc = ctx.lib.scg_feature_gram_targets(ctx._ctx, C.c_int64(n), *[p(t) for t in s], p(Y), n_tgt, len(off) - 1 if n_seg is None else n_seg,
                                          None if off is None else off.ctypes.data_as(C.c_void_p), p(A), p(B), ctx._stream())
    torch.cuda.synchronize()
    return rc


def guarded(n_seg, room):
    """A and a B buffer with room for `room` targets a segment, both between guard bands, all on the sentinel."""
    bufA = torch.full((2 * GUARD + n_seg * NF * NF,), FILL, dtype=torch.float32, device="cuda:0")
    bufB = torch.full((2 * GUARD + n_seg * room * NF,), FILL, dtype=torch.float32, device="cuda:0")
    return bufA, bufB, bufA.data_ptr() + 4 * GUARD, bufB.data_ptr() + 4 * GUARD


@pytest.mark.parametrize("n_tgt", [1, 5])
def test_writes_A_and_n_tgt_rows_of_B_only(data, n_tgt):
    """B sits in a buffer with room for 16 targets a segment: not a float beyond n_seg * n_tgt * 1296 changes (a lane of a zero
    column that stored would write there)."""
    ctx, off = data["ctx"][256], [2, 900, 900, 2040]
    bufA, bufB, pA, pB = guarded(3, T)
    s = [t.clone() for t in data["sd"]]
    Yd = data["Yd"][:n_tgt].clone()
    assert raw_call(ctx, N, s, Yd, n_tgt, off, pA, pB) == 0
    for buf, body in ((bufA, 3 * NF * NF), (bufB, 3 * n_tgt * NF)):
        h = buf.cpu().numpy()
        assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + body:] == FILL)
        assert not np.any(h[GUARD: GUARD + body] == FILL)             # fully overwritten, the empty segment too
    A, B = run(data, off, n_tgt=n_tgt)
    assert_bits_equal(bufA.cpu().numpy()[GUARD: GUARD + 3 * NF * NF].reshape(3, NF, NF), A, msg="A at an odd address:")
    assert_bits_equal(bufB.cpu().numpy()[GUARD: GUARD + 3 * n_tgt * NF].reshape(3, n_tgt, NF), B, msg="B at an odd address:")
    for t, w in zip(s + [Yd], data["sd"] + [data["Yd"][:n_tgt]]):
        assert torch.equal(t, w)


def test_refusals_leave_A_and_B_untouched_and_n_zero_zeroes_them(data):
    ctx = data["ctx"][256]
    bufA, bufB, pA, pB = guarded(1, T)
    s, Yd = data["sd"], data["Yd"][:5].contiguous()
    refused = {
        "n_tgt = 0": dict(n_tgt=0), "n_tgt = 17": dict(n_tgt=17), "null Y": dict(Y=None), "null B": dict(B=None),
        "offsets decrease": dict(offsets=[0, 9, 5]),
        "null x": dict(s=[None] + s[1:]), "null A": dict(A=None), "null offsets": dict(offsets=None, n_seg=1),
        "n < 0": dict(n=-1, offsets=[0, 0]), "n_seg = 0": dict(offsets=[0]), "n_seg = 65": dict(offsets=list(range(66))),
        "offsets beyond n": dict(offsets=[0, N + 1]),
    }
    for name, kw in refused.items():
        a = dict(n=N, s=s, Y=Yd, n_tgt=5, offsets=[0, N], A=pA, B=pB)
        a.update(kw)
        assert raw_call(ctx, a["n"], a["s"], a["Y"], a["n_tgt"], a["offsets"], a["A"], a["B"], a.get("n_seg")) == -1, name
        assert b"scg_feature_gram_targets" in ctx.lib.scg_last_error(ctx._ctx), name
        assert torch.all(bufA == FILL) and torch.all(bufB == FILL), name
    assert b"n_tgt" in (raw_call(ctx, N, s, Yd, 17, [0, N], pA, pB), ctx.lib.scg_last_error(ctx._ctx))[1]
    # the sequence: scg_feature_gram's checks come before n_tgt's
    assert b"offsets" in (raw_call(ctx, N, s, Yd, 0, [0, 9, 5], pA, pB), ctx.lib.scg_last_error(ctx._ctx))[1]
    assert torch.all(bufA == FILL) and torch.all(bufB == FILL)
    assert raw_call(ctx, 0, s, Yd, 5, [0, 0], pA, pB) == 0            # n = 0: zeroed, nothing else
    hA, hB = bufA.cpu().numpy(), bufB.cpu().numpy()
    assert not hA[GUARD: GUARD + NF * NF].view(np.uint32).any() and not hB[GUARD: GUARD + 5 * NF].view(np.uint32).any()
    assert np.all(hA[:GUARD] == FILL) and np.all(hA[GUARD + NF * NF:] == FILL)
    assert np.all(hB[:GUARD] == FILL) and np.all(hB[GUARD + 5 * NF:] == FILL)
    A, B = ctx.feature_gram_targets([t[:0] for t in s], [0, 0, 0], Yd[:, :0])      # ... and through the wrapper, from empty tensors
    assert A.shape == (2, NF, NF) and B.shape == (2, 5, NF)
    assert not A.cpu().numpy().view(np.uint32).any() and not B.cpu().numpy().view(np.uint32).any()
    for bad in (Yd[:, :5].contiguous(), Yd[0], torch.zeros((17, N), dtype=torch.float32, device="cuda:0"), Yd.cpu(), Yd.double()):
        with pytest.raises(scg.ScgError):
            ctx.feature_gram_targets(s, [0, N], bad)
    with pytest.raises(scg.ScgError):
        ctx.feature_gram_targets(s, [0, N + 1], Yd)
