"""scg_feature_gram (SPEC §16.1) against the host model of tests/gram_model.py: bit for bit on a fixed index set (all of b),
the whole matrix against the float64 Gram inside the derived chain bound, independence of the block build and of the order the
segments are listed in, write set and refusals."""
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
IDX = GM.index_set(_lib.GRAM_MACRO_TILE)
SEGMENTATIONS = {
    "five segments, starts off the multiples of 4": [0, 5, 410, 411, 1437, 2049],
    "a segment across the array's slab edge": [1000, 1050],           # one slab of 50, not 24 + 26
    "slabs are cut per segment": [3, 1030, 2049],                     # the second segment's first slab starts at 1030
    "an empty segment in the middle and one at the end": [0, 700, 700, 1300, 1300],
    "samples outside every segment": [7, 1000, 2001],
}


@pytest.fixture(scope="module")
def data():
    """The states, their features by the oracle, yv with +-0, a subnormal and 1e30 in it; one context per block build."""
    s = GM.gram_states(N, 21)
    orc, m = make_oracle("pinball_simple")
    phi = orc.features(*s)
    yv = np.random.default_rng(22).standard_normal(N).astype(np.float32)
    yv[[0, 2, 4, 1023, 1024, 2048]] = np.array([0.0, -0.0, 1e-41, 1e30, -1e30, 1e-41], np.float32)
    ctx = {b: ScgContext(64, 0, m, device=0, block_envs=b, **HP) for b in (256, 64, 128)}
    yield dict(s=s, phi=phi, yv=yv, ctx=ctx, sd=[dev(v) for v in s], yd=dev(yv))
    for c in ctx.values():
        c.close()


def run(data, offsets, n=N, build=256, rhs=True):
    s = [t[:n].contiguous() for t in data["sd"]]
    out = data["ctx"][build].feature_gram(s, offsets, data["yd"][:n].contiguous() if rhs else None)
    torch.cuda.synchronize()
    return (out[0].cpu().numpy(), out[1].cpu().numpy()) if rhs else out.cpu().numpy()


def check_bits(data, offsets, n, name):
    A, b = run(data, offsets, n)
    sub = A[np.ix_(range(A.shape[0]), IDX, IDX)]
    assert_bits_equal(sub, GM.gram(data["phi"][:n], offsets, IDX, IDX), msg=f"{name}: A on the index set:")
    assert_bits_equal(b, GM.rhs(data["phi"][:n], data["yv"][:n], offsets), msg=f"{name}: b:")
    assert_bits_equal(A, A.transpose(0, 2, 1), msg=f"{name}: A against its transpose:")
    return A, b


def test_index_set_covers_the_shipped_tiling():
    assert len(IDX) == 48 and {0, 15, 16, 17, 1279, 1280, 1295} <= set(IDX)
    for e in range(_lib.GRAM_MACRO_TILE, NF, _lib.GRAM_MACRO_TILE):
        assert e - 1 in IDX and e in IDX


@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 1023, 1024, 1025, 2049])
def test_one_segment_equals_the_model_by_bits(data, n):
    A, _ = check_bits(data, [0, n], n, f"n = {n}")
    assert A[0][0, 0] == n                                           # phi_0 = 1, exactly


@pytest.mark.parametrize("name", list(SEGMENTATIONS))
def test_segmentations_equal_the_model_by_bits(data, name):
    off = SEGMENTATIONS[name]
    A, b = check_bits(data, off, N, name)
    for g in range(len(off) - 1):
        assert A[g][0, 0] == off[g + 1] - off[g]
        if off[g + 1] == off[g]:                                     # an empty segment: all +0
            assert not A[g].view(np.uint32).any() and not b[g].view(np.uint32).any()


def test_whole_matrix_inside_the_chain_bound_symmetric_and_counting(data):
    off = [0, 5, 2049]
    A = run(data, off, rhs=False)
    ref, bound = GM.chain_bound(data["phi"], off)
    err = np.abs(A.astype(np.float64) - ref)
    print(f"largest |A - A64| / bound: {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    model = GM.gram(data["phi"], off, IDX, IDX)                       # the model itself stays inside it
    assert np.all(np.abs(model.astype(np.float64) - ref[np.ix_(range(2), IDX, IDX)]) <= bound[np.ix_(range(2), IDX, IDX)])
    assert_bits_equal(A, A.transpose(0, 2, 1), msg="A against its transpose:")
    assert A[0][0, 0] == 5 and A[1][0, 0] == 2044
    A2, _ = run(data, off)                                           # the same A with and without b
    assert_bits_equal(A2, A, msg="A with yv given:")


def test_same_bits_from_every_block_build(data):
    off = SEGMENTATIONS["five segments, starts off the multiples of 4"]
    want = run(data, off, build=256)
    for b in (64, 128):
        assert data["ctx"][b].block_envs == b
        got = run(data, off, build=b)
        assert_bits_equal(got[0], want[0], msg=f"A, {b}-env build:")
        assert_bits_equal(got[1], want[1], msg=f"b, {b}-env build:")


def test_same_bits_when_the_segments_are_listed_in_another_order(data):
    off = np.array(SEGMENTATIONS["five segments, starts off the multiples of 4"])
    want = run(data, off)
    perm = [3, 0, 4, 2, 1]
    order = np.concatenate([np.arange(off[g], off[g + 1]) for g in perm])
    s = [dev(v[order]) for v in data["s"]]
    off2 = np.concatenate([[0], np.cumsum([off[g + 1] - off[g] for g in perm])])
    A, b = data["ctx"][256].feature_gram(s, off2, dev(data["yv"][order]))
    for i, g in enumerate(perm):
        assert_bits_equal(A[i].cpu().numpy(), want[0][g], msg=f"A of segment {g} listed at {i}:")
        assert_bits_equal(b[i].cpu().numpy(), want[1][g], msg=f"b of segment {g} listed at {i}:")


# ---------------------------------------------------------------------------------------------------- write set and refusals

GUARD = 4099                  # floats either side (odd: the outputs sit at a 4-byte-aligned address only)
FILL = -12345.5


def raw_call(ctx, n, s, yv, offsets, A, b, n_seg=None):
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64)
    p = lambda t: C.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    rc = ctx.lib.scg_feature_gram(ctx._ctx, C.c_int64(n), *[p(t) for t in s], p(yv), len(off) - 1 if n_seg is None else n_seg,
                                  None if off is None else off.ctypes.data_as(C.c_void_p), p(A), p(b), ctx._stream())
    torch.cuda.synchronize()
    return rc


def guarded(n_seg):
    bufA = torch.full((2 * GUARD + n_seg * NF * NF,), FILL, dtype=torch.float32, device="cuda:0")
    bufb = torch.full((2 * GUARD + n_seg * NF,), FILL, dtype=torch.float32, device="cuda:0")
    return bufA, bufb, bufA.data_ptr() + 4 * GUARD, bufb.data_ptr() + 4 * GUARD


def test_writes_A_and_b_only(data):
    ctx, off = data["ctx"][256], [2, 900, 900, 2040]
    bufA, bufb, pA, pb = guarded(3)
    s = [t.clone() for t in data["sd"]]
    yd = data["yd"].clone()
    assert raw_call(ctx, N, s, yd, off, pA, pb) == 0
    for buf, body in ((bufA, 3 * NF * NF), (bufb, 3 * NF)):
        h = buf.cpu().numpy()
        assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + body:] == FILL)
        assert not np.any(h[GUARD: GUARD + body] == FILL)             # fully overwritten, the empty segment too
    A, b = run(data, off)
    assert_bits_equal(bufA.cpu().numpy()[GUARD: GUARD + 3 * NF * NF].reshape(3, NF, NF), A, msg="A at an odd address:")
    assert_bits_equal(bufb.cpu().numpy()[GUARD: GUARD + 3 * NF].reshape(3, NF), b, msg="b at an odd address:")
    for t, w in zip(s + [yd], data["sd"] + [data["yd"]]):
        assert torch.equal(t, w)


def test_refusals_leave_A_untouched_and_n_zero_zeroes_it(data):
    ctx = data["ctx"][256]
    bufA, bufb, pA, pb = guarded(1)
    s, yd = data["sd"], data["yd"]
    refused = {
        "null x": dict(s=[None] + s[1:]), "null vy": dict(s=s[:3] + [None]), "null A": dict(A=None, b=None, yv=None),
        "null offsets": dict(offsets=None, n_seg=1), "n < 0": dict(n=-1, offsets=[0, 0]),
        "n_seg = 0": dict(offsets=[0]), "n_seg = 65": dict(offsets=list(range(66))),
        "offsets decrease": dict(offsets=[0, 9, 5]), "offsets[0] < 0": dict(offsets=[-1, 5]),
        "offsets beyond n": dict(offsets=[0, N + 1]), "yv without b": dict(b=None), "b without yv": dict(yv=None),
    }
    for name, kw in refused.items():
        a = dict(n=N, s=s, yv=yd, offsets=[0, N], A=pA, b=pb)
        a.update(kw)
        assert raw_call(ctx, a["n"], a["s"], a["yv"], a["offsets"], a["A"], a["b"], a.get("n_seg")) == -1, name
        assert b"scg_feature_gram" in ctx.lib.scg_last_error(ctx._ctx), name
        assert torch.all(bufA == FILL) and torch.all(bufb == FILL), name
    assert raw_call(ctx, 0, s, yd, [0, 0], pA, pb) == 0              # n = 0: zeroed, nothing else
    hA, hb = bufA.cpu().numpy(), bufb.cpu().numpy()
    assert not hA[GUARD: GUARD + NF * NF].view(np.uint32).any() and not hb[GUARD: GUARD + NF].view(np.uint32).any()
    assert np.all(hA[:GUARD] == FILL) and np.all(hA[GUARD + NF * NF:] == FILL)
    A = ctx.feature_gram([t[:0] for t in s], [0, 0, 0])              # ... and through the wrapper, from empty tensors
    assert A.shape == (2, NF, NF) and not A.cpu().numpy().view(np.uint32).any()
    with pytest.raises(scg.ScgError):
        ctx.feature_gram(s, [0, N + 1])
    with pytest.raises(scg.ScgError):
        ctx.feature_gram(s, [0, N], yd[:5])


def test_needs_no_map(data):
    """A context that never saw scg_set_map: the Gram does not return SCG_ERR_STATE (the step does)."""
    lib = data["ctx"][256].lib
    raw = C.c_void_p()
    cfg = _lib.ScgConfig(n_envs=4, n_options=0, fourier_order=5, device=0, gamma=0.99, max_episode_steps=10, max_option_steps=5)
    assert lib.scg_create(C.byref(raw), C.byref(cfg)) == 0
    try:
        A = torch.empty((1, NF, NF), dtype=torch.float32, device="cuda:0")
        off = np.array([0, 4], np.int64)
        rc = lib.scg_feature_gram(raw, C.c_int64(4), *[C.c_void_p(t.data_ptr()) for t in data["sd"]], None, 1,
                                  off.ctypes.data_as(C.c_void_p), C.c_void_p(A.data_ptr()), None, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.scg_last_error(raw)
        assert_bits_equal(A.cpu().numpy()[0][np.ix_(IDX, IDX)], GM.gram(data["phi"], [0, 4], IDX, IDX)[0], msg="A without a map:")
        assert lib.scg_step(raw, *([None] * 13), 0, 0, 0, None) == -4
    finally:
        lib.scg_destroy(raw)
