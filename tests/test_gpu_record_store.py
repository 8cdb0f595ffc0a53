"""SPEC §30.1 on the device: scg_record_append, scg_record_offsets and scg_record_pack driven through the C-ABI on synthetic launch
buffers, against the rules restated here in numpy. Every array a kernel writes lies inside a longer allocation (guard bands), and
the whole allocation is compared: what a call may not write must keep its fill."""
import ctypes as C

import numpy as np
import pytest
import torch

import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd._lib import ROW_NONE, Record, RecordStore
from skill_chaining_with_graphs_amd.core import ScgContext
from gpu_util import dev
from util import HP

pytestmark = pytest.mark.gpu

F4 = ("x", "y", "vx", "vy", "reward")
F1 = ("action", "done", "vf", "term", "option_id")
FIELDS = F4 + F1
GUARD = 96                 # elements on either side of every output
FILL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = ScgContext(64, 2, scg.load_map("pinball_simple"), device=0, block_envs=256, **HP)
    yield c
    c.close()


def np_dtype(f):
    return np.uint32 if f in F4 else np.uint8          # (4-byte fields as their bits: every pattern, NaNs included, must survive)


class Banded:
    """A device buffer of `count` elements with GUARD elements of fill on either side; `ptr` is the inner array's address."""

    def __init__(self, count, dtype, inner=None):
        self.count, self.dtype = int(count), np.dtype(dtype)
        host = np.full(self.count + 2 * GUARD, FILL, np.uint8).repeat(self.dtype.itemsize).view(self.dtype).copy()
        if inner is not None:
            host[GUARD: GUARD + self.count] = np.asarray(inner, self.dtype).reshape(-1)
        self.start = host.copy()
        self.t = dev(host.view(np.uint8))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + GUARD * self.dtype.itemsize)

    def host(self):
        return self.t.cpu().numpy().view(self.dtype)

    def inner(self):
        return self.host()[GUARD: GUARD + self.count]

    def expect(self, inner):
        want = self.start.copy()
        want[GUARD: GUARD + self.count] = np.asarray(inner, self.dtype).reshape(-1)
        return want


def up(v):
    return dev(v.view(np.int32) if v.dtype == np.uint32 else v)


def launch_buffers(rng, n, rows, skip=()):
    return {f: (rng.integers(0, 2 ** 32, (rows, n), dtype=np.uint64).astype(np.uint32) if f in F4
                else rng.integers(0, 256, (rows, n), dtype=np.uint64).astype(np.uint8)) for f in FIELDS if f not in skip}


def call_append(ctx, launch, ln, store, have, overflow, n, rows, cap):
    keep = {f: up(v) for f, v in launch.items()}
    ln_d = dev(np.asarray(ln, np.int32))
    rec = Record(first=0, n=n, rows=rows, len=C.c_void_p(ln_d.data_ptr()), **{f: C.c_void_p(t.data_ptr()) for f, t in keep.items()})
    st = RecordStore(have=have.ptr, overflow=overflow.ptr, **{f: b.ptr for f, b in store.items()})
    rc = ctx.lib.scg_record_append(ctx._ctx, C.byref(rec), C.byref(st), cap, None)
    torch.cuda.synchronize()
    return rc


def model_append(store, have, overflow, launch, ln, cap):
    """dst[e][have[e] + r] = src[r][e] for r < len[e]; rows that pass cap are dropped and counted; have stops at cap."""
    for e in range(len(have)):
        for r in range(int(ln[e])):
            at = have[e] + r
            if at >= cap:
                overflow[0] += 1
                continue
            for f in store:
                if f in launch:
                    store[f][e, at] = launch[f][r, e]
        have[e] = min(have[e] + int(ln[e]), cap)


def lens_of(rng, n, rows, cap):
    """Two appends' len per env: random with 0 and `rows` among them and every env inside cap, but env 0 ending exactly at cap (n >= 2)
    and the last env passing it."""
    l1 = rng.integers(0, rows + 1, n)
    l2 = np.minimum(rng.integers(0, rows + 1, n), cap - l1)
    if n >= 4:
        l1[1], l2[1] = 0, rows
        l1[2], l2[2] = rows, 0
    if n >= 2:
        l1[0], l2[0] = rows, cap - rows
    l1[n - 1], l2[n - 1] = rows, rows
    return l1.astype(np.int32), l2.astype(np.int32)


def run_append_case(ctx, n, rows, seed=0):
    rng = np.random.default_rng(1000 * n + rows + seed)
    cap = rows + rows // 2 if rows > 1 else 1
    l1, l2 = lens_of(rng, n, rows, cap)
    assert l1[n - 1] + l2[n - 1] > cap and (n < 2 or l1[0] + l2[0] == cap)
    kept = [f for f in FIELDS if f != "term"]                  # the store keeps no term; the launches record no vy
    store = {f: Banded(n * cap, np_dtype(f)) for f in kept}
    have, overflow = Banded(n, np.int32, np.zeros(n)), Banded(1, np.int32, [0])
    m_store = {f: store[f].inner().reshape(n, cap).copy() for f in kept}
    m_have, m_over = np.zeros(n, np.int64), np.zeros(1, np.int64)
    for ln in (l1, l2):
        launch = launch_buffers(rng, n, rows, skip=("vy",))
        assert call_append(ctx, launch, ln, store, have, overflow, n, rows, cap) == 0
        model_append(m_store, m_have, m_over, launch, ln, cap)
    assert m_over[0] == l1[n - 1] + l2[n - 1] - cap and m_have[n - 1] == cap
    out = {f: store[f].host() for f in kept}
    for f in kept:
        assert np.array_equal(out[f], store[f].expect(m_store[f])), f"n {n} rows {rows}: {f}"
    assert np.array_equal(out["vy"], store["vy"].start), "a field the launch does not record was written"
    assert np.array_equal(have.host(), have.expect(m_have)) and np.array_equal(overflow.host(), overflow.expect(m_over))
    return out, have.host(), overflow.host()


@pytest.mark.parametrize("rows", [1, 64, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_two_appends_equal_the_rule_and_write_nothing_else(ctx, n, rows):
    run_append_case(ctx, n, rows)


def test_the_three_block_builds_give_the_same_bits(ctx):
    want = run_append_case(ctx, 130, 65)
    flat, tabs = run_pack_case(ctx)
    for b in (64, 128):
        c = ScgContext(64, 2, scg.load_map("pinball_simple"), device=0, block_envs=b, **HP)
        try:
            got = run_append_case(c, 130, 65)
            flat_b, tabs_b = run_pack_case(c)
        finally:
            c.close()
        for f in want[0]:
            assert np.array_equal(got[0][f], want[0][f]), (b, f)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert all(np.array_equal(flat[f], flat_b[f]) for f in flat) and all(np.array_equal(tabs[f], tabs_b[f]) for f in tabs)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130, 1024, 2500])
def test_offsets_are_the_exclusive_scan(ctx, n):
    rng = np.random.default_rng(n)
    have = rng.integers(0, 2 ** 31 - 1 if n in (65, 2500) else 1000, n).astype(np.int32)       # (sums past 2^31 need the int64)
    have_d = dev(have) if n else None
    off = Banded(n + 1, np.int64)
    rc = ctx.lib.scg_record_offsets(ctx._ctx, n, C.c_void_p(have_d.data_ptr() if n else 0), off.ptr, None)
    torch.cuda.synchronize()
    assert rc == 0
    want = np.concatenate([[0], np.cumsum(have.astype(np.int64))])
    assert np.array_equal(off.host(), off.expect(want))


# ---------------------------------------------------------------------------------------------------- pack

def pack_record(rng, cap=9):
    """Five envs: none, one row (its begin row), an episode that ends done on its last row, a record cut before its episode ended
    (done = 0 on its last row), and a full one at cap with an option that goes on, ends and is entered again."""
    L = np.array([0, 1, 6, 5, cap], np.int32)
    n = len(L)
    store = {f: (rng.integers(0, 2 ** 32, (n, cap), dtype=np.uint64).astype(np.uint32) if f in F4
                 else rng.integers(0, 256, (n, cap), dtype=np.uint64).astype(np.uint8)) for f in FIELDS}
    for e in range(n):
        store["done"][e, :] = 0
        store["done"][e, 0] = 2                                # a begin row
        store["vf"][e, :] = rng.integers(0, 3, cap)
        store["term"][e, :] = rng.choice([0, 0, 1, 4, 5], cap)
    store["done"][2, L[2] - 1] = 1                             # ends done; env 3 stays cut
    store["vf"][4, :] = [0, 2, 2, 2, 0, 2, 2, 1, 1]
    store["term"][4, :] = [0, 0, 0, 1, 0, 0, 4, 0, 0]
    store["done"][4, 4] = 1                                    # (an episode's end inside a record: the rule is per row)
    return store, L, n, cap


def model_pack(store, off, total, n, cap, fill):
    """The flat record and the tables by the rules of SPEC §30.1, with the kernel's clamps; rows no env owns keep `fill`."""
    flat = {f: fill[f].copy() for f in fill}
    for e in range(n):
        lo = min(max(int(off[e]), 0), total)
        hi = min(max(int(off[e + 1]), lo), total)
        Le = min(hi - lo, cap)
        for r in range(Le):
            i = lo + r
            for f in FIELDS:
                flat[f][i] = store[f][e, r]
            done, vf, term = int(store["done"][e, r]), int(store["vf"][e, r]), int(store["term"][e, r])
            flat["env"][i], flat["row"][i] = e, r
            flat["tab0"][i] = 0 if done == 0 else ROW_NONE
            flat["tabk"][i] = vf if (vf >= 1 and term == 0 and done == 0) else ROW_NONE
            flat["tabA"][i] = store["vf"][e, r + 1] if (r + 1 < Le and (r == 0 or done == 0)) else ROW_NONE
    return flat


OUT_DTYPES = {**{f: np_dtype(f) for f in FIELDS}, "env": np.int32, "row": np.int32, "tab0": np.uint8, "tabk": np.uint8, "tabA": np.uint8}


def call_pack(ctx, store, n, cap, off, total, skip=(), alloc=None):
    keep = {f: up(v) for f, v in store.items()}
    have_d, over_d = dev(np.zeros(max(n, 1), np.int32)), dev(np.zeros(1, np.int32))
    st = RecordStore(have=C.c_void_p(have_d.data_ptr()), overflow=C.c_void_p(over_d.data_ptr()),
                     **{f: C.c_void_p(t.data_ptr()) for f, t in keep.items()})
    off_d = dev(np.asarray(off, np.int64))
    out = {f: Banded(total if alloc is None else alloc, dt) for f, dt in OUT_DTYPES.items()}
    p = lambda f: C.c_void_p(0) if f in skip else out[f].ptr
    rc = ctx.lib.scg_record_pack(ctx._ctx, n, cap, C.byref(st), C.c_void_p(off_d.data_ptr()), C.c_int64(total),
                                 *[p(f) for f in FIELDS], *[p(f) for f in ("env", "row", "tab0", "tabk", "tabA")], None)
    torch.cuda.synchronize()
    return rc, out


def run_pack_case(ctx):
    store, L, n, cap = pack_record(np.random.default_rng(7))
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    total = int(off[-1])
    rc, out = call_pack(ctx, store, n, cap, off, total)
    assert rc == 0
    want = model_pack(store, off, total, n, cap, {f: out[f].start[GUARD: GUARD + total] for f in OUT_DTYPES})
    for f in OUT_DTYPES:
        assert np.array_equal(out[f].host(), out[f].expect(want[f])), f
    # the tables once more, as valuefit.row_tables forms them from the flat record
    done, vf, term, row = want["done"], want["vf"], want["term"], want["row"]
    has_next = row < L[want["env"]] - 1
    nxt = np.concatenate([vf[1:], [0]]).astype(np.uint8)
    assert np.array_equal(out["tab0"].inner(), np.where(done == 0, 0, ROW_NONE).astype(np.uint8))
    assert np.array_equal(out["tabk"].inner(), np.where((vf >= 1) & (term == 0) & (done == 0), vf, ROW_NONE).astype(np.uint8))
    assert np.array_equal(out["tabA"].inner(), np.where(has_next & ((row == 0) | (done == 0)), nxt, ROW_NONE).astype(np.uint8))
    assert done[off[2]] == 2 and done[off[3] - 1] == 1 and done[off[4] - 1] == 0 and out["tabA"].inner()[off[4] - 1] == ROW_NONE
    return {f: out[f].inner().copy() for f in FIELDS}, {f: out[f].inner().copy() for f in ("env", "row", "tab0", "tabk", "tabA")}


def test_pack_equals_the_rules_on_a_record_with_every_kind_of_env(ctx):
    run_pack_case(ctx)


def test_pack_skips_null_outputs_and_an_empty_record_writes_nothing(ctx):
    store, L, n, cap = pack_record(np.random.default_rng(8))
    off = np.concatenate([[0], np.cumsum(L)]).astype(np.int64)
    total = int(off[-1])
    skip = ("vy", "option_id", "row", "tabk")
    rc, out = call_pack(ctx, store, n, cap, off, total, skip=skip)
    assert rc == 0
    want = model_pack(store, off, total, n, cap, {f: out[f].start[GUARD: GUARD + total] for f in OUT_DTYPES})
    for f in OUT_DTYPES:
        assert np.array_equal(out[f].host(), out[f].start if f in skip else out[f].expect(want[f])), f
    rc, out = call_pack(ctx, store, n, cap, np.zeros(n + 1, np.int64), 0, alloc=16)            # total = 0: nothing is launched
    assert rc == 0 and all(np.array_equal(out[f].host(), out[f].start) for f in OUT_DTYPES)


def test_offsets_that_point_outside_are_clamped_and_nothing_is_written_outside(ctx):
    store, _, n, cap = pack_record(np.random.default_rng(9))
    n = 3
    total = 3 + cap + 4
    off = np.array([-5, 3, total + 9, 4], np.int64)            # below 0, beyond total, decreasing; env 1's range is longer than cap
    rc, out = call_pack(ctx, store, n, cap, off, total)
    assert rc == 0
    want = model_pack(store, off, total, n, cap, {f: out[f].start[GUARD: GUARD + total] for f in OUT_DTYPES})
    assert np.array_equal(want["env"][:3 + cap], [0] * 3 + [1] * cap)
    for f in OUT_DTYPES:
        assert np.array_equal(out[f].host(), out[f].expect(want[f])), f


def test_refusals_launch_nothing(ctx):
    store, L, n, cap = pack_record(np.random.default_rng(10))
    lib, h = ctx.lib, ctx._ctx
    have, over = dev(np.zeros(n, np.int32)), dev(np.zeros(1, np.int32))
    ln = dev(np.zeros(n, np.int32))
    q = lambda t: C.c_void_p(t.data_ptr())
    st = RecordStore(have=q(have), overflow=q(over))
    rec = Record(first=0, n=n, rows=4, len=q(ln))
    for bad_rec, bad_st, bad_cap in ((None, st, 4), (rec, None, 4), (Record(first=0, n=n, rows=4), st, 4), (rec, RecordStore(have=q(have)), 4),
                                     (Record(first=0, n=0, rows=4, len=q(ln)), st, 4), (Record(first=0, n=n, rows=0, len=q(ln)), st, 4),
                                     (rec, st, 0)):
        rc = lib.scg_record_append(h, None if bad_rec is None else C.byref(bad_rec), None if bad_st is None else C.byref(bad_st), bad_cap, None)
        assert rc == -1 and b"scg_record_append" in lib.scg_last_error(h)
    off = dev(np.zeros(n + 1, np.int64))
    assert lib.scg_record_offsets(h, -1, q(have), q(off), None) == -1 and lib.scg_record_offsets(h, n, q(have), None, None) == -1
    assert lib.scg_record_offsets(h, n, None, q(off), None) == -1
    nul = [None] * 15
    assert lib.scg_record_pack(h, -1, cap, C.byref(st), q(off), 0, *nul, None) == -1
    assert lib.scg_record_pack(h, n, 0, C.byref(st), q(off), 0, *nul, None) == -1
    assert lib.scg_record_pack(h, n, cap, C.byref(st), q(off), -1, *nul, None) == -1
    assert lib.scg_record_pack(h, n, cap, None, q(off), 0, *nul, None) == -1
    buf = dev(np.zeros(64, np.uint8))
    assert lib.scg_record_pack(h, n, cap, C.byref(st), q(off), 4, q(buf), *nul[1:], None) == -1           # x: the store keeps none
    assert b"does not keep" in lib.scg_last_error(h)
    assert lib.scg_record_pack(h, n, cap, C.byref(st), q(off), 4, *nul[:12], q(buf), None, None, None) == -1      # tab0 without done, vf, term
    assert b"tables need" in lib.scg_last_error(h)
    torch.cuda.synchronize()
    assert int(have.sum()) == 0 and int(over[0]) == 0
