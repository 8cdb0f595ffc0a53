"""SPEC §7 example collection, modelled in numpy from the SPEC's text alone (not from the oracle's sco_harvest /
sco_collect_examples, not from the kernels), and the buffer comparison every collector test uses. Everything here is integer
bookkeeping and data movement: results are compared bit for bit, no tolerance anywhere. (§13's model is tests/frontier_model.py.)

compare_buffers() checks the fill level, every row below it, AND that every element at or beyond the fill level, including a
guard region the test allocated past `cap`, still holds the sentinel the test put there: a stray write past the fill level or past
the buffer is a failure, not an unseen event."""
import numpy as np

XY_SENTINEL_BITS = np.uint32(0xFFC5A5A5)          # a NaN with a payload no ring holds: compared as bits, never as a float
XY_SENTINEL = np.array([XY_SENTINEL_BITS], np.uint32).view(np.float32)[0]
LABEL_SENTINEL = np.uint8(0xA5)                   # neither 0, 1 nor 255


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def harvest(ring_x, ring_y, ev_len, sel_env, l_pos, l_neg):
    """§7 harvest: (xy[n_sel, L, 2] f32, label[n_sel, L] u8). For each listed env and age j = 0 .. L-1: idx = ev_len[e] - 1 - j;
    the example exists iff idx >= 0 and j < ring_len; then xy = ring[idx & (ring_len - 1)][e], label = 1 if j < l_pos else 0;
    otherwise label = 255 (and xy = 0)."""
    ring_len, _ = ring_x.shape
    L = l_pos + l_neg
    sel = np.asarray(sel_env, np.int64).reshape(-1)
    xy = np.zeros((len(sel), L, 2), np.float32)
    lab = np.full((len(sel), L), 255, np.uint8)
    for si, e in enumerate(sel):
        for j in range(L):
            idx = int(ev_len[e]) - 1 - j
            if idx >= 0 and j < ring_len:
                slot = idx & (ring_len - 1)
                xy[si, j, 0], xy[si, j, 1] = ring_x[slot, e], ring_y[slot, e]
                lab[si, j] = 1 if j < l_pos else 0
    return xy, lab


def rows_per_env(events, ev_len, bits, prev_in, L, ring_len):
    """(in, v) per env: in = (events & bits) != 0; v = min(L, ev_len, ring_len) for a hit env (with prev_in: in and not prev_in),
    else 0."""
    inn = (np.asarray(events, np.int64) & int(bits)) != 0
    hit = inn if prev_in is None else inn & (np.asarray(prev_in) == 0)
    el = np.asarray(ev_len, np.int64)
    return inn, np.where(hit, np.maximum(np.minimum(np.minimum(L, el), ring_len), 0), 0)


def collect(ring_x, ring_y, events, ev_len, bits, prev_in, l_pos, l_neg, ex_xy, ex_label, count, cap=None):
    """§7 collect, in place: ex_xy[>= cap, 2] f32, ex_label[>= cap] u8, count int32[1]; prev_in u8[N] or None. `cap` defaults to
    len(ex_label); pass it when the arrays carry a guard region behind the buffer. Envs in env order: in = (events & bits) != 0;
    with prev_in hit = in and not prev_in[e], and prev_in[e] = in; otherwise hit = in. A hit env appends its
    v = min(l_pos + l_neg, ev_len, ring_len) rows, ages 0 .. v-1, at count, count + 1, ...; positions outside the buffer are
    dropped; count = min(cap, count + sum v)."""
    ring_len, n = ring_x.shape
    cap = len(ex_label) if cap is None else int(cap)
    L = l_pos + l_neg
    inn, v = rows_per_env(events, ev_len, bits, prev_in, L, ring_len)
    if prev_in is not None:
        prev_in[:] = inn.astype(np.uint8)
    el = np.asarray(ev_len, np.int64)
    total = int(v.sum())
    first = np.cumsum(v) - v                              # rows of the envs before e
    env = np.repeat(np.arange(n), v)
    age = np.arange(total) - np.repeat(first, v)          # 0 .. v-1 inside each env: ascending
    pos = int(count[0]) + np.arange(total)
    keep = (pos >= 0) & (pos < cap)
    env, age, pos = env[keep], age[keep], pos[keep]
    slot = (el[env] - 1 - age) & (ring_len - 1)
    ex_xy[pos, 0] = ring_x[slot, env]
    ex_xy[pos, 1] = ring_y[slot, env]
    ex_label[pos] = (age < l_pos).astype(np.uint8)
    count[0] = min(cap, int(count[0]) + total)


def _first(bad):
    return int(np.nonzero(bad)[0][0])


def compare_buffers(got_xy, got_label, got_count, want_xy, want_label, want_count, cap, guard, *, got_prev=None, want_prev=None,
                    what=""):
    """One example buffer against the model's. The arrays hold cap + guard rows (xy[cap + guard, 2], label[cap + guard]); both
    sides started from the same contents (sentinels, and whatever the case pre-filled below count_0) and the model ran in place on
    `want_*`. Raises AssertionError naming the field and the first offending position."""
    tag = f"{what}: " if what else ""
    gx, wx = _bits(got_xy).reshape(-1, 2), _bits(want_xy).reshape(-1, 2)
    gl, wl = np.asarray(got_label, np.uint8).reshape(-1), np.asarray(want_label, np.uint8).reshape(-1)
    assert gx.shape[0] == wx.shape[0] == gl.shape[0] == wl.shape[0] == cap + guard, f"{tag}buffer shapes do not fit cap + guard"
    gc, wc = int(np.asarray(got_count).reshape(-1)[0]), int(np.asarray(want_count).reshape(-1)[0])
    assert gc <= cap, f"{tag}count = {gc} is not clamped to cap = {cap}"
    assert gc == wc, f"{tag}count = {gc}, the model has {wc}"
    k = max(wc, 0)
    bad = np.any(gx[:k] != wx[:k], 1)
    assert not bad.any(), (f"{tag}ex_xy differs first at position {_first(bad)} of {k}: got bits {gx[_first(bad)].tolist()}, "
                           f"want {wx[_first(bad)].tolist()} ({int(bad.sum())} rows differ)")
    bad = gl[:k] != wl[:k]
    assert not bad.any(), (f"{tag}ex_label differs first at position {_first(bad)} of {k}: got {gl[_first(bad)]}, "
                           f"want {wl[_first(bad)]} ({int(bad.sum())} rows differ)")
    for name, bad in (("ex_xy", np.any(gx[k:] != XY_SENTINEL_BITS, 1)), ("ex_label", gl[k:] != LABEL_SENTINEL)):
        if bad.any():
            p = k + _first(bad)
            where = "the guard region behind cap" if p >= cap else "the free part of the buffer"
            raise AssertionError(f"{tag}{name} written at position {p} (fill level {k}, cap {cap}): {where} no longer holds "
                                 f"its sentinel ({int(bad.sum())} positions)")
    if want_prev is not None or got_prev is not None:
        gp, wp = np.asarray(got_prev, np.uint8), np.asarray(want_prev, np.uint8)
        bad = gp != wp
        assert not bad.any(), (f"{tag}prev_in differs first at env {_first(bad)}: got {gp[_first(bad)]}, want {wp[_first(bad)]} "
                               f"({int(bad.sum())} envs differ)")


def compare_nodes(got_xy, got_label, got_count, want_xy, want_label, want_count, cap, guard_xy=None, guard_label=None, what=""):
    """§13: compare_buffers for every node's buffer (xy[n_vf, cap, 2], label[n_vf, cap], count[n_vf]; the nodes' buffers lie back
    to back, so a write at position cap of node p is seen as a wrong row 0 or a lost sentinel of node p + 1). Nodes outside the
    target mask are covered too: the model leaves them alone, so their count and every sentinel must be as before.
    `guard_xy` / `guard_label`: the rows the test allocated behind the last node, which must all hold their sentinels."""
    for p in range(len(want_count)):
        compare_buffers(got_xy[p], got_label[p], got_count[p:p + 1], want_xy[p], want_label[p], want_count[p:p + 1], cap, 0,
                        what=f"{what} node {p}".strip())
    if guard_xy is not None:
        bad = np.any(_bits(guard_xy).reshape(-1, 2) != XY_SENTINEL_BITS, 1) | (np.asarray(guard_label).reshape(-1) != LABEL_SENTINEL)
        assert not bad.any(), f"{what}: guard region behind the last node written at row {_first(bad)}"


def fresh_buffers(cap, guard, count0=0, n_nodes=None, rng=None):
    """Sentinel-filled buffers of cap + guard rows (per node with n_nodes) and their count; rows below count_0 hold the examples
    an earlier collection would have left (finite values, labels 0 / 1)."""
    shape = (cap + guard,) if n_nodes is None else (n_nodes, cap + guard)
    xy = np.full(shape + (2,), XY_SENTINEL, np.float32)
    lab = np.full(shape, LABEL_SENTINEL, np.uint8)
    c0 = np.broadcast_to(np.asarray(count0, np.int32), (1,) if n_nodes is None else (n_nodes,)).copy()
    rng = rng or np.random.default_rng(0)
    for p, c in enumerate(c0):
        k = min(max(int(c), 0), cap)
        sl = (slice(0, k),) if n_nodes is None else (p, slice(0, k))
        xy[sl] = rng.uniform(2.0, 3.0, (k, 2)).astype(np.float32)
        lab[sl] = rng.integers(0, 2, k).astype(np.uint8)
    return xy, lab, c0
