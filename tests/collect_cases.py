"""Hand-built traces for the collector tests (SPEC §7, §13), numpy only: the same generators feed the CPU comparison of the models
with the oracle (tests/test_collect_model.py) and the HIP collectors on the GPU (tests/test_gpu_collect_edges.py).

Ring values are unique per (slot, env), so that a wrong index can never read a right value:
  §7   ring_x / ring_y are float32 BIT CODES (0x3F000000 + slot * 2^18 + env, 0x40000000 + env * 256 + slot): finite, normal,
       unique in x and in y alone for ring_len <= 256 and n <= 2^18; the collectors only move them.
  §13  x = 0.5 + (slot * n + env) * 2^-24 (exact in binary32 for slot * n + env < 2^23, unique), y places the state deep inside
       one initiation set or far outside all of them; the sets are bands in y with a small dependence on x.
"""
import numpy as np

from ref64 import clf_model

SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 65536, 65537, 70000, 262144)
CPU_SIZES = tuple(n for n in SIZES if n <= 70000)
DENSITIES = ("none", "all", "env0", "envlast", "lane63", "lane0", "fullrow", "altwaves", "rand1", "rand50", "rand99")
EVLENS = ("zero", "one", "ringm1", "ring", "ringp1", "million", "mixed")
LPN = ((1, 0), (0, 1), (0, 5), (5, 0), (32, 32), (33, 32), (100, 100), (1, 255))
RING_LENS = (1, 2, 64, 256)
N_OPTIONS = 5


def hit_mask(n, density, rng):
    e = np.arange(n)
    if density == "none":
        return np.zeros(n, bool)
    if density == "all":
        return np.ones(n, bool)
    if density == "env0":
        return e == 0
    if density == "envlast":
        return e == n - 1
    if density == "lane63":
        return (e & 63) == 63
    if density == "lane0":
        return (e & 63) == 0
    if density == "fullrow":                          # one full 256-env row between empty rows (row 1; the only row of a small n)
        return (e >> 8) == (1 if n > 256 else 0)
    if density == "altwaves":
        return ((e >> 6) & 1) == 0
    p = {"rand1": 0.01, "rand50": 0.5, "rand99": 0.99}[density]
    return rng.random(n) < p


def ev_lens(n, ring_len, family, hit, rng):
    """ev_len per env: the family's value on the hit envs, anything on the others (they must not matter)."""
    table = {"zero": 0, "one": 1, "ringm1": ring_len - 1, "ring": ring_len, "ringp1": ring_len + 1, "million": 10 ** 6}
    other = rng.integers(0, 4 * ring_len + 2, n)
    if family == "mixed":
        pool = np.array(list(table.values()) + [2, 3, 63, 64, 65, 2 * ring_len + 1], np.int64)
        el = np.where(rng.random(n) < 0.7, pool[rng.integers(0, len(pool), n)], other)
    else:
        el = np.where(hit, table[family], other)
    assert el.min() >= 0
    return el.astype(np.int32)


_CODES = {}


def ring_codes(n, ring_len):
    """§7 ring contents: unique float32 bit codes per (slot, env) (cached: they do not depend on the case)."""
    if (n, ring_len) not in _CODES:
        assert n <= 1 << 18 and ring_len <= 256
        slot = np.arange(ring_len, dtype=np.uint32)[:, None]
        env = np.arange(n, dtype=np.uint32)[None, :]
        rx = (np.uint32(0x3F000000) + (slot << np.uint32(18)) + env).view(np.float32)
        ry = (np.uint32(0x40000000) + (env << np.uint32(8)) + slot).view(np.float32)
        assert np.isfinite(rx).all() and np.isfinite(ry).all()
        _CODES.clear()                                # (one set at a time: the large ones take 0.5 GB)
        _CODES[(n, ring_len)] = (np.ascontiguousarray(rx), np.ascontiguousarray(ry))
    return _CODES[(n, ring_len)]


def build_trace(n, ring_len, family, rng, bits=1):
    """§7 trace: family = (density, ev_len family). Hit envs carry an events byte that meets `bits`, all others a byte that
    does not (bits outside `bits` set at random, so that the mask matters)."""
    density, evf = family
    hit = hit_mask(n, density, rng)
    noise = rng.integers(0, 256, n).astype(np.uint8) & np.uint8(~bits & 0xFF)
    choice = np.array([b for b in range(8) if (bits >> b) & 1], np.int64)
    events = noise | np.where(hit, 1 << choice[rng.integers(0, len(choice), n)], 0).astype(np.uint8)
    ev_len = ev_lens(n, ring_len, evf, hit, rng)
    ring_x, ring_y = ring_codes(n, ring_len)
    return dict(ring_x=ring_x, ring_y=ring_y, events=events, ev_len=ev_len, hit=hit)


def prev_in_random(tr, bits, rng):
    """prev_in with all four (in, prev) combinations per env at random (non-zero bytes other than 1 count as set)."""
    n = len(tr["events"])
    return np.where(rng.random(n) < 0.5, 0, rng.choice(np.array([1, 1, 1, 2, 255], np.uint8), n)).astype(np.uint8)


def total_rows_ok(count0, total):
    assert int(np.max(count0)) + int(total) < 2 ** 31, "count_0 + sum v must stay below 2^31"


# ---------------------------------------------------------------------------------------------------- SPEC §13
BAND_C = (-0.8, -0.4, 0.0, 0.4, 0.8)                  # centres of the sets 1..5 in v = 2 y - 1
BAND_R = 0.1
GAPS = (-0.6, -0.2, 0.2, 0.6, -0.98, 0.97)            # far outside every set


def band_classifiers():
    """clf[6, 8]: set k is the band |v - c_k| < r (z = r^2 - (v - c_k)^2) bent a little along u."""
    clf = np.zeros((N_OPTIONS + 1, 8), np.float32)
    for k, c in enumerate(BAND_C, 1):
        clf[k, :6] = [BAND_R ** 2 - c * c, 0.003, 2 * c, -0.002, 0.001, -1.0]
    return clf


def frontier_ring(n, ring_len, rng):
    """§13 ring: unique exact x, y = the band table entry of a random class per (slot, env). Returns (ring_x, ring_y)."""
    assert n * ring_len < 1 << 23
    code = (np.arange(ring_len, dtype=np.int64)[:, None] * n + np.arange(n, dtype=np.int64)[None, :])
    ring_x = (0.5 + code * 2.0 ** -24).astype(np.float32)
    assert np.array_equal(ring_x.astype(np.float64), 0.5 + code * 2.0 ** -24)          # exactly representable: unique
    v_tab = np.array([c + d for c in BAND_C for d in (-0.05, 0.0, 0.04)] + list(GAPS))
    ring_y = ((v_tab[rng.integers(0, len(v_tab), (ring_len, n))] + 1.0) / 2.0).astype(np.float32)
    return ring_x, ring_y


def inside_sets(clf, x, y, rows=range(1, N_OPTIONS + 1)):
    """inside[k][i]: the float64 sign of z_k at (x, y), and whether every |z_k| clears 4 x its binary32 bound."""
    inside = np.zeros((clf.shape[0], len(x)), bool)
    safe = np.ones(len(x), bool)
    for k in rows:
        z, tol = clf_model(clf[k], x, y)
        inside[k] = z > 0
        safe &= np.abs(z) >= 4 * tol
    return inside, safe


def build_frontier_trace(n, ring_len, family, rng, nodes="mixed"):
    """§13 trace: family as in build_trace; a hit env's events byte names 1, 2 or all 6 nodes (`nodes`: 'one', 'two', 'all',
    'mixed'), the others' bytes name none (bits 6, 7 at random). s_t of every env is classifier-safe: |z_k| >= 4 tol_z for every
    set k, resampled until it is, asserted. Returns the trace with `inside` [6, n] (float64 decision per set) added."""
    density, evf = family
    hit = hit_mask(n, density, rng)
    k_nodes = {"one": np.ones(n, int), "two": np.full(n, 2), "all": np.full(n, 6),
               "mixed": rng.choice(np.array([1, 1, 2, 2, 3, 6]), n)}[nodes]
    order = np.argsort(rng.random((n, 6)), 1)                                          # a random subset of k nodes per env
    ev = ((np.arange(6)[None, :] < k_nodes[:, None]) * (1 << order)).sum(1).astype(np.uint8)
    events = np.where(hit, ev, 0).astype(np.uint8) | (rng.integers(0, 4, n).astype(np.uint8) << np.uint8(6))
    ev_len = ev_lens(n, ring_len, evf, hit, rng)
    ring_x, ring_y = frontier_ring(n, ring_len, rng)
    clf = band_classifiers()
    envs = np.arange(n)
    slot0 = (np.maximum(ev_len.astype(np.int64), 1) - 1) & (ring_len - 1)
    for _ in range(8):
        inside, safe = inside_sets(clf, ring_x[slot0, envs], ring_y[slot0, envs])
        if safe.all():
            break
        bad = np.nonzero(~safe)[0]
        ring_y[slot0[bad], bad] = np.float32((rng.choice(np.array(GAPS[:4]), len(bad)) + 1.0) / 2.0)
    assert safe.all(), "a state s_t is too close to a set's boundary for the float64 sign to be the binary32 decision"
    return dict(ring_x=ring_x, ring_y=ring_y, events=events, ev_len=ev_len, hit=hit, clf=clf, inside=inside)


def covered_by(tr, cover_mask):
    cov = np.zeros(tr["inside"].shape[1], bool)
    for k in range(1, N_OPTIONS + 1):
        if (cover_mask >> k) & 1:
            cov |= tr["inside"][k]
    return cov


def frontier_rows(tr, target_mask, cover_mask, L):
    """Rows each node would gain (sum of v over its hits): for sizing `cap` in the capacity cases."""
    ring_len = tr["ring_x"].shape[0]
    el = tr["ev_len"].astype(np.int64)
    v = np.minimum(np.minimum(L, el), ring_len)
    ok = (el >= 1) & ~covered_by(tr, cover_mask)
    return [int(v[ok & (((tr["events"] >> p) & 1) != 0)].sum()) if (target_mask >> p) & 1 else 0 for p in range(N_OPTIONS + 1)]


# masks of §13: (target_mask, cover_mask) — cover 0 / one set / every set; a target option must be covered
MASKS = ((0b000001, 0), (0b001001, 0b001000), (0b111111, 0b111110), (0b000101, 0b111110), (0, 0b000110), (0b100000, 0b100000))


# ---------------------------------------------------------------------------------------------------- the case lists
GUARD = 64                                            # sentinel rows in front of and behind every buffer
CAPMODES = ("roomy", "cap1", "exact", "oneless", "midenv", "full", "append", "cap0", "neg")


def cap_and_count0(capmode, v):
    """(cap, count_0) of a capacity case from the rows per env `v` (env order)."""
    T = int(v.sum())
    if capmode == "roomy":
        return T + 7, 0
    if capmode == "cap1":
        return 1, 0
    if capmode == "exact":                            # cap = exactly count_0 + sum v
        return 3 + T, 3
    if capmode == "oneless":
        return max(3 + T - 1, 1), 3
    if capmode == "midenv":                           # cap cuts one env's rows in the middle
        first = np.cumsum(v) - v
        big = np.nonzero(v >= 2)[0]
        if len(big) == 0:
            return max(2 + T // 2, 1), 2
        e = big[len(big) // 2]
        return 2 + int(first[e]) + int(v[e]) // 2, 2
    if capmode == "full":                             # count_0 = cap: nothing may be written
        return 37, 37
    if capmode == "append":
        return 11 + T + 5, 11
    if capmode == "cap0":
        return 0, 5
    if capmode == "neg":                              # a negative fill level: rows at negative positions are dropped
        return T + 7, -3
    raise KeyError(capmode)


def _case(kind, n, ring_len, density, evf, lpn, capmode="roomy", prev="none", bits=1, masks=None, nodes="mixed"):
    c = dict(kind=kind, n=n, ring_len=ring_len, family=(density, evf), l_pos=lpn[0], l_neg=lpn[1], capmode=capmode, prev=prev,
             bits=bits, masks=masks, nodes=nodes)
    c["id"] = (f"{kind}-n{n}-H{ring_len}-{density}-{evf}-L{lpn[0]}+{lpn[1]}-{capmode}"
               + (f"-prev_{prev}" if prev != "none" else "") + (f"-bits{bits}" if bits != 1 else "")
               + (f"-t{masks[0]:06b}c{masks[1]:06b}-{nodes}" if masks else ""))
    return c


def _ring_for(n, i):
    """ring_len of the density sweep: small where n is large (the ring is n * ring_len floats twice)."""
    return (2, 64, 1, 256)[i % 4] if n <= 4097 else (2, 1, 64)[i % 3] if n < 262144 else (2, 1)[i % 2]


def collect_cases(sizes=SIZES):
    """SPEC §7 cases. Pruned to what the kernels' code paths distinguish (see tests/test_gpu_collect_edges.py's docstring):
    A  every hit density x every size n (row / wave / lane structure), ev_len mixed, (l_pos, l_neg), ring_len, event bits and
       prev_in rotating;
    B  every (l_pos, l_neg) x every ring_len x every ev_len family at n = 257 (v, the wrap and the gather loop depend on the env
       alone, not on n), and (l_pos, l_neg) x ring_len with ev_len mixed at n = 4097;
    C  every capacity mode at n = 65, 257, 4097, 65537 (the bound is per row, the level a prefix over rows);
    D  prev_in with all four (in, prev) combinations at n = 63, 257, 4097, 70000 and 262144."""
    out = []
    for a, n in enumerate(sizes):
        for b, d in enumerate(DENSITIES):
            i = a + b
            lpn = LPN[i % len(LPN)] if n <= 4097 else ((0, 5), (5, 0), (1, 0), (0, 1), (33, 32))[i % 5]
            if n > 65537 and d in ("all", "rand50", "rand99", "altwaves"):
                lpn = ((0, 5), (5, 0), (1, 0))[i % 3]                                   # (keeps sum v near a million rows)
            out.append(_case("A", n, _ring_for(n, i), d, "mixed", lpn, prev=("none", "random", "zeros")[i % 3],
                             bits=(1, 0b10, 0b100100, 0b111111)[i % 4]))
    for n in (257, 4097):
        if n not in sizes:
            continue
        for lpn in LPN:
            for H in RING_LENS:
                for evf in (EVLENS if n == 257 else ("mixed",)):
                    out.append(_case("B", n, H, "rand50", evf, lpn))
    for n in (65, 257, 4097, 65537):
        if n not in sizes:
            continue
        for j, cm in enumerate(CAPMODES):
            out.append(_case("C", n, 64 if n < 65537 else 2, ("rand50", "all", "rand99")[j % 3], "mixed",
                             ((5, 3), (33, 32), (2, 0))[j % 3] if n < 65537 else (2, 1), capmode=cm))
    for n in (63, 257, 4097, 70000, 262144):
        if n in sizes:
            out.append(_case("D", n, 2, "rand50", "mixed", (3, 2), prev="random", bits=0b110))
    return out


def frontier_cases(sizes=SIZES):
    """SPEC §13 cases, n_options = 5:
    A  every hit density x every size up to 4097 and a third of the densities at each larger size (every density at one of them
       at least), masks (cover 0 / one set / every set; all six nodes, two, one, none targeted) and the nodes per env (1, 2,
       all 6, mixed) rotating;
    B  every (l_pos, l_neg) x every ring_len at n = 257 with ev_len mixed, and every ev_len family at ring_len 2 and 64;
    C  every capacity mode (cap0 aside: cap < 1 is refused) at n = 257 and 4097, all six nodes targeted, each node with its
       own count_0 under the shared cap."""
    out = []
    for a, n in enumerate(sizes):
        for b, d in enumerate(DENSITIES):
            i = a + b
            if n >= 65536 and b % 3 != a % 3:                                           # (a third of the densities per large size)
                continue
            H = (2, 64, 1, 256)[i % 4] if n <= 4097 else (2, 1, 16)[i % 3]
            lpn = LPN[i % len(LPN)] if n <= 4097 else ((0, 5), (5, 0), (1, 0), (0, 1))[i % 4]
            out.append(_case("FA", n, H, d, "mixed", lpn, masks=MASKS[i % len(MASKS)], nodes=("mixed", "one", "two", "all")[i % 4]))
    if 257 in sizes:
        for lpn in LPN:
            for H in RING_LENS:
                out.append(_case("FB", 257, H, "rand50", "mixed", lpn, masks=MASKS[2]))
        for evf in EVLENS:
            for H in (2, 64):
                out.append(_case("FB", 257, H, "rand99", evf, (3, 4), masks=MASKS[2], nodes="two"))
    for n in (257, 4097):
        if n in sizes:
            for cm in CAPMODES:
                if cm != "cap0":
                    out.append(_case("FC", n, 64, "rand50", "mixed", (5, 3), capmode=cm, masks=MASKS[2]))
    return out


# (n, ring_len, l_pos, l_neg, selection): n_sel * L one below / at / above a multiple of 256, unsorted, duplicates, 1, 0
HARVEST_CASES = (
    (257, 64, 3, 2, "unsorted51"),        # 51 * 5 = 255
    (257, 64, 2, 2, "unsorted64"),        # 64 * 4 = 256
    (257, 64, 1, 0, "dups257"),           # 257 * 1 = 257, duplicates
    (4097, 2, 100, 100, "dups9"),         # L > ring_len: 255-labels
    (65, 1, 1, 255, "one"),               # n_sel = 1, ring_len = 1
    (1, 256, 33, 32, "one"),
    (70000, 2, 0, 5, "unsorted300"),
    (262144, 2, 5, 0, "unsorted300"),
    (256, 256, 32, 32, "none"),           # n_sel = 0: the output keeps its sentinels
)


def harvest_selection(n, mode, rng):
    if mode == "none":
        return np.zeros(0, np.int32)
    if mode == "one":
        return np.array([n - 1], np.int32)
    k = int(mode.lstrip("unsorteddups"))
    if mode.startswith("dups"):
        return rng.integers(0, n, k).astype(np.int32)[rng.integers(0, k, k)]
    sel = rng.permutation(n)[:k] if n >= k else rng.integers(0, n, k)
    return np.concatenate([sel[:-2], [n - 1, 0]]).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- one case, set up
def setup_collect(case, rng):
    """Trace, initial buffers (GUARD rows of sentinels behind cap), prev_in and the model's answer for a §7 case."""
    import collect_model as cm
    tr = build_trace(case["n"], case["ring_len"], case["family"], rng, bits=case["bits"])
    n, L = case["n"], case["l_pos"] + case["l_neg"]
    prev0 = {"none": None, "zeros": np.zeros(n, np.uint8), "random": prev_in_random(tr, case["bits"], rng)}[case["prev"]]
    _, v = cm.rows_per_env(tr["events"], tr["ev_len"], case["bits"], prev0, L, case["ring_len"])
    cap, c0 = cap_and_count0(case["capmode"], v)
    total_rows_ok(c0, v.sum())
    xy0, lab0, cnt0 = cm.fresh_buffers(cap, GUARD, c0, rng=rng)
    want = (xy0.copy(), lab0.copy(), cnt0.copy(), None if prev0 is None else prev0.copy())
    cm.collect(tr["ring_x"], tr["ring_y"], tr["events"], tr["ev_len"], case["bits"], want[3], case["l_pos"], case["l_neg"],
               want[0], want[1], want[2], cap=cap)
    return tr, cap, (xy0, lab0, cnt0, prev0), want


def setup_frontier(case, rng):
    """The same for a §13 case: buffers [6, cap] flat with GUARD rows behind the last node, each node its own count_0."""
    import collect_model as cm
    import frontier_model as fm
    tr = build_frontier_trace(case["n"], case["ring_len"], case["family"], rng, nodes=case["nodes"])
    target, cover = case["masks"]
    L, n_vf = case["l_pos"] + case["l_neg"], N_OPTIONS + 1
    rows = np.array(frontier_rows(tr, target, cover, L))
    cap, c0 = cap_and_count0(case["capmode"], rows[[int(np.argmax(rows))]])            # sized on the fullest node ...
    cap = max(cap, 1)
    cnt0 = np.array([min(max(c0 + p, -3) if case["capmode"] != "full" else cap - (p % 2), cap) for p in range(n_vf)], np.int32)
    cnt0[int(np.argmax(rows))] = c0                                                    # ... the others start near it
    total_rows_ok(cnt0, rows.max())
    xy0, lab0, _ = cm.fresh_buffers(cap, 0, cnt0, n_nodes=n_vf, rng=rng)
    want = (xy0.copy(), lab0.copy(), cnt0.copy())
    fm.collect_frontier(tr["ring_x"], tr["ring_y"], tr["events"], tr["ev_len"], target, cover, tr["clf"], case["l_pos"],
                        case["l_neg"], want[0], want[1], want[2], covered=covered_by(tr, cover))
    return tr, cap, (xy0, lab0, cnt0), want
