"""scg_row_values_cross (SPEC §29.1) on every block build: v, a and vs, bit for bit, against ScgContext.q_values per table and
tests/double_model.py's selection, at the slab's and the unit's edges (n = 1 .. 777 rows, three tables) and under
tests/test_gpu_row_values.py's table patterns, with W_val an independent table; with W_val = W_sel scg_row_values itself; the given
mode against q_values[act], act in {5, 255} and NaN states under rows without a table included; a = NULL and vs = NULL; fewer
workgroups than slabs; the write set behind guard bands, the inputs kept; the refusals in their sequence."""
import ctypes as C

import numpy as np
import pytest
import torch

import double_model as DM
import lambda_model as LM
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd import _lib
from skill_chaining_with_graphs_amd.core import ScgContext
from bits import assert_bits_equal
from gpu_util import block_envs, dev  # noqa: F401  (block_envs: the indirect fixture)
from util import HP, random_states, random_weights

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 9, 255, 256, 257, 777)
N_TAB, NONE = 3, LM.ROW_NONE
GUARD, FILL_V, FILL_A = 4099, -12345.5, 0x5A
GIVEN = _lib.CROSS_GIVEN
_rigs = {}


def rig(block):
    """One context (three value functions) and two independent sets of tables per block build."""
    if block not in _rigs:
        m = scg.load_map("pinball_simple")
        ctx = ScgContext(1024, N_TAB - 1, m, device=0, block_envs=block, **HP)
        Ws, Wv = random_weights(N_TAB, 31, std=0.05), random_weights(N_TAB, 32, std=0.05)
        _rigs[block] = (ctx, m, Ws, Wv, dev(Ws), dev(Wv))
    return _rigs[block]


def patterns(n, seed):
    """tests/test_gpu_row_values.py's: name -> (tab [n], the rows whose state is NaN)."""
    rng = np.random.default_rng(seed)
    none = np.zeros(n, bool)
    mixed = rng.choice(N_TAB, n, p=[0.5, 0.3, 0.2]).astype(np.uint8)
    holes = mixed.copy()
    holes[rng.random(n) < 0.3] = NONE
    edge = mixed.copy()
    edge[rng.random(n) < 0.25] = N_TAB
    edge[rng.random(n) < 0.25] = 254
    return {"one table": (np.full(n, 1, np.uint8), none),
            "a table without a row": (np.where(mixed == 1, 2, mixed).astype(np.uint8), none),
            "mixed lists": (mixed, none),
            "every row NONE": (np.full(n, NONE, np.uint8), ~none),
            "NaN states under NONE": (holes, holes == NONE),
            "tab = n_tab and 254": (edge, edge >= N_TAB)}


def given_actions(n, seed):
    """act [n]: mostly 0 .. 4, some 5 and 255 (rows the given mode treats as rows without a table)."""
    return np.random.default_rng(seed).choice([0, 1, 2, 3, 4, 5, 255], n, p=[0.16] * 5 + [0.1, 0.1]).astype(np.uint8)


def raw(ctx, n, s, tab, W_sel, W_val, n_tab, act, flags, v, a, vs):
    q = lambda t: C.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    rc = ctx.lib.scg_row_values_cross(ctx._ctx, C.c_int64(n), q(s[0]), q(s[1]), q(s[2]), q(s[3]), q(tab), q(W_sel), q(W_val), n_tab, q(act),
                                      C.c_uint32(flags), q(v), q(a), q(vs), ctx._stream())
    torch.cuda.synchronize()
    return rc


def same32(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("block_envs", [64, 128, 256], indirect=True)
@pytest.mark.parametrize("n", SIZES)
def test_cross_and_given_values_equal_the_model_by_bits(block_envs, n):
    ctx, m, Ws, Wv, Wsd, Wvd = rig(block_envs)
    q_values = lambda st, Wk: ctx.q_values([dev(v) for v in st], dev(Wk).view(-1)).cpu().numpy()
    differ = 0
    for name, (tab, nan) in patterns(n, 1000 + n).items():
        states = [v.copy() for v in random_states(m, n, 5 + n, vmax=1.5)]
        act = given_actions(n, 2000 + n)
        # the given mode's rows without a table: tab names none, or act >= 5 — NaN states under all of them
        nan_g = nan | (act >= 5)
        for given in (False, True):
            st = [v.copy() for v in states]
            for v in st:
                v[nan_g if given else nan] = np.nan
            sd, td, ad = [dev(v) for v in st], dev(tab), dev(act)
            if given:
                want_v, want_a, _ = DM.row_values_cross(q_values, st, tab, None, Wv, act=act)
                v = ctx.row_action_values(sd, td, Wvd, ad)
                torch.cuda.synchronize()
                assert_bits_equal(v.cpu().numpy(), want_v, allow_nan=False, msg=f"n {n}, {name}, given: v:")
                a = torch.full((n,), FILL_A, dtype=torch.uint8, device="cuda:0")                 # the given mode writes a = act too
                assert raw(ctx, n, sd, td, None, Wvd, N_TAB, ad, GIVEN, v, a, None) == 0          # (W_sel = NULL is accepted)
                assert np.array_equal(a.cpu().numpy(), want_a), (n, name)
                listed = (tab < N_TAB) & (act < 5)
                assert np.array_equal(want_a[listed], act[listed]) and np.all(want_a[~listed] == 255)
            else:
                want_v, want_a, want_vs = DM.row_values_cross(q_values, st, tab, Ws, Wv)
                v, a, vs = ctx.row_values_cross(sd, td, Wsd, Wvd, sel_values=True)
                v_only, none_a, none_vs = ctx.row_values_cross(sd, td, Wsd, Wvd, actions=False)      # a = NULL and vs = NULL
                torch.cuda.synchronize()
                assert_bits_equal(v.cpu().numpy(), want_v, allow_nan=False, msg=f"n {n}, {name}: v:")
                assert_bits_equal(vs.cpu().numpy(), want_vs, allow_nan=False, msg=f"n {n}, {name}: vs:")
                assert np.array_equal(a.cpu().numpy(), want_a), (n, name)
                assert none_a is None and none_vs is None and same32(v_only, v), (n, name)
                # SPEC §29.1's identity: one table on both sides is scg_row_values, and vs = v
                v1, a1, vs1 = ctx.row_values_cross(sd, td, Wsd, Wsd.clone(), sel_values=True)
                rv, ra = ctx.row_values(sd, td, Wsd)
                torch.cuda.synchronize()
                assert same32(v1, rv) and torch.equal(a1, ra) and same32(vs1, v1), (n, name)
                assert same32(vs, rv) and torch.equal(a, ra), (n, name)          # whatever W_val holds: vs and a are the selecting table's
                _, a_val = ctx.row_values(sd, td, Wvd)
                differ += int(((a != a_val) & (a < 5)).sum())
                if name == "mixed lists" and n >= 255:
                    assert sum((tab == k).sum() % 8 != 0 for k in range(N_TAB)) >= 2, "the seeded lists must end in partial units"
            for got, host in zip(sd + [td, ad], st + [tab, act]):                # the inputs are kept
                assert np.array_equal(got.cpu().numpy().view(np.uint8), host.view(np.uint8)), (n, name)
    # the seeded tables' argmax must differ on some rows, or the W_val = W_sel identity would be the whole test
    # (two independent random tables agree on a row's argmax about one time in five; every pattern but one lists rows)
    if n >= 7:
        assert differ >= n // 4, (n, differ)


@pytest.mark.parametrize("blocks", [1, 3])
def test_the_launch_geometry_changes_no_bit(monkeypatch, blocks):
    """SCG_ROW_VALUES_CROSS_BLOCKS: 777 rows are four slabs; one workgroup walks all of them, three walk two, one and one."""
    ctx, m, Ws, Wv, Wsd, Wvd = rig(256)
    n = 777
    tab = patterns(n, 1000 + n)["NaN states under NONE"][0]
    sd, td, ad = [dev(v) for v in random_states(m, n, 5 + n, vmax=1.5)], dev(tab), dev(given_actions(n, 3))
    v0, a0, vs0 = ctx.row_values_cross(sd, td, Wsd, Wvd, sel_values=True)
    g0 = ctx.row_action_values(sd, td, Wvd, ad)
    monkeypatch.setenv("SCG_ROW_VALUES_CROSS_BLOCKS", str(blocks))
    v1, a1, vs1 = ctx.row_values_cross(sd, td, Wsd, Wvd, sel_values=True)
    g1 = ctx.row_action_values(sd, td, Wvd, ad)
    torch.cuda.synchronize()
    assert same32(v1, v0) and torch.equal(a1, a0) and same32(vs1, vs0) and same32(g1, g0)
    assert (a0 == 255).any() and (a0 < 5).sum() > 400 and not same32(v0, vs0) and int((g0 != 0).sum()) > 300


@pytest.mark.parametrize("n", [1, 257, 777])
def test_writes_n_entries_of_v_a_and_vs_only(n):
    ctx, m, Ws, Wv, Wsd, Wvd = rig(256)
    states = random_states(m, n, 9, vmax=1.5)
    tab = patterns(n, 77)["NaN states under NONE"][0]
    sd, td, ad = [dev(v) for v in states], dev(tab), dev(given_actions(n, 4))
    keep = [t.clone() for t in sd + [td, ad, Wsd, Wvd]]
    vb = torch.full((2 * GUARD + n,), FILL_V, dtype=torch.float32, device="cuda:0")
    sb = torch.full((2 * GUARD + n,), FILL_V, dtype=torch.float32, device="cuda:0")
    ab = torch.full((2 * GUARD + n,), FILL_A, dtype=torch.uint8, device="cuda:0")
    at = lambda t, size: t.data_ptr() + size * GUARD           # (4099 entries in: an odd offset, 4-byte aligned for the floats)
    outside = lambda h, fill: np.all(h[:GUARD] == fill) and np.all(h[GUARD + n:] == fill)
    assert raw(ctx, n, sd, td, Wsd, Wvd, N_TAB, None, 0, at(vb, 4), at(ab, 1), at(sb, 4)) == 0
    want_v, want_a, want_vs = (t.cpu().numpy() for t in ctx.row_values_cross(sd, td, Wsd, Wvd, sel_values=True))
    hv, ha, hs = vb.cpu().numpy(), ab.cpu().numpy(), sb.cpu().numpy()
    assert outside(hv, FILL_V) and outside(hs, FILL_V) and outside(ha, FILL_A)
    assert_bits_equal(hv[GUARD: GUARD + n], want_v, allow_nan=False, msg=f"n {n}: v at an odd offset:")
    assert_bits_equal(hs[GUARD: GUARD + n], want_vs, allow_nan=False, msg=f"n {n}: vs at an odd offset:")
    assert np.array_equal(ha[GUARD: GUARD + n], want_a)
    ab.fill_(FILL_A), sb.fill_(FILL_V)                          # a = NULL, vs = NULL: neither is written
    assert raw(ctx, n, sd, td, Wsd, Wvd, N_TAB, None, 0, at(vb, 4), None, None) == 0 and torch.all(ab == FILL_A) and torch.all(sb == FILL_V)
    vb.fill_(FILL_V)                                            # the given mode: v and a behind the same bands
    assert raw(ctx, n, sd, td, None, Wvd, N_TAB, ad, GIVEN, at(vb, 4), at(ab, 1), None) == 0
    want_g = ctx.row_action_values(sd, td, Wvd, ad).cpu().numpy()
    hv, ha = vb.cpu().numpy(), ab.cpu().numpy()
    assert outside(hv, FILL_V) and outside(ha, FILL_A) and torch.all(sb == FILL_V)
    assert_bits_equal(hv[GUARD: GUARD + n], want_g, allow_nan=False, msg=f"n {n}: given v at an odd offset:")
    for got, was in zip(sd + [td, ad, Wsd, Wvd], keep):          # the inputs are kept
        assert torch.equal(got.view(torch.uint8), was.view(torch.uint8))


def test_refusals_in_their_sequence_write_nothing():
    ctx, m, Ws, Wv, Wsd, Wvd = rig(256)
    n = 100
    sd, td, ad = [dev(v) for v in random_states(m, n, 9)], dev(np.zeros(n, np.uint8)), dev(np.zeros(n, np.uint8))
    v = torch.full((n,), FILL_V, dtype=torch.float32, device="cuda:0")
    vs = torch.full((n,), FILL_V, dtype=torch.float32, device="cuda:0")
    a = torch.full((n,), FILL_A, dtype=torch.uint8, device="cuda:0")
    base = dict(n=n, x=sd[0], y=sd[1], vx=sd[2], vy=sd[3], tab=td, W_sel=Wsd, W_val=Wvd, n_tab=N_TAB, act=None, flags=0, v=v, vs=vs)
    given = dict(act=ad, flags=GIVEN, vs=None, W_sel=None)
    cases = [("n must be", dict(n=-1)), ("n must be", dict(n=-1, x=None, n_tab=0, flags=6))]
    cases += [("null array", {f: None}) for f in ("x", "y", "vx", "vy", "tab", "W_sel", "W_val", "v")]
    cases += [("null array", dict(given, **{f: None})) for f in ("x", "tab", "W_val", "v")]
    cases += [("null array", dict(v=None, n_tab=0)), ("null array", dict(W_val=None, flags=2)), ("null array", dict(given, v=None, act=None))]
    cases += [("n_tab out of range", dict(n_tab=k)) for k in (0, -1, N_TAB + 1)]
    cases += [("n_tab out of range", dict(n=0, n_tab=0)), ("n_tab out of range", dict(n_tab=0, flags=2)), ("n_tab out of range", dict(given, n_tab=4, act=None))]
    cases += [("unknown flag bits", dict(flags=f)) for f in (2, 3, 0x80000000)] + [("unknown flag bits", dict(given, flags=3, act=None))]
    cases += [("needs act", dict(given, act=None)), ("needs act", dict(given, vs=vs)), ("needs act", dict(given, act=None, vs=vs))]
    for want, kw in cases:
        k = dict(base, **kw)
        rc = raw(ctx, k["n"], [k["x"], k["y"], k["vx"], k["vy"]], k["tab"], k["W_sel"], k["W_val"], k["n_tab"], k["act"], k["flags"], k["v"], a, k["vs"])
        assert rc == -1, (want, kw)
        err = ctx.lib.scg_last_error(ctx._ctx)
        assert b"scg_row_values_cross" in err and want.encode() in err, (want, kw, err)
        assert torch.all(v == FILL_V) and torch.all(a == FILL_A) and torch.all(vs == FILL_V)
    assert ctx.lib.scg_row_values_cross(None, C.c_int64(-1), None, None, None, None, None, None, None, 0, None, C.c_uint32(2), None, None,
                                        None, None) == -1
    assert b"null ctx" in ctx.lib.scg_last_error(None)
    assert raw(ctx, n, sd, td, Wsd, Wvd, N_TAB, ad, 0, v, a, vs) == 0                # act is not read with the flag clear; accepted
    v.fill_(FILL_V), a.fill_(FILL_A), vs.fill_(FILL_V)
    for act, flags, s in ((None, 0, vs), (ad, GIVEN, None)):                         # n = 0: nothing written
        assert raw(ctx, 0, sd, td, Wsd, Wvd, N_TAB, act, flags, v, a, s) == 0
        assert torch.all(v == FILL_V) and torch.all(a == FILL_A) and torch.all(vs == FILL_V)
    ve, ae, se = ctx.row_values_cross([t[:0] for t in sd], td[:0], Wsd, Wvd, sel_values=True)
    assert ve.numel() == ae.numel() == se.numel() == 0 and ctx.row_action_values([t[:0] for t in sd], td[:0], Wvd, ad[:0]).numel() == 0
    for bad in (dict(tab=td.int()), dict(tab=td[:5]), dict(W_sel=Wsd.view(-1)), dict(W_val=Wvd.double()), dict(W_val=torch.cat([Wvd, Wvd])),
                dict(W_val=Wvd[:2])):
        with pytest.raises(scg.ScgError):
            ctx.row_values_cross(sd, bad.get("tab", td), bad.get("W_sel", Wsd), bad.get("W_val", Wvd))
    for W_sel, W_val in ((Wsd, None), (None, Wvd), (None, None)):                    # a missing table is refused in Python, by name
        with pytest.raises(scg.ScgError):
            ctx.row_values_cross(sd, td, W_sel, W_val)
    for bad in (dict(act=ad.int()), dict(act=ad[:5]), dict(act=None), dict(W=Wvd.view(-1)), dict(W=None)):
        with pytest.raises(scg.ScgError):
            ctx.row_action_values(sd, td, bad.get("W", Wvd), bad.get("act", ad))
