"""scg_row_values (SPEC §27.1) on every block build: v and a, bit for bit, against ScgContext.q_values per table followed by
valuefit.greedy_max (tests/lambda_model.py's row_values), at the slab's and the unit's edges (n = 1 .. 777 rows, three tables) and
under every table pattern — one table, a table without a row, list lengths off the unit's 8, no table at all, NaN states under
rows without a table, tab = n_tab and 254 —; a = NULL; fewer workgroups than slabs; the write set behind guard bands, the inputs kept; the refusals in their
sequence."""
import ctypes as C

import numpy as np
import pytest
import torch

import lambda_model as LM
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd.core import ScgContext
from bits import assert_bits_equal
from gpu_util import block_envs, dev  # noqa: F401  (block_envs: the indirect fixture)
from util import HP, random_states, random_weights

pytestmark = pytest.mark.gpu

SIZES = (1, 7, 8, 9, 255, 256, 257, 777)
N_TAB, NONE = 3, LM.ROW_NONE
GUARD, FILL_V, FILL_A = 4099, -12345.5, 0x5A
_rigs = {}


def rig(block):
    """One context (three value functions), tables and 777 seeded states per block build."""
    if block not in _rigs:
        m = scg.load_map("pinball_simple")
        ctx = ScgContext(1024, N_TAB - 1, m, device=0, block_envs=block, **HP)
        W = random_weights(N_TAB, 31, std=0.05)
        _rigs[block] = (ctx, m, W, dev(W))
    return _rigs[block]


def patterns(n, seed):
    """name -> (tab [n], the rows whose state is NaN)."""
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


def raw(ctx, n, s, tab, W, n_tab, v, a):
    q = lambda t: C.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    rc = ctx.lib.scg_row_values(ctx._ctx, C.c_int64(n), q(s[0]), q(s[1]), q(s[2]), q(s[3]), q(tab), q(W), n_tab, q(v), q(a), ctx._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("block_envs", [64, 128, 256], indirect=True)
@pytest.mark.parametrize("n", SIZES)
def test_values_equal_q_values_and_greedy_max_by_bits(block_envs, n):
    ctx, m, W, Wd = rig(block_envs)
    q_values = lambda st, Wk: ctx.q_values([dev(v) for v in st], dev(Wk).view(-1)).cpu().numpy()
    for name, (tab, nan) in patterns(n, 1000 + n).items():
        states = [v.copy() for v in random_states(m, n, 5 + n, vmax=1.5)]
        for v in states:
            v[nan] = np.nan
        want_v, want_a = LM.row_values(q_values, states, tab, W)
        sd, td = [dev(v) for v in states], dev(tab)
        v, a = ctx.row_values(sd, td, Wd)
        v_only, none = ctx.row_values(sd, td, Wd, actions=False)                 # a = NULL
        torch.cuda.synchronize()
        assert_bits_equal(v.cpu().numpy(), want_v, allow_nan=False, msg=f"n {n}, {name}: v:")
        assert np.array_equal(a.cpu().numpy(), want_a), (n, name)
        assert none is None and torch.equal(v_only.view(torch.int32), v.view(torch.int32)), (n, name)
        if name == "mixed lists" and n >= 255:
            assert sum((tab == k).sum() % 8 != 0 for k in range(N_TAB)) >= 2, "the seeded lists must end in partial units"
        for got, host in zip(sd + [td], states + [tab]):                         # the inputs are kept
            assert np.array_equal(got.cpu().numpy().view(np.uint8), host.view(np.uint8)), (n, name)
    assert (want_a == 255).any() and not want_v[want_a == 255].any() and not np.signbit(want_v[want_a == 255]).any()


@pytest.mark.parametrize("blocks", [1, 3])
def test_the_launch_geometry_changes_no_bit(monkeypatch, blocks):
    """SCG_ROW_VALUES_BLOCKS: 777 rows are four slabs; one workgroup walks all of them, three walk two, one and one."""
    ctx, m, W, Wd = rig(256)
    n = 777
    tab = patterns(n, 1000 + n)["NaN states under NONE"][0]
    sd, td = [dev(v) for v in random_states(m, n, 5 + n, vmax=1.5)], dev(tab)
    v0, a0 = ctx.row_values(sd, td, Wd)
    monkeypatch.setenv("SCG_ROW_VALUES_BLOCKS", str(blocks))
    v1, a1 = ctx.row_values(sd, td, Wd)
    torch.cuda.synchronize()
    assert torch.equal(v1.view(torch.int32), v0.view(torch.int32)) and torch.equal(a1, a0)
    assert (a0 == 255).any() and (a0 < 5).sum() > 400


@pytest.mark.parametrize("n", [1, 257, 777])
def test_writes_n_entries_of_v_and_a_only(n):
    ctx, m, W, Wd = rig(256)
    states = random_states(m, n, 9, vmax=1.5)
    tab = patterns(n, 77)["NaN states under NONE"][0]
    sd, td = [dev(v) for v in states], dev(tab)
    vb = torch.full((2 * GUARD + n,), FILL_V, dtype=torch.float32, device="cuda:0")
    ab = torch.full((2 * GUARD + n,), FILL_A, dtype=torch.uint8, device="cuda:0")
    assert raw(ctx, n, sd, td, Wd, N_TAB, vb.data_ptr() + 4 * GUARD, ab.data_ptr() + GUARD) == 0
    want_v, want_a = (t.cpu().numpy() for t in ctx.row_values(sd, td, Wd))
    hv, ha = vb.cpu().numpy(), ab.cpu().numpy()
    assert np.all(hv[:GUARD] == FILL_V) and np.all(hv[GUARD + n:] == FILL_V) and np.all(ha[:GUARD] == FILL_A) and np.all(ha[GUARD + n:] == FILL_A)
    assert_bits_equal(hv[GUARD: GUARD + n], want_v, allow_nan=False, msg=f"n {n}: v at an odd address:")
    assert np.array_equal(ha[GUARD: GUARD + n], want_a)
    ab.fill_(FILL_A)                                                             # a = NULL: a is not written
    assert raw(ctx, n, sd, td, Wd, N_TAB, vb.data_ptr() + 4 * GUARD, None) == 0 and torch.all(ab == FILL_A)


def test_refusals_in_their_sequence_write_nothing():
    ctx, m, W, Wd = rig(256)
    n = 100
    sd, td = [dev(v) for v in random_states(m, n, 9)], dev(np.zeros(n, np.uint8))
    v = torch.full((n,), FILL_V, dtype=torch.float32, device="cuda:0")
    a = torch.full((n,), FILL_A, dtype=torch.uint8, device="cuda:0")
    base = dict(n=n, x=sd[0], y=sd[1], vx=sd[2], vy=sd[3], tab=td, W=Wd, n_tab=N_TAB, v=v)
    cases = [("n must be", dict(n=-1)), ("n must be", dict(n=-1, x=None, n_tab=0))]
    cases += [("null array", {f: None}) for f in ("x", "y", "vx", "vy", "tab", "W", "v")] + [("null array", dict(v=None, n_tab=0))]
    cases += [("n_tab out of range", dict(n_tab=k)) for k in (0, -1, N_TAB + 1)] + [("n_tab out of range", dict(n=0, n_tab=0))]
    for want, kw in cases:
        k = dict(base, **kw)
        assert raw(ctx, k["n"], [k["x"], k["y"], k["vx"], k["vy"]], k["tab"], k["W"], k["n_tab"], k["v"], a) == -1, (want, kw)
        err = ctx.lib.scg_last_error(ctx._ctx)
        assert b"scg_row_values" in err and want.encode() in err, (want, kw, err)
        assert torch.all(v == FILL_V) and torch.all(a == FILL_A)
    assert ctx.lib.scg_row_values(None, C.c_int64(-1), None, None, None, None, None, None, 0, None, None, None) == -1
    assert b"null ctx" in ctx.lib.scg_last_error(None)
    assert raw(ctx, 0, sd, td, Wd, N_TAB, v, a) == 0 and torch.all(v == FILL_V) and torch.all(a == FILL_A)      # n = 0: nothing written
    ve, ae = ctx.row_values([t[:0] for t in sd], td[:0], Wd)
    assert ve.numel() == ae.numel() == 0
    for bad in (dict(tab=td.int()), dict(tab=td[:5]), dict(W=Wd.view(-1)), dict(W=Wd.double()), dict(W=torch.cat([Wd, Wd]))):
        with pytest.raises(scg.ScgError):
            ctx.row_values(sd, bad.get("tab", td), bad.get("W", Wd))
