"""scg_trace_returns (SPEC §28.1) against tests/trace_model.py, bit for bit, on tests/test_gpu_lambda_returns.py's shape of record (70
envs whose lengths sit on the scan's chunk edges, edge rows planted, every fifth env a cut record) with SPEC §28.3's action / greedy
action pattern; the three identities against ScgContext.lambda_returns on the device's own output; h = NULL; offsets that leave the
arrays or decrease, behind guard bands; the refusal sequence; valuefit.trace_targets and fit_values_to_returns(trace=...) on the small
agent of test_gpu_lambda_returns.py — the premise (a greedy record cuts nowhere) and the end-to-end fit — and the report tool at toy
size."""
import ctypes as C

import numpy as np
import pytest
import torch

import lambda_model as LM
import trace_model as TM
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd import ScgError
from skill_chaining_with_graphs_amd.core import ScgContext
from skill_chaining_with_graphs_amd.valuefit import trace_targets
from gpu_util import dev
from util import HP
from test_gpu_lambda_returns import FILL, GAMMA, GUARD, N_ENV, same_bits, small_agent, synthetic  # noqa: F401 (small_agent: a fixture)

pytestmark = pytest.mark.gpu

FIELDS = ("reward", "done", "vf", "term", "action", "ag", "v0", "vk")
LAM_VF = (0.9, 0.3, 1.0)


def traced(seed, all_done):
    flat = synthetic(seed, all_done)
    flat["action"], flat["ag"] = TM.synthetic_actions(np.random.default_rng(seed + 1000), flat)
    return flat


@pytest.fixture(scope="module")
def ctx():
    c = ScgContext(64, 2, scg.load_map("pinball_simple"), device=0, block_envs=256, **HP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def records():
    return {"cut": traced(41, False), "done": traced(42, True)}


def device_scan(ctx, flat, lam, R, cut, horizon=True, **over):
    f = dict(flat, **over)
    out = ctx.trace_returns(dev(f["offsets"]), *[dev(f[k]) for k in FIELDS], GAMMA, lam, R, cut=cut, horizon=horizon)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def model(flat, lam, R, cut, offsets=None, total=None, **over):
    f = dict(flat, **over)
    total = len(f["reward"]) if total is None else total
    return TM.trace_returns(f["offsets"] if offsets is None else offsets, total, *[f[k][:total] for k in FIELDS], GAMMA,
                            np.atleast_1d(lam), TM.TRACE_CUT if cut else 0, R)


def assert_bits(got, want, what):
    for name, g, w in zip(("y0", "yk", "h"), got, want):
        bad = np.nonzero(g.view(np.uint64) != w.view(np.uint64))[0]
        assert len(bad) == 0, f"{what} {name}: {len(bad)} of {len(g)} rows differ, first row {bad[0]}: {g[bad[0]]!r} != {w[bad[0]]!r}"


@pytest.mark.parametrize("R", [0.0, 100.0])
@pytest.mark.parametrize("lam", [0.0, 0.9, 1.0, LAM_VF], ids=["0", "0.9", "1", "per_vf"])
@pytest.mark.parametrize("cut", [False, True])
def test_device_scan_equals_the_model_by_bits(ctx, records, cut, lam, R):
    flat = records["cut"]
    inputs = [dev(flat[k]) for k in FIELDS]
    off = dev(flat["offsets"])
    got = ctx.trace_returns(off, *inputs, GAMMA, lam, R, cut=cut, horizon=True)
    torch.cuda.synchronize()
    want = model(flat, lam, R, cut)
    assert_bits([t.cpu().numpy() for t in got], want, f"cut={cut} lam={lam} R={R}")
    assert np.isfinite(want[0]).all() and np.any(want[1] != 0) and np.any((want[1] != want[0]) & (flat["vf"] >= 1))
    if cut and lam != 0.0:                                     # the cut is exercised: other targets than without it
        assert not same_bits(want[0], model(flat, lam, R, False)[0])
    for t, k in zip(inputs, FIELDS):                           # inputs unchanged by bits
        assert np.array_equal(t.cpu().numpy().view(np.uint8), flat[k].view(np.uint8)), k
    assert np.array_equal(off.cpu().numpy(), flat["offsets"])
    y0, yk, none = device_scan(ctx, flat, lam, R, cut, horizon=False)              # h = NULL: the same y0 / yk
    assert none is None and same_bits(y0, want[0]) and same_bits(yk, want[1])


@pytest.mark.parametrize("block_envs", [64, 128])
def test_the_other_block_builds_give_the_same_bits(records, block_envs):
    c = ScgContext(64, 2, scg.load_map("pinball_simple"), device=0, block_envs=block_envs, **HP)
    try:
        assert_bits(device_scan(c, records["cut"], LAM_VF, 100.0, True), model(records["cut"], LAM_VF, 100.0, True), f"block {block_envs}")
    finally:
        c.close()


def test_the_identities_on_the_device_output(ctx, records):
    R = 100.0
    for name in ("cut", "done"):
        flat = records[name]
        total = len(flat["reward"])
        lr_fields = [dev(flat[k]) for k in ("reward", "done", "vf", "term", "v0", "vk")]
        peng = lambda lam: [t.cpu().numpy() for t in ctx.lambda_returns(dev(flat["offsets"]), *lr_fields, GAMMA, lam, R)]
        L = np.diff(flat["offsets"])
        env = np.repeat(np.arange(N_ENV), L)
        step = (np.arange(total) - flat["offsets"][:-1][env]) >= 1
        everywhere = np.concatenate([flat["action"][1:], [255]]).astype(np.uint8)
        nowhere = ((np.concatenate([flat["action"][1:], [0]]) + 1) % 5).astype(np.uint8)
        zero = peng(0.0)
        for lam in (0.3, 0.9, 1.0):
            want = peng(lam)
            for lam_arg in (lam, [lam] * 3):                   # 1: no cut, one lambda
                y0, yk, _ = device_scan(ctx, flat, lam_arg, R, False)
                assert same_bits(y0, want[0]) and same_bits(yk, want[1]), (name, lam)
            y0, yk, h_all = device_scan(ctx, flat, lam, R, True, ag=everywhere)    # 2: a cut that never fires
            assert same_bits(y0, want[0]) and same_bits(yk, want[1]), (name, lam)
            for ag in (nowhere, np.full(total, 255, np.uint8)):                    # 3: a cut that always fires is lambda = 0
                y0, yk, h = device_scan(ctx, flat, lam, R, True, ag=ag)
                assert same_bits(y0, zero[0]) and same_bits(yk, zero[1]), (name, lam)
                assert np.all(h[step] == 1.0) and not h[~step].any()
            assert not same_bits(want[0], zero[0])
            if name == "done":                                 # 4: every env ends done: h is the geometric sum in Horner form
                horner = [1.0]
                for _ in range(int(L.max())):
                    horner.append(1.0 + lam * horner[-1])
                for e in range(N_ENV):
                    w = [0.0] + [horner[L[e] - 1 - j] for j in range(1, L[e])]
                    assert same_bits(h_all[flat["offsets"][e]: flat["offsets"][e + 1]], w[:L[e]]), (lam, e)


def raw(ctx, n_env, off, total, arrs, gamma, lam_vf, n_lam, flags, R, y0, yk, h):
    q = lambda t: C.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    lam = None if lam_vf is None else (C.c_double * len(lam_vf))(*lam_vf)
    rc = ctx.lib.scg_trace_returns(ctx._ctx, n_env, q(off), C.c_int64(total), *[q(t) for t in arrs], C.c_double(gamma), lam, n_lam,
                                   C.c_uint32(flags), C.c_double(R), q(y0), q(yk), q(h), ctx._stream())
    torch.cuda.synchronize()
    return rc


def test_offsets_that_leave_the_arrays_or_decrease_write_nothing_outside(ctx, records):
    """Every array the kernel indexes by row is `total` long and lies inside a longer allocation (the guard bands): the float
    inputs' bands hold NaN, done / vf / term's 1, action's and ag's 255 (a read outside would change a value), the outputs' a fill
    value that must stay."""
    flat = records["cut"]
    total = 300
    band = lambda v, fill: torch.cat([torch.full((GUARD,), fill, dtype=v.dtype, device=v.device), v,
                                      torch.full((GUARD,), fill, dtype=v.dtype, device=v.device)])
    fills = {"reward": float("nan"), "v0": float("nan"), "vk": float("nan"), "done": 1, "vf": 1, "term": 1, "action": 255, "ag": 255}
    bufs = [band(dev(flat[k][:total]), fills[k]) for k in FIELDS]
    ptrs = [b.data_ptr() + GUARD * b.element_size() for b in bufs]
    for off, exact in (([0, 40, 140, total + 7, total + 90], True),           # past the end: clamped
                       ([-5, 70, 2 ** 40], True),                              # in front of the start, far past the end
                       ([0, 130, 60, 60, 2 ** 62, -2 ** 62, 10], False),       # decreasing: empty envs and envs that overlap (which of two
                       ([total + 1, total + 1, 0], False)):                    # writers of a row wins is not defined: the bands only)
        off = np.array(off, np.int64)
        outs = [torch.full((2 * GUARD + total,), FILL, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        assert raw(ctx, len(off) - 1, dev(off), total, ptrs, GAMMA, LAM_VF, 3, TM.TRACE_CUT, 100.0,
                   *[t.data_ptr() + 8 * GUARD for t in outs]) == 0
        want = model(flat, LAM_VF, 100.0, True, offsets=off, total=total)
        for name, y, w in zip(("y0", "yk", "h"), outs, want):
            got = y.cpu().numpy()
            assert np.all(got[:GUARD] == FILL) and np.all(got[GUARD + total:] == FILL), (name, off)
            if exact:
                owned = np.zeros(total, bool)
                for e in range(len(off) - 1):
                    owned[min(max(off[e], 0), total): min(max(off[e + 1], 0), total)] = True
                assert same_bits(got[GUARD: GUARD + total][owned], w[owned]) and np.all(got[GUARD: GUARD + total][~owned] == FILL), (name, off)
                assert np.isfinite(w).all()


def test_the_refusal_sequence_writes_nothing(ctx, records):
    flat = records["done"]
    total = len(flat["reward"])
    off, arrs = dev(flat["offsets"]), [dev(flat[k]) for k in FIELDS]
    y0, yk, h = (torch.full((total,), FILL, dtype=torch.float64, device="cuda:0") for _ in range(3))
    nan = float("nan")
    base = dict(n_env=N_ENV, off=off, total=total, gamma=GAMMA, lam_vf=LAM_VF, n_lam=3, flags=1, y0=y0, yk=yk, h=h, **dict(zip(FIELDS, arrs)))
    cases = [("n_env must be", dict(n_env=-1, total=-1)), ("total must be", dict(total=-1, off=None)), ("total must be", dict(total=-1, n_lam=0))]
    cases += [("null array", {k: None}) for k in ("off", "y0", "yk", "lam_vf") + FIELDS] + [("null array", dict(y0=None, n_lam=0, gamma=nan))]
    cases += [("n_lam out of range", dict(n_lam=v, gamma=nan)) for v in (0, -1, 4)]
    cases += [("gamma must be", dict(gamma=v, flags=2)) for v in (-0.1, 1.5, nan)]
    cases += [("lam_vf must be", dict(lam_vf=v, flags=2)) for v in ((0.5, -1e-9, 0.5), (0.5, 0.5, 1.0000001), (nan, 0.5, 0.5))]
    cases += [("unknown flag", dict(flags=v)) for v in (2, 3, 0x80000000)]
    for want, kw in cases:
        k = dict(base, **kw)
        rc = raw(ctx, k["n_env"], k["off"], k["total"], [k[f] for f in FIELDS], k["gamma"], k["lam_vf"], k["n_lam"], k["flags"], 100.0,
                 k["y0"], k["yk"], k["h"])
        assert rc == -1, (want, kw)
        err = ctx.lib.scg_last_error(ctx._ctx)
        assert b"scg_trace_returns" in err and want.encode() in err, (want, kw, err)
        assert torch.all(y0 == FILL) and torch.all(yk == FILL) and torch.all(h == FILL)
    # only the first n_lam entries are looked at; n_env = 0 and total = 0 succeed and write nothing
    assert raw(ctx, 0, off, total, arrs, GAMMA, (0.5, 7.0), 1, 0, 0.0, y0, yk, h) == 0
    assert raw(ctx, N_ENV, off, 0, arrs, GAMMA, LAM_VF, 3, 1, 0.0, y0, yk, h) == 0
    assert torch.all(y0 == FILL) and torch.all(yk == FILL) and torch.all(h == FILL)
    for bad in (dict(lam=1.5), dict(lam=[0.5] * 4), dict(lam=[]), dict(lam=[0.5, nan])):
        with pytest.raises(ScgError, match="lam"):
            ctx.trace_returns(off, *arrs, GAMMA, bad["lam"], 0.0)
    with pytest.raises(ScgError):
        ctx.trace_returns(off.cpu(), *arrs, GAMMA, 0.5, 0.0)
    with pytest.raises(ScgError):
        ctx.trace_returns(off, *arrs[:4], arrs[4].to(torch.int32), *arrs[5:], GAMMA, 0.5, 0.0)
    st = dict(flat, offsets=np.array([0, 5, 3, total], np.int64), x=flat["reward"], y=flat["reward"], vx=flat["reward"], vy=flat["reward"])
    with pytest.raises(ScgError, match="offsets"):                                # trace_targets checks the offsets on the host
        trace_targets(ctx, st, dev(np.zeros((3, 5, 1296), np.float32)), GAMMA, 0.5, 0.0)


# ---------------------------------------------------------------------------------------------------- the agent

def test_a_greedy_record_cuts_nowhere_and_watkins_is_peng_on_it(small_agent):
    """The premise: in a record made at epsilon = 0 every recorded action is the greedy action of the table that acted (SPEC §4.3:
    the first maximum wins; §27.1: the lowest index), so the cut never fires and the two traces give the same fit by bits."""
    ag = small_agent[0]
    traj, _ = ag.record_episodes(n_episodes=64, epsilon=0.0, seed=9)
    flat = traj.to_numpy()
    c = ag.ctx.cfg
    lt = trace_targets(ag._eval_ctx[64][0], flat, ag.W, float(c.gamma), 0.9, float(c.r_option_success), cut=True)
    rows = np.nonzero(lt["sample"])[0]
    assert len(rows) > 500 and set(np.unique(flat["vf"][rows])) >= {0, 2}
    bad = rows[flat["action"][rows] != lt["ag"][rows - 1]]
    assert len(bad) == 0, (f"{len(bad)} of {len(rows)} step rows differ, first row {bad[0]}: vf {flat['vf'][bad[0]]} term {flat['term'][bad[0] - 1]} "
                           f"action {flat['action'][bad[0]]} greedy {lt['ag'][bad[0] - 1]}")
    assert not lt["cut"].any() and np.all(lt["c"][rows] == 0.9)
    _, W_peng = ag.fit_values_to_returns(trajectory=traj, epsilon=0.0, seed=9, lam=0.9)
    rep, W_wat = ag.fit_values_to_returns(trajectory=traj, epsilon=0.0, seed=9, lam=0.9, trace="watkins")
    assert torch.equal(W_wat.view(torch.int32), W_peng.view(torch.int32)) and not torch.equal(W_wat, ag.W)
    assert rep["trace"] == "watkins" and all(rep["vf"][k]["cut_share"] == 0.0 for k in (0, 2))


def test_watkins_fit_end_to_end_on_an_exploring_record(small_agent):
    ag, report, _ = small_agent
    traj = report["trajectory"]                                # 64 episodes at epsilon = 0.5
    W0 = ag.W.clone()
    kw = dict(trajectory=traj, epsilon=0.5, seed=9, sweeps=2, apply=False)
    rep_p, W_scalar = ag.fit_values_to_returns(lam=0.9, **kw)
    rep_s, W_peng = ag.fit_values_to_returns(lam=[0.9] * 3, **kw)                  # "peng" through trace_targets(cut=False)
    rep_w, W_wat = ag.fit_values_to_returns(lam=0.9, trace="watkins", keep=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(ag.W, W0)
    assert torch.equal(W_peng.view(torch.int32), W_scalar.view(torch.int32))       # identity 1 through the whole fit
    assert not torch.equal(W_wat, W_peng) and not torch.equal(W_wat, W0)
    assert rep_p["trace"] == "peng" and "cut_share" not in rep_p["vf"][0] and rep_s["lam"] == [0.9] * 3 and rep_w["lam"] == 0.9
    assert len(rep_w["sweeps"]) == 2
    for s in range(2):
        for k in (0, 2):
            w, p = rep_w["sweeps"][s]["vf"][k], rep_s["sweeps"][s]["vf"][k]
            assert 0.0 < w["cut_share"] < 1.0 and w["cut_share"] == w["off_greedy"], (s, k, w["cut_share"])
            assert p["cut_share"] == 0.0 and 0.0 < p["off_greedy"] < 1.0
            assert 1.0 <= w["horizon"] < p["horizon"], (s, k, w["horizon"], p["horizon"])
    lt = rep_w["lambda_targets"]
    assert set(lt) >= {"ag", "h", "c", "cut", "y", "y0", "yk", "sample"} and np.array_equal(lt["c"] == 0.0, lt["cut"] | ~lt["sample"])
    with pytest.raises(ScgError, match="trace must be"):
        ag.fit_values_to_returns(trajectory=traj, lam=0.9, trace="retrace")
    with pytest.raises(ScgError, match="needs lam"):
        ag.fit_values_to_returns(trajectory=traj, trace="watkins")
    with pytest.raises(ScgError, match="lam sequence"):
        ag.fit_values_to_returns(trajectory=traj, lam=[0.9, 0.9])
    with pytest.raises(ScgError, match="lam sequence"):
        ag.fit_values_to_returns(trajectory=traj, lam=[0.9, 1.5, 0.9], trace="watkins")
    with pytest.raises(ScgError, match="lam and order"):
        ag.fit_values_to_returns(trajectory=traj, lam=[0.9] * 3, order=3)


def test_trace_fit_report_runs_end_to_end_at_toy_size(tmp_path):
    from test_gpu_tools import tool
    out = tool("trace_fit_report.py", "--maps", "pinball_simple", "--seeds", 1, "--envs", 256, "--warm", 40, "--after", 8, "--steps-per-option", 16,
               "--min-examples", 64, "--episodes", 64, "--options", 2, "--lambdas", 0.5, 1.0, "--sweeps", 2, "--eval-episodes", 64,
               "--out-dir", tmp_path).splitlines()
    assert out[0].startswith("# trace_fit_report map pinball_simple envs 256 ")
    assert (tmp_path / "r34_trace_fit_pinball_simple.txt").read_text().splitlines() == out
    rows = [ln.split() for ln in out if ln.startswith("    ") and ln.split()[0] in ("peng", "watkins") and len(ln.split()) == 12]
    assert len(rows) == (1 + 2 * 2) * 2 * 3                    # lambda = 0 once, then two arms x two lambdas; two sweeps; three value functions
    assert {(r[0], r[1]) for r in rows} == {("peng", "0.00"), ("peng", "0.50"), ("peng", "1.00"), ("watkins", "0.50"), ("watkins", "1.00")}
    ran = [r for r in rows if int(r[4]) + int(r[5]) > 0]       # (a value function without a row in the record: nan)
    assert len(ran) >= len(rows) // 3 and all(0.0 <= float(r[6]) <= 1.0 and float(r[7]) >= 1.0 for r in ran)
    assert all(float(r[6]) == 0.0 for r in ran if r[0] == "peng" and r[1] != "0.00")           # cut_share of an uncut trace
    assert all(float(r[6]) == 1.0 for r in ran if r[1] == "0.00")
    pol = [ln.split() for ln in out if "+-" in ln and " table " not in ln]
    assert len(pol) == (1 + 5 * 2) * 2 and [p[0] for p in pol[:2]] == ["W", "W"] and pol[-1][0] == "watkins/1.00/2"
    assert all(float(p[5]) == 0.0 and float(p[7]) == 0.0 for p in pol[:2])       # W against itself: exact zeros
    head = [ln for ln in out if ln.startswith("  descent ")]
    assert len(head) == 5 * 2 and all(len(ln.split()) == 4 + 2 for ln in head)   # per arm and lambda and epsilon: the return over sweeps 1, 2
