"""scg_lambda_returns (SPEC §27.2) against tests/lambda_model.py, bit for bit, on synthetic records of 70 envs whose lengths sit on
the scan's chunk edges (0, 1, 2, 3, 63 .. 66, 128, 129, 200 rows) with the edge rows of tests/test_lambda_host.py planted; offsets
that leave the arrays or decrease, behind guard bands; the two identities of test_lambda_host.py on the device's output (lambda = 1:
valuefit.returns_to_go, lambda = 0: SPEC §17.2's targets); the refusals; and fit_values_to_returns(lam=...) end to end on a small
agent."""
import ctypes as C

import numpy as np
import pytest
import torch

import lambda_model as LM
import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd import ScgError
from skill_chaining_with_graphs_amd.agent import SkillChainingAgent
from skill_chaining_with_graphs_amd.core import ScgContext
from skill_chaining_with_graphs_amd.valuefit import TD_BOOT, TD_CONT, TD_END, lambda_targets, returns_to_go, td_samples
from gpu_util import dev
from util import HP, dense_map, disc_weights

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 63, 64, 65, 66, 128, 129, 200)
N_ENV, GAMMA = 70, 0.99
GUARD, FILL = 515, -777.25
FIELDS = ("reward", "done", "vf", "term", "v0", "vk")


def synthetic(seed, all_done):
    """70 envs over LENGTHS; the edge rows planted in every second env that has room; unless all_done every fifth env is a cut
    record. v0 and vk are arbitrary binary32 values."""
    rng = np.random.default_rng(seed)
    envs = []
    for e in range(N_ENV):
        L = LENGTHS[e % len(LENGTHS)]
        env = LM.synthetic_env(rng, L, end_done=all_done or e % 5 != 4)
        envs.append(LM.plant_edges(env) if L >= 12 and e % 2 else env)
    flat = LM.flatten(envs)
    total = int(flat["offsets"][-1])
    flat["v0"], flat["vk"] = (rng.normal(0, 50, total).astype(np.float32) for _ in range(2))
    return flat


@pytest.fixture(scope="module")
def ctx():
    c = ScgContext(64, 2, scg.load_map("pinball_simple"), device=0, block_envs=256, **HP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def records():
    return {"cut": synthetic(41, False), "done": synthetic(42, True)}


def device_scan(ctx, flat, lam, R, gamma=GAMMA):
    y0, yk = ctx.lambda_returns(dev(flat["offsets"]), *[dev(flat[f]) for f in FIELDS], gamma, lam, R)
    torch.cuda.synchronize()
    return y0.cpu().numpy(), yk.cpu().numpy()


def model(flat, lam, R, gamma=GAMMA, offsets=None):
    off = flat["offsets"] if offsets is None else offsets
    return LM.lambda_returns(off, len(flat["reward"]), *[flat[f] for f in FIELDS], gamma, lam, R)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("R", [0.0, 100.0])
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.9, 1.0])
def test_device_scan_equals_the_model_by_bits(ctx, records, lam, R):
    flat = records["cut"]
    inputs = [dev(flat[f]) for f in FIELDS]
    got, want = device_scan(ctx, flat, lam, R), model(flat, lam, R)
    for name, g, w in zip(("y0", "yk"), got, want):
        bad = np.nonzero(g.view(np.uint64) != w.view(np.uint64))[0]
        assert len(bad) == 0, f"{name}: {len(bad)} of {len(g)} rows differ, first row {bad[0]}: {g[bad[0]]!r} != {w[bad[0]]!r}"
    assert np.isfinite(want[0]).all() and np.any(want[1] != 0) and np.any((want[1] != want[0]) & (flat["vf"] >= 1))
    for t, f in zip(inputs, FIELDS):
        assert np.array_equal(t.cpu().numpy().view(np.uint8), flat[f].view(np.uint8)), f


def raw(ctx, n_env, off, total, arrs, gamma, lam, R, y0, yk):
    q = lambda t: C.c_void_p(0 if t is None else (t if isinstance(t, int) else t.data_ptr()))
    rc = ctx.lib.scg_lambda_returns(ctx._ctx, n_env, q(off), C.c_int64(total), *[q(t) for t in arrs], C.c_double(gamma), C.c_double(lam),
                                    C.c_double(R), q(y0), q(yk), ctx._stream())
    torch.cuda.synchronize()
    return rc


def test_offsets_that_leave_the_arrays_or_decrease_write_nothing_outside(ctx, records):
    """Every array the kernel indexes by row is `total` long and lies inside a longer allocation (the guard bands): the inputs'
    bands hold NaN (a read outside would poison a value), the outputs' a fill value that must stay."""
    flat = records["cut"]
    total = 300
    inner = lambda v, fill: torch.cat([torch.full((GUARD,), fill, dtype=v.dtype, device=v.device), v, torch.full((GUARD,), fill, dtype=v.dtype, device=v.device)])
    bufs = [inner(dev(flat[f][:total]), float("nan") if flat[f].dtype == np.float32 else 1) for f in FIELDS]
    ptrs = [b.data_ptr() + GUARD * b.element_size() for b in bufs]
    sub = {f: flat[f][:total] for f in FIELDS}
    for off, exact in (([0, 40, 140, total + 7, total + 90], True),           # past the end: clamped
                       ([-5, 70, 2 ** 40], True),                              # in front of the start, far past the end
                       ([0, 130, 60, 60, 2 ** 62, -2 ** 62, 10], False),       # decreasing: empty envs and envs that overlap (which of two
                       ([total + 1, total + 1, 0], False)):                    # writers of a row wins is not defined: the bands only)
        off = np.array(off, np.int64)
        y0, yk = (torch.full((2 * GUARD + total,), FILL, dtype=torch.float64, device="cuda:0") for _ in range(2))
        assert raw(ctx, len(off) - 1, dev(off), total, ptrs, GAMMA, 0.9, 100.0, y0.data_ptr() + 8 * GUARD, yk.data_ptr() + 8 * GUARD) == 0
        for name, y, w in zip(("y0", "yk"), (y0, yk), LM.lambda_returns(off, total, *[sub[f] for f in FIELDS], GAMMA, 0.9, 100.0)):
            h = y.cpu().numpy()
            assert np.all(h[:GUARD] == FILL) and np.all(h[GUARD + total:] == FILL), (name, off)
            if exact:
                owned = np.zeros(total, bool)
                for e in range(len(off) - 1):
                    owned[min(max(off[e], 0), total): min(max(off[e + 1], 0), total)] = True
                assert same_bits(h[GUARD: GUARD + total][owned], w[owned]) and np.all(h[GUARD: GUARD + total][~owned] == FILL), (name, off)
                assert np.isfinite(w).all()


def test_the_two_identities_on_the_device_output(ctx, records):
    flat = records["done"]
    L = np.diff(flat["offsets"])
    env = np.repeat(np.arange(N_ENV), L)
    step = (np.arange(len(env)) - flat["offsets"][:-1][env]) >= 1
    opt = flat["vf"] >= 1
    # lambda = 1, every env ending done: the Monte-Carlo return
    tg0 = returns_to_go(flat, GAMMA, 0.0)
    y0, yk = device_scan(ctx, flat, 1.0, 0.0)
    assert same_bits(y0, tg0["g"]) and same_bits(yk[opt], tg0["g"][opt]) and not yk[~opt].any()
    R = 100.0
    tg = returns_to_go(flat, GAMMA, R)
    y0, yk = device_scan(ctx, flat, 1.0, R)
    assert same_bits(y0, tg["g"])
    r_abs = np.abs(flat["reward"].astype(np.float64))
    for e in range(N_ENV):
        sl = slice(flat["offsets"][e], flat["offsets"][e + 1])
        bound = (L[e] + 2) * 2.0 ** -52 * (np.cumsum(r_abs[sl][::-1])[::-1] + R)
        assert np.all(np.abs(yk[sl] - tg["y"][sl])[opt[sl]] <= bound[opt[sl]]), e
    assert np.any(tg["y"][opt] != tg["g"][opt])
    # lambda = 0: SPEC §17.2's one-step targets
    y0, yk = device_scan(ctx, flat, 0.0, R)
    r64, b0, bk = (flat[f].astype(np.float64) for f in ("reward", "v0", "vk"))
    live, end = step & (flat["done"] == 0), step & (flat["done"] != 0)
    assert same_bits(y0[live], (r64 + GAMMA * b0)[live]) and same_bits(y0[end], r64[end]) and not y0[~step].any()
    kinds = set()
    for k in (1, 2):
        it = td_samples(flat, k, R)
        rows, kind = it["rows"], it["kind"]
        m = np.where(kind == TD_CONT, bk[rows], np.where(kind == TD_BOOT, b0[rows], 0.0))
        assert same_bits(yk[rows], np.where(kind == TD_END, it["r"], it["r"] + GAMMA * m)), k
        kinds |= set(int(v) for v in kind)
    assert kinds == {TD_CONT, TD_BOOT, TD_END}


def test_refusals_write_nothing(ctx, records):
    flat = records["done"]
    total = len(flat["reward"])
    off, arrs = dev(flat["offsets"]), [dev(flat[f]) for f in FIELDS]
    y0, yk = (torch.full((total,), FILL, dtype=torch.float64, device="cuda:0") for _ in range(2))
    base = dict(n_env=N_ENV, off=off, total=total, gamma=GAMMA, lam=0.5, y0=y0, yk=yk, **dict(zip(FIELDS, arrs)))
    cases = [("n_env must be", dict(n_env=-1)), ("total must be", dict(total=-1)), ("total must be", dict(total=-1, off=None, lam=2.0))]
    cases += [("null array", {f: None}) for f in ("off", "y0", "yk") + FIELDS] + [("null array", dict(y0=None, gamma=float("nan")))]
    cases += [("gamma must be", dict(gamma=v)) for v in (-0.1, 1.5, float("nan"))] + [("lam must be", dict(lam=v)) for v in (-1e-9, 1.0000001, float("nan"))]
    for want, kw in cases:
        k = dict(base, **kw)
        assert raw(ctx, k["n_env"], k["off"], k["total"], [k[f] for f in FIELDS], k["gamma"], k["lam"], 100.0, k["y0"], k["yk"]) == -1, (want, kw)
        err = ctx.lib.scg_last_error(ctx._ctx)
        assert b"scg_lambda_returns" in err and want.encode() in err, (want, kw, err)
        assert torch.all(y0 == FILL) and torch.all(yk == FILL)
    assert raw(ctx, 0, off, total, arrs, GAMMA, 0.5, 0.0, y0, yk) == 0 and torch.all(y0 == FILL) and torch.all(yk == FILL)
    with pytest.raises(ScgError):
        ctx.lambda_returns(off.cpu(), *arrs, GAMMA, 0.5, 0.0)
    with pytest.raises(ScgError):
        ctx.lambda_returns(off, *arrs, GAMMA, 1.5, 0.0)
    bad = dict(flat, offsets=np.array([0, 5, 3, total], np.int64), x=flat["reward"], y=flat["reward"], vx=flat["reward"], vy=flat["reward"])
    with pytest.raises(ScgError, match="offsets"):                                # lambda_targets checks the offsets on the host
        lambda_targets(ctx, bad, dev(np.zeros((3, 5, 1296), np.float32)), GAMMA, 0.5, 0.0)


# ---------------------------------------------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def small_agent():
    """tests/test_gpu_value_fit.py's agent (option 2 runs from the start, option 1 gestates) at r_option_success = 0, and one kept
    record of 64 episodes."""
    m = dense_map()
    ag = SkillChainingAgent(m, 256, 2, seed=5, block_envs=256, **dict(HP, max_episode_steps=63, r_option_success=0.0))
    ag.init_weights(std=0.05, seed=3)
    sx, sy = (float(v) for v in m.starts[0])
    clf = np.zeros((3, 8), np.float32)
    clf[1], clf[2] = -disc_weights(sx, sy, 0.04), disc_weights(0.5, 0.5, 1.5)
    ag.clf.copy_(dev(clf))
    ag.enable_option(2)
    ag.gest_mask = 0b010
    ag.gest_counts = ag.ctx.set_gestation(ag.gest_mask)
    report, W_mc = ag.fit_values_to_returns(n_episodes=64, epsilon=0.5, seed=9, keep=True)
    yield ag, report, W_mc
    ag.ctx.close()


def test_fit_at_lambda_one_is_the_monte_carlo_fit_by_bits(small_agent):
    ag, report, W_mc = small_agent
    traj = report["trajectory"]
    flat = traj.to_numpy()
    assert np.all(flat["done"][flat["offsets"][1:] - 1] != 0), "every recorded episode must end done"
    assert sum(report["vf"][0]["n"]) > 100 and sum(report["vf"][2]["n"]) > 20, "both value functions must run"
    rep_none, W_none = ag.fit_values_to_returns(trajectory=traj, epsilon=0.5, seed=9)
    rep_one, W_one = ag.fit_values_to_returns(trajectory=traj, epsilon=0.5, seed=9, lam=1.0, keep=True)
    assert torch.equal(W_none.view(torch.int32), W_mc.view(torch.int32))
    assert torch.equal(W_one.view(torch.int32), W_none.view(torch.int32)) and not torch.equal(W_one, ag.W)
    assert "lam" not in rep_none and rep_one["lam"] == 1.0 and len(rep_one["sweeps"]) == 1
    lt = rep_one["lambda_targets"]
    assert same_bits(lt["y"], report["targets"]["y"]) and np.array_equal(lt["sample"], report["targets"]["sample"])
    for k in (0, 2):                                                             # judged on §16's scale: at lambda = 1 the same numbers
        assert rep_one["vf"][k]["mc"]["held_out"] == rep_one["vf"][k]["held_out"] == rep_none["vf"][k]["held_out"]


def test_sweeps_report_and_leave_the_agent_alone(small_agent):
    ag, report, _ = small_agent
    W0 = ag.W.clone()
    rep, W_new = ag.fit_values_to_returns(trajectory=report["trajectory"], epsilon=0.5, seed=9, lam=0.5, sweeps=2, apply=False)
    torch.cuda.synchronize()
    assert torch.equal(ag.W, W0) and not torch.equal(W_new, W0)
    assert rep["lam"] == 0.5 and len(rep["sweeps"]) == 2 and rep["vf"] is rep["sweeps"][1]["vf"]
    assert torch.equal(rep["sweeps"][1]["W"], W_new) and not torch.equal(rep["sweeps"][0]["W"], W_new)
    for sw in rep["sweeps"]:
        for k in (0, 2):
            mc = sw["vf"][k]["mc"]["held_out"]
            assert mc["old"]["n"] == sw["vf"][k]["held_out"]["old"]["n"] > 0 and np.isfinite(mc["new"]["rmse"])
    with pytest.raises(ScgError, match="lam and order"):
        ag.fit_values_to_returns(trajectory=report["trajectory"], lam=0.5, order=3)
    with pytest.raises(ScgError, match="lam must be"):
        ag.fit_values_to_returns(trajectory=report["trajectory"], lam=1.5)
    with pytest.raises(ScgError, match="sweeps"):
        ag.fit_values_to_returns(trajectory=report["trajectory"], sweeps=2)


def test_lambda_fit_report_runs_end_to_end_at_toy_size(tmp_path):
    from test_gpu_tools import tool
    out = tool("lambda_fit_report.py", "--maps", "pinball_simple", "--seeds", 1, "--envs", 256, "--warm", 40, "--after", 8, "--steps-per-option", 16,
               "--min-examples", 64, "--episodes", 64, "--options", 2, "--lambdas", 0.5, 1.0, "--sweeps", 2, "--eval-episodes", 64,
               "--out-dir", tmp_path).splitlines()
    assert out[0].startswith("# lambda_fit_report map pinball_simple envs 256 ")
    assert (tmp_path / "r33_lambda_fit_pinball_simple.txt").read_text().splitlines() == out
    rows = [ln.split() for ln in out if ln.startswith("      ") and len(ln.split()) == 12]
    assert len(rows) == 2 * 2 * 3 and {r[0] for r in rows} == {"0.50", "1.00"} and {r[1] for r in rows} == {"1", "2"}
    pol = [ln.split() for ln in out if "+-" in ln and " table " not in ln]
    assert len(pol) == (1 + 2 * 2) * 2 and [p[0] for p in pol[:2]] == ["W", "W"] and pol[-1][0] == "1.00/2"
    assert all(float(p[5]) == 0.0 and float(p[7]) == 0.0 for p in pol[:2])       # W against itself: exact zeros
