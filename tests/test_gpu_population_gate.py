"""SPEC §25.1 on the GPU (scg_rollout_population_gate): a population rollout whose value gate compares under a gate table per
policy and whose every other read is W[c] as before. The yardstick is always the existing entry point, scg_rollout_population_clf
(and ScgContext.q_values for recomputed values), never the new one. The rig (Run, the map, the inputs, the policies, the launches,
the comparison) is tests/test_gpu_population.py's. In every gated call the W-shaped rows of the gate differ from the policy's W
unless the test is about their being equal, and the gate table is checked as unwritten after every call."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_population as P
from skill_chaining_with_graphs_amd import _lib, gatefit
from skill_chaining_with_graphs_amd.core import EnvState
from skill_chaining_with_graphs_amd.trajectory import offer_rows
from gpu_util import as_bytes, block_envs, clone_state, current_block_envs, dev  # noqa: F401  (block_envs: the fixture)

pytestmark = pytest.mark.gpu

INT, BEST, B, ONE, AT = P.INT, P.BEST, P.B, P.ONE, P.AT
N_OPT, K, T0, MAX_EP, REOFFER = P.N_OPT, P.K, P.T0, P.MAX_EP, P.REOFFER
assert MAX_EP == 12 and K == 8 and len(P.LAUNCHES) == 2    # the issue's inputs: two launches of 8 steps end every 12-step episode
MASK_ARG = P.MASK_ARG
SHAPES = [(3, 40), (3, 257)]
EPISODE = ("x", "y", "vx", "vy", "action", "reward", "done", "qcache", "ep_steps", "opt_steps", "stats.ep_return", "stats.ret_sum",
           "stats.episodes", "stats.goals", "stats.len_sum", "stats.finished", "stats.vf_steps", "stats.successes")


class Run(P.Run):
    def population_clf(self, W, clf, mask, t0, n_steps, flags, rules, pop, pop_clf, first=None):
        """The yardstick: scg_rollout_population_clf."""
        keep, a = self.args(W, clf, mask, t0, n_steps, flags, rules, first)
        self.ctx._call("scg_rollout_population_clf", *a, None if pop is None else C.byref(pop), _p(pop_clf))

    def population_gate(self, W, clf, mask, t0, n_steps, flags, rules, pop, pop_clf, pop_gate, first=None):
        keep, a = self.args(W, clf, mask, t0, n_steps, flags, rules, first)
        self.ctx._call("scg_rollout_population_gate", *a, None if pop is None else C.byref(pop), _p(pop_clf), _p(pop_gate))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _shipped(W):
    """shipped_gate of every policy's table, host [C][n_vf][2][5][1296]."""
    return np.stack([gatefit.shipped_gate(torch.from_numpy(w)).numpy() for w in W])


def _noisy(W, scale, seed=77):
    """shipped_gate(W[c]) plus seeded noise on every row: no W-shaped row of it equals a row of W."""
    g = _shipped(W)
    g[:, 1:] += (np.random.default_rng(seed).standard_normal(g[:, 1:].shape) * scale).astype(np.float32)
    return g


def _launch(m, parents, clf, pol, st_np, n_per, gates=None, rules=0, launches=P.LAUNCHES, force=None, first=None, block=None,
            enabled=None, entry="gate"):
    """The launches on one context of C * n_per envs; the outputs after each. gates = None with entry "clf": the yardstick."""
    W, eps, en = pol
    en = en if enabled is None else np.asarray(enabled, np.int32)
    n_pol = len(eps)
    ctx = P._context(m, parents, n_pol * n_per, 0.3, block)
    run = Run(ctx, st_np, force=force)
    Wd, ed, md = dev(W).view(-1), dev(eps), dev(en)
    gd = None if gates is None else dev(np.ascontiguousarray(gates))
    pop = P._pop_struct(n_pol, n_per, ed, md)
    fa = None if first is None else dev(first)
    snaps = []
    for t0, k, flags in launches:
        if entry == "gate":
            run.population_gate(Wd, clf, MASK_ARG, t0, k, flags, rules, pop, None, gd, fa)
        else:
            run.population_clf(Wd, clf, MASK_ARG, t0, k, flags, rules, pop, None, fa)
        snaps.append(run.outputs())
    if gates is not None:
        assert np.array_equal(as_bytes(gd), as_bytes(np.ascontiguousarray(gates))), "pop_gate was written"
    assert np.array_equal(as_bytes(Wd), as_bytes(W.reshape(-1)))
    ctx.close()
    return snaps


def _q(ctx, s, w):
    """Q(s, .) [5][len(s)] under the table w [5][1296], by ScgContext.q_values in batches of the context's size."""
    out = [ctx.q_values([dev(np.ascontiguousarray(v[i:i + ctx.n_envs])) for v in s], dev(np.ascontiguousarray(w)).view(-1)).cpu().numpy()
           for i in range(0, len(s[0]), ctx.n_envs)]
    return np.concatenate(out, axis=1)


def _same(got, want, n, msg):
    for j, (g, w) in enumerate(zip(got, want)):
        P._assert_slice(g, w, 0, n, (0, n), f"{msg} launch {j}")


def _env_rows(snaps, e):
    """Env e's recorded rows over the launches, one array per field."""
    return {f: np.concatenate([rec[f][:int(rec["len"][0, e]), e] for _, rec in snaps]) for f in snaps[0][1] if f != "len"}


def _assert_prefix(a, b, upto, msg):
    for f in a:
        assert np.array_equal(as_bytes(np.ascontiguousarray(a[f][:upto])), as_bytes(np.ascontiguousarray(b[f][:upto]))), f"{msg}: record {f}"


# ---------------------------------------------------------------------------------------------------- 1. the shipped gate is the ungated rollout

def _nonvacuous(want, n_per, n_pol, msg):
    last, first = want[-1][0], want[0][0]
    ent = [int(last["stats.entries"][:, c * n_per:(c + 1) * n_per].sum()) for c in range(n_pol)]
    dec = [int(last["stats.declines"][:, c * n_per:(c + 1) * n_per].sum()) for c in range(n_pol)]
    offered = first["audit.cand"][0] >= 1
    differ = int((first["audit.v_cand"][0][offered] != first["audit.v_root"][0][offered]).sum())
    print(f"{msg}: entries {ent}, declines {dec}, begin offers {int(offered.sum())} of which v_cand != v_root {differ}")
    assert max(ent) > 0 and max(dec) > 0 and differ > 0, msg


@pytest.mark.parametrize("block_envs", [64, 128, 256], indirect=True)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_shipped_gate_is_the_ungated_rollout(shape, block_envs, monkeypatch):
    n_pol, n_per = shape
    n = n_pol * n_per
    m, parents, clf, st_np = P._inputs(n)
    pol = P._policies(n_pol)
    monkeypatch.delenv("SCG_ROLLOUT_EPW", raising=False)
    blk = current_block_envs()
    want = _launch(m, parents, clf, pol, st_np, n_per, entry="clf", block=blk)
    _nonvacuous(want, n_per, n_pol, f"{shape} block {block_envs}")
    for epw in (None, 2, 32):
        if epw is not None:
            monkeypatch.setenv("SCG_ROLLOUT_EPW", str(epw))
        _same(_launch(m, parents, clf, pol, st_np, n_per, _shipped(pol[0]), block=blk), want, n, f"{shape} block {block_envs} epw {epw}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_shipped_gate_with_begin_at_a_force_and_a_first_action(shape):
    n_pol, n_per = shape
    n = n_pol * n_per
    m, parents, clf, st_np = P._inputs(n)
    pol = P._policies(n_pol)
    e = np.arange(n)
    force = ((e * 5 + e // n_per) % 5 - 2).astype(np.int8)                  # -2 .. +2, another pattern in every policy's range
    first = ((e * 7 + 3 * (e // n_per)) % 6).astype(np.uint8)              # 5: not forced
    kw = dict(launches=((T0, 2 * K, AT),), force=force, first=first)       # (a force needs a begin flag: one launch)
    want = _launch(m, parents, clf, pol, st_np, n_per, entry="clf", **kw)
    applied = want[0][0]["audit.applied"][0]
    assert (applied == 1).any() and (applied == 0).any()
    _same(_launch(m, parents, clf, pol, st_np, n_per, _shipped(pol[0]), **kw), want, n, f"begin_at {shape}")


# ---------------------------------------------------------------------------------------------------- 2. NULL forwards

@pytest.mark.parametrize("rules", P.ALL_RULES, ids=P.RULE_IDS)
def test_a_null_gate_is_the_population_clf_rollout(rules):
    n_pol, n_per = 3, 40
    n = n_pol * n_per
    m, parents, clf, st_np = P._inputs(n)
    pol = P._policies(n_pol)
    want = _launch(m, parents, clf, pol, st_np, n_per, entry="clf", rules=rules)
    assert int(want[-1][0]["stats.entries"].sum()) > 0
    _same(_launch(m, parents, clf, pol, st_np, n_per, None, rules=rules), want, n, f"pop_gate = NULL rules {rules}")


# ---------------------------------------------------------------------------------------------------- 3. never enter

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_never_enter_is_the_roots_trajectory(shape):
    n_pol, n_per = shape
    n = n_pol * n_per
    m, parents, clf, st_np = P._inputs(n)
    pol = P._policies(n_pol)
    gates = np.stack([gatefit.never_enter(N_OPT + 1).numpy()] * n_pol)
    got = _launch(m, parents, clf, pol, st_np, n_per, gates)
    want = _launch(m, parents, clf, pol, st_np, n_per, entry="clf", enabled=np.zeros(n_pol, np.int32))
    for j, ((g, g_rec), (w, w_rec)) in enumerate(zip(got, want)):
        for f in EPISODE:
            assert np.array_equal(as_bytes(g[f]), as_bytes(w[f])), f"launch {j}: {f} differs from the root's trajectory"
        for f in ("x", "y", "vx", "vy", "action", "reward", "done", "vf", "term", "len"):
            assert np.array_equal(as_bytes(g_rec[f]), as_bytes(w_rec[f])), f"launch {j}: record {f}"
        assert int(g["stats.entries"].sum()) == 0 and (g["option_id"] <= 0).all() and (g_rec["option_id"] <= 0).all()
        assert int(w["stats.declines"].sum()) == 0 and (w["option_id"] == 0).all()
    assert int(got[-1][0]["stats.declines"].sum()) > 0 and (got[0][1]["option_id"] < 0).any()
    assert int(want[-1][0]["stats.goals"].sum()) > 0


# ---------------------------------------------------------------------------------------------------- 4. always enter

def test_always_enter_parts_from_the_shipped_run_at_its_first_decline():
    n_pol, n_per = 3, 257
    m, parents, clf, st_np = P._inputs(n_pol * n_per)
    pol = P._policies(n_pol)
    got = _launch(m, parents, clf, pol, st_np, n_per, np.stack([gatefit.always_enter(N_OPT + 1).numpy()] * n_pol))
    ship = _launch(m, parents, clf, pol, st_np, n_per, _shipped(pol[0]))
    last = got[-1][0]
    assert int(last["stats.declines"].sum()) == 0 and int(last["stats.entries"].sum()) > 0
    parted = np.zeros(n_pol, np.int64)
    for e in range(n_pol * n_per):
        a, s = _env_rows(got, e), _env_rows(ship, e)
        neg = np.nonzero(s["option_id"] < 0)[0]            # the first negative id of an episode is a declined offer: a stay follows one
        if not len(neg):
            assert len(a["option_id"]) == len(s["option_id"])
            _assert_prefix(a, s, None, f"env {e}: the shipped run never declined")
            continue
        j = int(neg[0])
        _assert_prefix(a, s, j, f"env {e} before row {j}")
        for f in a:
            if f != "option_id":
                assert a[f][j:j + 1].tobytes() == s[f][j:j + 1].tobytes(), f"env {e} row {j}: {f}"
        assert int(a["option_id"][j]) == -int(s["option_id"][j]) >= 1, f"env {e} row {j}"
        parted[e // n_per] += 1
    print(f"always enter: envs that part from the shipped run, per policy {parted.tolist()}")
    assert (parted > 0).all()                              # every policy has options enabled


# ---------------------------------------------------------------------------------------------------- 5. a transplanted gate

def test_a_transplanted_gate_decides_as_the_other_table_does():
    n_pol, n_per = 3, 257
    n = n_pol * n_per
    m, parents, clf, st_np = P._inputs(n)
    W, eps, enabled = P._policies(n_pol)
    Wt = np.ascontiguousarray(np.roll(W, -1, axis=0))       # W'[c] = W[c + 1]: no policy's own
    assert all(not np.array_equal(Wt[c], W[c]) for c in range(n_pol))
    launches = ((T0, 0, AT),)
    got = _launch(m, parents, clf, (W, eps, enabled), st_np, n_per, _shipped(Wt), launches=launches)[0][0]
    want = _launch(m, parents, clf, (Wt, eps, enabled), st_np, n_per, entry="clf", launches=launches)[0][0]
    for f in ("audit.v_cand", "audit.cand"):
        assert np.array_equal(as_bytes(got[f]), as_bytes(want[f])), f
    off = want["audit.cand"][0] >= 1                       # v_root of an offered env: the gate's root side; of any other: its own V_0
    assert np.array_equal(as_bytes(got["audit.v_root"][0][off]), as_bytes(want["audit.v_root"][0][off])), "audit.v_root of the offered envs"
    assert np.array_equal(as_bytes(got["audit.v_root"][0][~off]), as_bytes(got["qcache"][:, ~off].max(axis=0))) and (~off).any()
    assert np.array_equal(np.sign(got["option_id"]), np.sign(want["option_id"]))
    assert np.array_equal(np.abs(got["option_id"]), np.abs(want["option_id"]))
    oid, cand = got["option_id"][0], got["audit.cand"][0].astype(np.int64)
    offered = cand >= 1
    assert (oid[offered] > 0).any() and (oid[offered] < 0).any() and (np.abs(oid[offered]) == cand[offered]).all()
    # the qcache is the policy's OWN table's: Q_cand under W[c] where entered, Q_0 under W[c] where declined (or nothing offered)
    ctx = P._context(m, parents, n_per, 0.0)
    moved = 0
    for c in range(n_pol):
        lo, hi = c * n_per, (c + 1) * n_per
        s = [st_np[f][lo:hi] for f in ("x", "y", "vx", "vy")]
        vf = np.where(oid[lo:hi] > 0, oid[lo:hi], 0)
        q = np.stack([_q(ctx, s, W[c][k]) for k in range(N_OPT + 1)])      # [k][5][n_per]
        mine = q[vf, :, np.arange(n_per)].T
        assert np.array_equal(as_bytes(got["qcache"][:, lo:hi]), as_bytes(np.ascontiguousarray(mine))), f"policy {c}: qcache"
        moved += int((got["qcache"][:, lo:hi] != want["qcache"][:, lo:hi]).any(axis=0).sum())
    ctx.close()
    assert moved > 0                                       # ... which is not what the run under W' caches


# ---------------------------------------------------------------------------------------------------- 6. record audit

NOISE = 0.05             # of crossing_weights' own scale (option rows = the root's + 0.05 noise): the sides cross both ways


def test_every_recorded_offer_is_decided_by_the_gate_tables_two_sides():
    n_pol, n_per = 3, 257
    n = n_pol * n_per
    m, parents, clf, st_np = P._inputs(n)
    pol = P._policies(n_pol)
    gates = _noisy(pol[0], NOISE)
    snaps = _launch(m, parents, clf, pol, st_np, n_per, gates)
    per = [_env_rows(snaps, e) for e in range(n)]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(p["vf"]) for p in per])
    flat = {f: np.concatenate([p[f] for p in per]) for f in per[0]}
    flat["offsets"] = off
    rows = offer_rows(flat, REOFFER, T0, np.arange(n) % n_per)
    real = ~rows["stay"]
    assert rows["stay"].any() and real.sum() >= 200
    at, env, k, entered = rows["flat"][real], rows["env"][real], rows["option"][real], rows["entered"][real]
    ctx = P._context(m, parents, n_per, 0.0)
    holds = np.zeros(len(at), bool)
    for c in range(n_pol):
        for kk in np.unique(k[env // n_per == c]):
            sel = np.nonzero((env // n_per == c) & (k == kk))[0]
            s = [flat[f][at[sel]] for f in ("x", "y", "vx", "vy")]
            v = [_q(ctx, s, gates[c, kk, side]) for side in (0, 1)]
            v_opt, v_root = (np.maximum.reduce([q[a] for a in range(5)]) for q in v)        # (no NaN here: SPEC §5's max is the max)
            holds[sel] = v_opt >= v_root
    ctx.close()
    print(f"record audit: {len(at)} offers ({int(rows['stay'].sum())} stays left out), entered {int(holds.sum())}, declined {int((~holds).sum())}")
    assert holds.mean() >= 0.1 and (~holds).mean() >= 0.1, "the noise scale does not exercise both outcomes"
    assert np.array_equal(entered, holds), f"{int((entered != holds).sum())} recorded offers disagree with the gate table"


# ---------------------------------------------------------------------------------------------------- 7. a NaN side declines

@pytest.mark.parametrize("side", [0, 1], ids=["option side", "root side"])
def test_a_nan_side_declines(side):
    n_pol, n_per, k_nan = 3, 257, 1
    m, parents, clf, st_np = P._inputs(n_pol * n_per)
    pol = P._policies(n_pol)
    gates = _shipped(pol[0])
    gates[:, k_nan, side] = np.nan
    got = _launch(m, parents, clf, pol, st_np, n_per, gates)
    ship = _launch(m, parents, clf, pol, st_np, n_per, _shipped(pol[0]))
    assert int(got[-1][0]["stats.entries"][k_nan].sum()) == 0 and int(got[-1][0]["stats.declines"][k_nan].sum()) > 0
    assert int(ship[-1][0]["stats.entries"][k_nan].sum()) > 0
    parted = 0
    for e in range(n_pol * n_per):                         # every row before the shipped run first enters k_nan is the shipped run's
        a, s = _env_rows(got, e), _env_rows(ship, e)
        ent = np.nonzero((s["option_id"] == k_nan) & (s["vf"] != k_nan))[0]
        if not len(ent):
            assert len(a["option_id"]) == len(s["option_id"])
            _assert_prefix(a, s, None, f"env {e}: option {k_nan} is never entered")
            continue
        j = int(ent[0])
        _assert_prefix(a, s, j, f"env {e} before row {j}")
        assert int(a["option_id"][j]) == -k_nan, f"env {e} row {j}"
        parted += 1
    assert parted > 0


# ---------------------------------------------------------------------------------------------------- 8. refusals

def test_refusals_in_their_sequence_launch_nothing(monkeypatch):
    n_pol, n_per = 3, 40
    n = n_pol * n_per
    m, parents, clf, st_np = P._inputs(n)
    W, eps, enabled = P._policies(n_pol)
    gates = _noisy(W, NOISE)
    tabs = np.stack([P.sibling_tree(m)[1]] * n_pol)
    Wd, ed, md, gd, td = dev(W).view(-1), dev(eps), dev(enabled), dev(gates), dev(tabs)
    monkeypatch.delenv("SCG_ROLLOUT_EPW", raising=False)
    ctx = P._context(m, parents, n, 0.3)
    run = Run(ctx, st_np, rows=2)
    before = clone_state(run.st)
    for f in P.STATS:
        getattr(run.stats, f).fill_(77)
    run.interrupts.fill_(77)
    run.overrides.fill_(77)
    first = torch.full((n,), 3, dtype=torch.uint8, device=ctx.device)
    lib = ctx.lib
    good = P._pop_struct(n_pol, n_per, ed, md)

    def call(pop, pop_clf, pop_gate, flags=B, n_steps=1, rules=0, c=ctx._ctx):
        keep, a = run.args(Wd, clf, MASK_ARG, 0, n_steps, flags, rules, first)
        rc = lib.scg_rollout_population_gate(c, *a, None if pop is None else C.byref(pop), _p(pop_clf), _p(pop_gate))
        return rc, lib.scg_last_error(c).decode()

    name = "scg_rollout_population_gate: "
    rc, msg = call(None, None, gd)
    assert rc == -1 and msg == name + "pop_gate without pop", msg
    for rules in (INT, BEST, BEST | INT):
        rc, msg = call(good, None, gd, rules=rules)
        assert rc == -1 and msg.startswith(name + "pop_gate with SCG_SELECT_INTERRUPT or SCG_SELECT_BEST"), msg
        rc, msg = call(None, None, gd, rules=rules)        # ... behind the one for a missing pop
        assert rc == -1 and msg == name + "pop_gate without pop", msg
    rc, msg = call(None, td, gd, rules=INT)                # scg_rollout_population_clf's own refusal comes before both
    assert rc == -1 and msg == name + "pop_clf without pop", msg
    # every earlier refusal wins, in scg_rollout_population_clf's sequence
    for pop, rules in ((None, 0), (good, INT)):
        for kw, theirs in ((dict(rules=4), "unknown rule"), (dict(flags=B | AT), "SCG_ROLLOUT_BEGIN and SCG_ROLLOUT_BEGIN_AT together"),
                           (dict(flags=0x80), "unknown flag"), (dict(n_steps=-1), "n_steps out of range [0, SCG_ROLLOUT_MAX_STEPS]"),
                           (dict(n_steps=2), "rec->rows too small for the launch's pseudo-steps"),
                           (dict(n_steps=0), "first_action with n_steps == 0: no real step to force")):
            rc, msg = call(pop, None, gd, **dict(dict(rules=rules), **kw))
            assert rc == -1 and msg == name + theirs, msg
    rc, msg = call(None, None, gd, c=None)
    assert rc == -1 and msg == name + "null ctx"
    monkeypatch.setenv("SCG_ROLLOUT_EPW", "3")                              # the launch geometry's refusal is an earlier one too
    rc, msg = call(good, None, gd, rules=INT)
    assert rc == -1 and msg == name + "SCG_ROLLOUT_EPW must be 2, 4, 8, 16 or 32", msg
    monkeypatch.delenv("SCG_ROLLOUT_EPW")
    for pop, why in ((P._pop_struct(0, n, ed, md), "pop->n_policies out of range [1, SCG_POP_MAX]"),
                     (P._pop_struct(n_pol, 0, ed, md), "pop->n_per must be >= 1"),
                     (P._pop_struct(n_pol, n_per + 1, ed, md), "pop->n_policies * pop->n_per is not the context's n_envs")):
        rc, msg = call(pop, None, gd, rules=BEST)
        assert rc == -1 and msg == name + why, msg
    # the wrapper refuses a misshapen table, and a gate under interruption or value-ranked choice, before the call
    W4 = dev(W)
    for bad in (gd[:2].contiguous(), gd.view(-1), gd[:, :, :1].contiguous(), gd.double(), gd.cpu(), gates, gd[:, 1:].contiguous()):
        with pytest.raises(_lib.ScgError):
            ctx.rollout(run.st, W4, clf, MASK_ARG, 0, 1, begin=True, population=(ed, md, None, bad))
    for kw in (dict(interrupt=True), dict(choose="value")):
        with pytest.raises(_lib.ScgError):
            ctx.rollout(run.st, W4, clf, MASK_ARG, 0, 1, begin=True, population=(ed, md, None, gd), **kw)
    with pytest.raises(_lib.ScgError):
        ctx.rollout(run.st, W4, clf, MASK_ARG, 0, 1, begin=True, population=(ed, md, None, gd, None))
    torch.cuda.synchronize()
    for f in EnvState.FIELDS:
        assert np.array_equal(as_bytes(getattr(run.st, f)), as_bytes(getattr(before, f))), f"a refused call wrote {f}"
    for f in P.STATS:
        assert int((getattr(run.stats, f) != 77).sum()) == 0, f"a refused call wrote stats.{f}"
    assert int((run.interrupts != 77).sum()) == 0 and int((run.overrides != 77).sum()) == 0 and int(run.rec.len.abs().sum()) == 0
    a = run.audit
    assert all(int((getattr(a, f) != P.G8).sum()) == 0 for f in ("applied", "cand"))
    assert all(int((getattr(a, f) != P.GUARD).sum()) == 0 for f in ("v_root", "v_cand", "disc_final"))
    assert (first == 3).all() and np.array_equal(as_bytes(gd), as_bytes(gates)) and np.array_equal(as_bytes(Wd), as_bytes(W.reshape(-1)))
    # well-formed: it runs; and the wrapper's four-element population is the entry point's launch, with and without a clf table
    run.stats.zero_()
    rc, _ = call(good, td, gd)
    torch.cuda.synchronize()
    assert rc == 0 and (run.rec.len == 2).all() and (run.st.action == 3).all() and np.array_equal(as_bytes(gd), as_bytes(gates))
    for pop_clf in (None, td):
        twin, ref = Run(ctx, st_np, rows=2), Run(ctx, st_np, rows=2)
        ctx.rollout(twin.st, W4, clf, MASK_ARG, 0, 1, stats=twin.stats, begin=True, first_action=first, population=(ed, md, pop_clf, gd))
        ref.population_gate(Wd, clf, MASK_ARG, 0, 1, B, 0, good, pop_clf, gd, first)
        torch.cuda.synchronize()
        for f in EnvState.FIELDS:
            assert np.array_equal(as_bytes(getattr(twin.st, f)), as_bytes(getattr(ref.st, f))), f
    ctx.close()
