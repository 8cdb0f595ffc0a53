"""SPEC §26 on the GPU (scg_step_gated): a step-batch whose entry decisions of the masked options compare under a gate table.

Through the C-ABI, on the three block builds. The yardsticks are existing entry points and the host model: scg_step (the shipped
gate, refreshed before every step, is the plain learner by bits; G, n_k and the applied W of a gated step are the plain step's),
scg_rollout_population_gate with C = 1 (an independent kernel that decides under the same table) and tests/step_gate_model.py
(the oracle's primitives). The scenarios are step_gate_model.scenario's: 257 and 300 envs (a partial last block, more than one
block on every build, more than one row of 256 for the histogram move), a chain and a tree of three options, re-offer periods 1
and 4, an env id base past 2^33. The gate table sits between guard bands and is compared by bytes after every call.

tests/test_step_gate_model.py shows on the CPU that the noisy table flips offers both ways in these scenarios, on every build's
oracle; the tests here assert it again on what the library did."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_gate_model as M
import test_gpu_population as P
import test_gpu_population_gate as PG
from gpu_util import (as_bytes, assert_same_bits, block_envs, clone_state, crossing_agent, current_block_envs, dev,  # noqa: F401
                      host_state, make_context, spy_calls, state_to_device)                                          # (block_envs: the fixture)
from skill_chaining_with_graphs_amd import ScgError, _lib, gatefit
from skill_chaining_with_graphs_amd.core import EnvState

pytestmark = pytest.mark.gpu

LEARN, APPLY, INTERRUPT = _lib.STEP_LEARN, _lib.STEP_APPLY, _lib.STEP_INTERRUPT
N_VF = M.N_OPT + 1
FULL = M.full_mask(N_VF)
TAB = N_VF * 2 * M.NACT * M.NF
GUARD = 256                                    # floats either side of the table
CASES = [(257, "chain", 4, 0), (300, "tree", 1, 0), (300, "chain", 4, (1 << 33) + 77)]
IDS = ["257-chain-reoffer4", "300-tree-reoffer1", "300-chain-base2^33"]
BUILDS = [64, 128, 256]
K_ACT = 16


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Rig:
    """One context on a scenario: the env state, W, clf, the grad buffers, and a gate table between guard bands."""

    def __init__(self, sc, st_np=None):
        self.sc = sc
        self.ctx = make_context(sc["map"], sc["n"], M.N_OPT, current_block_envs(), sc["parents"], 0, sc["seed"],
                                env_id_base=sc["env_id_base"], **sc["hp"])
        self.st = state_to_device(sc["state"] if st_np is None else st_np, self.ctx)
        self.W = dev(sc["W"]).view(-1).clone()
        self.clf = dev(sc["clf"]).view(-1)
        self.G, self.nk = self.ctx.grad_buffers()
        self.gbuf = torch.full((GUARD + TAB + GUARD,), -777.25, dtype=torch.float32, device=self.ctx.device)
        self.gate = self.gbuf[GUARD:GUARD + TAB]
        self.gref = self.gbuf.clone()

    def set_gate(self, table):
        self.gate.copy_(torch.as_tensor(np.ascontiguousarray(table) if isinstance(table, np.ndarray) else table).reshape(-1))
        self.gref = self.gbuf.clone()

    def call(self, t, flags, mask, gate="own", plain=False, st=None):
        st = self.st if st is None else st
        a = [_p(getattr(st, f)) for f in EnvState.FIELDS] + [_p(self.W), _p(self.clf), C.c_uint32(M.ENABLED), C.c_uint64(t),
                                                              C.c_uint32(flags), self.ctx._stream()]
        lib = self.ctx.lib
        if plain:
            rc = lib.scg_step(self.ctx._ctx, *a)
        else:
            rc = lib.scg_step_gated(self.ctx._ctx, *a, _p(self.gate) if gate == "own" else gate, C.c_uint32(mask))
        return rc, lib.scg_last_error(self.ctx._ctx).decode()

    def step(self, t, flags=LEARN | APPLY, mask=FULL, **kw):
        rc, msg = self.call(t, flags, mask, **kw)
        assert rc == 0, msg

    def load(self, st, W):
        """Another state and W into this rig's arrays (the prepared env order no longer holds)."""
        for f in EnvState.FIELDS:
            getattr(self.st, f).copy_(getattr(st, f) if not isinstance(st, dict) else dev(st[f]))
        self.W.copy_(W.reshape(-1) if isinstance(W, torch.Tensor) else dev(W).view(-1))
        self.ctx.invalidate_order()

    def gate_unwritten(self):
        torch.cuda.synchronize()
        assert np.array_equal(as_bytes(self.gbuf), as_bytes(self.gref)), "the gate table or its guard bands were written"

    def outputs(self):
        torch.cuda.synchronize()
        return dict(host_state(self.st), W=self.W.cpu().numpy().copy(), G=self.G.cpu().numpy().copy(), n_k=self.nk.cpu().numpy().copy())

    def close(self):
        self.ctx.close()


ALL = EnvState.FIELDS + ("W", "G", "n_k")


def _same(a, b, msg, fields=ALL):
    assert_same_bits(a, b, fields=[f for f in fields if f not in ("W", "G", "n_k")], msg=msg)
    for f in fields:
        if f in ("W", "G", "n_k"):
            assert np.array_equal(as_bytes(a[f]), as_bytes(b[f])), f"{msg}: {f} differs"


def _flips(gated, plain):
    """(entered -> declined, declined -> entered) of a gated step against the plain step from the same state, by the ids left."""
    g, p = gated["option_id"].astype(np.int64), plain["option_id"].astype(np.int64)
    return int(((p > 0) & (g == -p)).sum()), int(((p < 0) & (g == -p)).sum())


class Roll:
    """scg_rollout_population_gate with C = 1 on a context of its own: the independent kernel of test 2 and 3."""

    def __init__(self, sc):
        self.ctx = make_context(sc["map"], sc["n"], M.N_OPT, current_block_envs(), sc["parents"], 0, sc["seed"],
                                env_id_base=sc["env_id_base"], **sc["hp"])
        self.run = PG.Run(self.ctx, sc["state"])
        self.eps, self.en = dev(np.array([sc["hp"]["epsilon"]], np.float32)), dev(np.array([M.ENABLED], np.int32))
        self.pop = P._pop_struct(1, sc["n"], self.eps, self.en)
        self.clf = dev(sc["clf"]).view(-1)

    def launch(self, st, W, gate, t0, k):
        for f in EnvState.FIELDS:
            getattr(self.run.st, f).copy_(getattr(st, f))
        self.run.population_gate(W, self.clf, M.ENABLED, t0, k, 0, 0, self.pop, None, gate)
        torch.cuda.synchronize()
        return host_state(self.run.st)

    def close(self):
        self.ctx.close()


# ---------------------------------------------------------------------------------------------------- 1. identity, learning

@pytest.mark.parametrize("block_envs", BUILDS, indirect=True)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_shipped_gate_refreshed_every_step_is_the_plain_learner(case, block_envs):
    sc = M.scenario(*case)
    a, b = Rig(sc), Rig(sc)
    entered = declined = 0
    for j in range(M.STEPS):
        a.set_gate(gatefit.shipped_gate(a.W.view(N_VF, M.NACT, M.NF)))
        before = a.st.option_id.clone()
        a.step(M.T0 + j)
        b.step(M.T0 + j, plain=True)
        _same(a.outputs(), b.outputs(), f"{case} block {block_envs} step {j}")
        a.gate_unwritten()
        now = a.st.option_id
        entered += int(((now > 0) & (now != before)).sum())
        declined += int((now < 0).sum())
    assert entered > 100 and declined > 100, (entered, declined)       # the kernel had offers of both outcomes to decide
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------- 2. acting, against an independent kernel

@pytest.mark.parametrize("block_envs", BUILDS, indirect=True)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_acting_steps_under_a_noisy_table_equal_the_population_gate_rollout(case, block_envs):
    sc = M.scenario(*case)
    a, r = Rig(sc), Roll(sc)
    a.set_gate(M.noisy_gate(sc["W"]))
    want = r.launch(a.st, a.W, a.gate, M.T0, K_ACT)
    plain = Rig(sc)
    for j in range(K_ACT):
        a.step(M.T0 + j, flags=0)
        plain.step(M.T0 + j, flags=0, plain=True)
    got = a.outputs()
    assert_same_bits(got, want, msg=f"{case} block {block_envs}")
    assert np.array_equal(got["W"], sc["W"].reshape(-1))
    assert not np.array_equal(got["option_id"], plain.outputs()["option_id"])          # the table mattered
    a.gate_unwritten()
    a.close(), r.close(), plain.close()


# ---------------------------------------------------------------------------------------------------- 3. learning with a noisy table

@pytest.mark.parametrize("block_envs", BUILDS, indirect=True)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_gated_learning_step_learns_as_the_plain_step_and_acts_as_the_table_says(case, block_envs):
    sc = M.scenario(*case)
    a, b, r = Rig(sc), Rig(sc), Roll(sc)
    orc = M.make_oracle(sc)
    st_h, W_h = M.oracle_state(sc), sc["W"].copy()
    to_d = to_e = m_d = m_e = 0
    for j in range(M.STEPS):
        t = M.T0 + j
        gate_h = M.noisy_gate(W_h)
        a.set_gate(gate_h)
        pre, W_pre = clone_state(a.st), a.W.clone()
        b.load(pre, W_pre)
        a.step(t)
        b.step(t, plain=True)
        got, plain = a.outputs(), b.outputs()
        msg = f"{case} block {block_envs} step {j}"
        _same(got, plain, msg + " (learning)", fields=("W", "G", "n_k"))
        _same(got, plain, msg + " (what the gate does not touch)",
              fields=("x", "y", "vx", "vy", "opt_steps", "ep_steps", "action", "reward", "done"))
        assert_same_bits(got, r.launch(pre, W_pre, a.gate, t, 1), msg=msg + " (population-gate launch)")
        st_h, G, n_k, info = M.step(orc, st_h, W_h, sc["clf"], t, M.ENABLED, gate_h, FULL)
        W_h = M.apply(orc, W_h, G, n_k)
        assert_same_bits(got, st_h, msg=msg + " (host model)")
        assert np.array_equal(as_bytes(got["W"]), as_bytes(W_h.reshape(-1))), msg + ": W differs from the model's"
        d, e = _flips(got, plain)
        to_d, to_e, m_d, m_e = to_d + d, to_e + e, m_d + int(info["to_declined"].sum()), m_e + int(info["to_entered"].sum())
        a.gate_unwritten()
    print(f"{case} block {block_envs}: entered -> declined {to_d}, declined -> entered {to_e}")
    assert (to_d, to_e) == (m_d, m_e) and to_d >= 1 and to_e >= 1
    a.close(), b.close(), r.close()


@pytest.mark.parametrize("envs", [64, 128, 256])
def test_every_scan_range_of_the_gate_launch_gives_the_same_results(envs, monkeypatch):
    """The gate launch picks its positions per workgroup from the env count (64 at these sizes); SCG_STEP_GATE_ENVS pins it. Each
    of the three against the host model, learning, with flips both ways and the order checked by the steps that follow."""
    monkeypatch.setenv("SCG_STEP_GATE_ENVS", str(envs))
    sc = M.scenario(*CASES[1])
    a = Rig(sc)
    orc = M.make_oracle(sc)
    st_h, W_h = M.oracle_state(sc), sc["W"].copy()
    to_d = to_e = 0
    for j in range(6):
        gate_h = M.noisy_gate(W_h)
        a.set_gate(gate_h)
        a.step(M.T0 + j)
        st_h, G, n_k, info = M.step(orc, st_h, W_h, sc["clf"], M.T0 + j, M.ENABLED, gate_h, FULL)
        W_h = M.apply(orc, W_h, G, n_k)
        got = a.outputs()
        assert_same_bits(got, st_h, msg=f"envs {envs} step {j}")
        assert np.array_equal(as_bytes(got["W"]), as_bytes(W_h.reshape(-1))) and np.array_equal(as_bytes(got["G"]), as_bytes(G))
        to_d, to_e = to_d + int(info["to_declined"].sum()), to_e + int(info["to_entered"].sum())
    assert to_d >= 1 and to_e >= 1
    a.gate_unwritten()
    a.close()


# ---------------------------------------------------------------------------------------------------- 4. the order after a flip

@pytest.mark.parametrize("block_envs", BUILDS, indirect=True)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_order_a_gated_learning_step_leaves_is_a_fresh_sort(case, block_envs):
    sc = M.scenario(*case)
    a, b, plain = Rig(sc), Rig(sc), Rig(sc)
    for r in (a, b):
        r.set_gate(M.noisy_gate(sc["W"]))
        r.step(M.T0)
    plain.step(M.T0, plain=True)
    d, e = _flips(a.outputs(), plain.outputs())
    assert d >= 1 and e >= 1, (d, e)                               # counts moved in hist_next in both directions
    _same(a.outputs(), b.outputs(), "the gated step itself")
    b.ctx.invalidate_order()
    for j in (1, 2):
        a.step(M.T0 + j, plain=True)
        b.step(M.T0 + j, plain=True)
        _same(a.outputs(), b.outputs(), f"{case} block {block_envs}: step {j} behind the gated step")
    a.close(), b.close(), plain.close()


# ---------------------------------------------------------------------------------------------------- 5. mask per option

@pytest.mark.parametrize("block_envs", BUILDS, indirect=True)
def test_a_masked_option_follows_the_table_and_the_others_follow_w(block_envs):
    sc = M.scenario(*CASES[0])
    a = Rig(sc)
    never = gatefit.never_enter(N_VF).numpy()
    a.set_gate(never)
    orc = M.make_oracle(sc)
    st_h, W_h = M.oracle_state(sc), sc["W"].copy()
    offers2 = others = 0
    for j in range(M.STEPS):
        a.step(M.T0 + j, mask=0b0100)
        st_h, G, n_k, info = M.step(orc, st_h, W_h, sc["clf"], M.T0 + j, M.ENABLED, never, 0b0100)
        W_h = M.apply(orc, W_h, G, n_k)
        got = a.outputs()
        assert_same_bits(got, st_h, msg=f"block {block_envs} step {j}")            # options 1 and 3: §4.2's decision on W, by the model
        two = info["entering"] & (info["cand"] == 2)
        assert (got["option_id"][two] == -2).all()                                # every offer of option 2 writes -2
        assert not ((got["option_id"] == 2) & ~info["keep"]).any()                 # ... and it is never entered
        offers2 += int(two.sum())
        others += int((info["entering"] & ~two & ~info["declined"]).sum())
    assert offers2 > 0 and others > 0
    a.gate_unwritten()
    a.close()


# ---------------------------------------------------------------------------------------------------- 6. always / never

@pytest.mark.parametrize("block_envs", BUILDS, indirect=True)
@pytest.mark.parametrize("which", ["never", "always"])
def test_always_and_never_enter_with_every_option_masked(which, block_envs):
    sc = M.scenario(*CASES[1])
    a = Rig(sc)
    table = (gatefit.never_enter if which == "never" else gatefit.always_enter)(N_VF).numpy()
    a.set_gate(table)
    orc = M.make_oracle(sc)
    st_h, W_h = M.oracle_state(sc), sc["W"].copy()
    offers = 0
    for j in range(M.STEPS):
        before = a.outputs()["option_id"]
        a.step(M.T0 + j)
        st_h, G, n_k, info = M.step(orc, st_h, W_h, sc["clf"], M.T0 + j, M.ENABLED, table, FULL)
        W_h = M.apply(orc, W_h, G, n_k)
        got = a.outputs()
        assert_same_bits(got, st_h, msg=f"{which} block {block_envs} step {j}")
        now = got["option_id"]
        if which == "never":
            assert not ((before <= 0) & (now > 0)).any() and not ((now > 0) & ~info["keep"]).any()
        else:
            assert not ((now < 0) & ~info["stay"]).any()                           # no fresh -k: every negative id is a stay
            assert (now[info["entering"]] > 0).all()
        offers += int(info["entering"].sum())
    assert offers > 100
    a.gate_unwritten()
    a.close()


# ---------------------------------------------------------------------------------------------------- 7. a NaN side declines

@pytest.mark.parametrize("block_envs", BUILDS, indirect=True)
@pytest.mark.parametrize("side", [0, 1], ids=["option side", "root side"])
def test_a_nan_side_declines(side, block_envs):
    sc = M.scenario(*CASES[0])
    a = Rig(sc)
    orc = M.make_oracle(sc)
    st_h, W_h = M.oracle_state(sc), sc["W"].copy()
    offers = 0
    for j in range(4):
        table = M.shipped(W_h)
        table[1, side] = np.nan
        a.set_gate(table)
        a.step(M.T0 + j)
        st_h, G, n_k, info = M.step(orc, st_h, W_h, sc["clf"], M.T0 + j, M.ENABLED, table, FULL)
        W_h = M.apply(orc, W_h, G, n_k)
        got = a.outputs()
        assert_same_bits(got, st_h, msg=f"side {side} block {block_envs} step {j}")
        one = info["entering"] & (info["cand"] == 1)
        assert (got["option_id"][one] == -1).all()
        offers += int(one.sum())
        a.gate_unwritten()
    assert offers > 0
    a.close()


# ---------------------------------------------------------------------------------------------------- 8. the refusals, in sequence

def _guarded(t):
    """A copy of tensor t between guard bands: (whole buffer, the view to pass)."""
    n = t.numel()
    buf = torch.empty(n + 128, dtype=t.dtype, device=t.device)
    buf.view(torch.uint8).fill_(0x5a)
    buf[64:64 + n].copy_(t.reshape(-1))
    return buf, buf[64:64 + n]


def test_the_refusals_in_their_sequence_write_nothing(monkeypatch):
    monkeypatch.setenv("SCG_STEP_GATE_ENVS", "96")             # the launch geometry's refusal is the last one (lifted below)
    sc = M.scenario(*CASES[0])
    a = Rig(sc)
    a.set_gate(M.noisy_gate(sc["W"]))
    bufs = {f: _guarded(getattr(a.st, f)) for f in EnvState.FIELDS}
    st = object.__new__(EnvState)
    st.n = a.st.n
    for f in EnvState.FIELDS:
        setattr(st, f, bufs[f][1])
    wbuf, a.W = _guarded(a.W)
    before = {f: b.clone() for f, (b, _) in bufs.items()}
    w_before, g_before, nk_before = wbuf.clone(), a.G.clone(), a.nk.clone()
    name = "scg_step_gated: "
    no_table, bad_mask = name + "gate_mask without a gate table", name + "gate_mask names the root"
    with_int, with_diag = name + "gate_mask with SCG_STEP_INTERRUPT", name + "gate_mask with the diagnostic flag 0x100"
    LI = LEARN | INTERRUPT
    for flags, mask, gate, want in [
            (LEARN, 0b0010, None, no_table), (LEARN, 0b0001, None, no_table), (LI | 0x100, 1 << N_VF, None, no_table),      # 1 before 2, 3, 4
            (LEARN, 0b0001, "own", bad_mask), (LEARN, 0b0011, "own", bad_mask), (LEARN, 1 << N_VF, "own", bad_mask),
            (LEARN, 1 << 31, "own", bad_mask), (LI | 0x100, 1 << N_VF, "own", bad_mask),                                 # 2 before 3, 4
            (LI, FULL, "own", with_int), (LI | 0x100, 0b0100, "own", with_int),                                         # 3 before 4
            (LEARN | 0x100, FULL, "own", with_diag), (0x100, 0b0010, "own", with_diag),
            # scg_step's own refusals come first
            (INTERRUPT, FULL, None, "scg_step: SCG_STEP_INTERRUPT without SCG_STEP_LEARN"),
            (INTERRUPT | 0x100, 0b0001, "own", "scg_step: SCG_STEP_INTERRUPT without SCG_STEP_LEARN")]:
        rc, msg = a.call(M.T0, flags, mask, gate=gate, st=st)
        assert rc == -1 and msg.startswith(want), (flags, mask, gate, msg)
    rc, msg = a.call(M.T0, LEARN | APPLY, FULL, st=st)
    assert rc == -1 and msg == name + "SCG_STEP_GATE_ENVS must be 64, 128 or 256", msg
    torch.cuda.synchronize()
    for f, (b, _) in bufs.items():
        assert np.array_equal(as_bytes(b), as_bytes(before[f])), f"a refused call wrote {f}"
    assert np.array_equal(as_bytes(wbuf), as_bytes(w_before)) and np.array_equal(as_bytes(a.G), as_bytes(g_before))
    rc, msg = a.call(M.T0, LEARN | APPLY, 0, st=st, gate=None)   # ... and no refusal of a call without a mask: scg_step
    assert rc == 0, msg
    for f, (b, _) in bufs.items():                               # (that step ran: from here on its results are the arrays' contents)
        before[f] = b.clone()
    w_before, g_before, nk_before = wbuf.clone(), a.G.clone(), a.nk.clone()
    keep_x = st.x
    st.x = None
    rc, msg = a.call(M.T0, LEARN, 0b0001, gate=None, st=st)
    assert rc == -1 and msg == "scg_step: null array argument", msg
    st.x = keep_x
    assert a.ctx.lib.scg_step_gated(None, *([None] * 13), 0, 0, 0, None, None, 1) == -1
    torch.cuda.synchronize()
    for f, (b, _) in bufs.items():
        assert np.array_equal(as_bytes(b), as_bytes(before[f])), f"a refused call wrote {f}"
    assert np.array_equal(as_bytes(wbuf), as_bytes(w_before)) and np.array_equal(as_bytes(a.G), as_bytes(g_before))
    assert np.array_equal(as_bytes(a.nk), as_bytes(nk_before))
    a.gate_unwritten()
    # the refused calls left the context usable: the same call, well-formed, runs
    monkeypatch.delenv("SCG_STEP_GATE_ENVS")
    rc, msg = a.call(M.T0 + 1, LEARN | APPLY, FULL, st=st)
    assert rc == 0, msg
    torch.cuda.synchronize()
    for f, (b, _) in bufs.items():                              # ... and writes inside the arrays only
        assert (as_bytes(b[:64]) == 0x5a).all() and (as_bytes(b[-64:]) == 0x5a).all(), f"guard band of {f}"
    assert (as_bytes(wbuf[:64]) == 0x5a).all() and (as_bytes(wbuf[-64:]) == 0x5a).all()
    a.close()


@pytest.mark.parametrize("block_envs", BUILDS, indirect=True)
def test_a_zero_mask_is_scg_step(block_envs):
    sc = M.scenario(*CASES[2])
    plain, null, table = Rig(sc), Rig(sc), Rig(sc)
    table.set_gate(np.full(TAB, np.nan, np.float32))
    for j in range(4):
        flags = (LEARN | APPLY) if j < 3 else 0
        plain.step(M.T0 + j, flags=flags, plain=True)
        null.step(M.T0 + j, flags=flags, mask=0, gate=None)
        table.step(M.T0 + j, flags=flags, mask=0)
        want = plain.outputs()
        _same(null.outputs(), want, f"block {block_envs} step {j}: mask 0, NULL table")
        _same(table.outputs(), want, f"block {block_envs} step {j}: mask 0, a table of NaNs")
    table.gate_unwritten()
    plain.close(), null.close(), table.close()


# ---------------------------------------------------------------------------------------------------- 9. Python

def _agents(n=300, **kw):
    return crossing_agent(n=n, **kw), crossing_agent(n=n, **kw)


def test_learner_gate_drives_step_batch():
    ag, twin = _agents()
    n_vf = ag.n_vf
    before = ag.state_dict()
    ag.set_learner_gate(gatefit.never_enter(n_vf))
    assert ag.learner_gate_mask == 0b110 and ag.learner_gate.device == ag.ctx.device and ag.gate is None
    after = ag.state_dict()
    assert sorted(after) == sorted(before) and not any("gate" in k for k in after)
    for k in ("W", "clf"):
        assert torch.equal(after[k], before[k])
    with spy_calls(ag.ctx) as (calls, steps):
        ag.step_batch()
        ag.step_batch(learn=False)
    assert "scg_step_gated" in calls and "scg_step" not in calls
    assert set(calls) <= {"step", "scg_step_gated", "scg_invalidate_order"} and calls.count("step") == 2
    for _ in range(30):                                          # longer than an option may run (max_option_steps = 25)
        ag.step_batch()
        twin.step_batch()
    torch.cuda.synchronize()
    assert int((ag.state.option_id > 0).sum()) == 0 and int((twin.state.option_id > 0).sum()) > 0
    assert int((ag.state.option_id < 0).sum()) > 0
    # the default options: the rows that differ from zero
    t = gatefit.always_enter(n_vf)
    t[2, 0, :, 3] = 0.5
    ag.set_learner_gate(t)
    assert ag.learner_gate_mask == 0b100
    ag.set_learner_gate(gatefit.always_enter(n_vf), options=[1])
    assert ag.learner_gate_mask == 0b010
    ag.set_learner_gate(None)
    assert ag.learner_gate is None and ag.learner_gate_mask == 0
    with spy_calls(ag.ctx) as (calls, steps):
        ag.ctx.invalidate_order()
        ag.step_batch()
    assert "scg_step" in calls and "scg_step_gated" not in calls


def test_the_evaluation_gate_alone_changes_nothing_in_training():
    ag, twin = _agents()
    ag.gate = gatefit.never_enter(ag.n_vf).to(ag.ctx.device)
    with spy_calls(ag.ctx) as (calls, steps):
        for _ in range(6):
            ag.step_batch()
            twin.step_batch()
    torch.cuda.synchronize()
    assert "scg_step_gated" not in calls and ag.learner_gate is None
    assert_same_bits(ag.state, twin.state, msg="agent.gate set")
    assert torch.equal(ag.W, twin.W) and int((ag.state.option_id > 0).sum()) > 0


def test_learner_gate_refusals():
    ag, _ = _agents(n=64)
    table = gatefit.never_enter(ag.n_vf)
    for bad in (table[:2], table.view(-1), table[:, :1]):
        with pytest.raises(ValueError):
            ag.set_learner_gate(bad)
    for opts in ([0], [ag.n_vf], [-1]):
        with pytest.raises(ValueError):
            ag.set_learner_gate(table, options=opts)
    ag.interrupt_learning = True
    with pytest.raises(ValueError):
        ag.set_learner_gate(table)
    ag.interrupt_learning = False
    ag.set_learner_gate(table)
    ag.interrupt_learning = True
    with pytest.raises(ValueError):
        ag.step_batch()
    ag.interrupt_learning = False
    ag.group = object()                                          # a sharded agent (the check comes before any collective)
    with pytest.raises(ValueError):
        ag.step_batch()
    with pytest.raises(ValueError):
        ag.set_learner_gate(table)
    ag.group = None
    # the context's own checks
    st, W, clf, g = ag.state, ag.W, ag.clf, ag.learner_gate
    for gate, mask in ((g.cpu(), 0b10), (g.double(), 0b10), (g.view(-1), 0b10), (g[:2].contiguous(), 0b10), (None, 0b10),
                       (g, 0b01), (g, 1 << ag.n_vf), (g, -2)):
        with pytest.raises(ScgError):
            ag.ctx.step(st, W, clf, ag.enabled_mask, 0, gate=gate, gate_mask=mask)
    with pytest.raises(ScgError):                                # the library's refusal, through the wrapper
        ag.ctx.step(st, W, clf, ag.enabled_mask, 0, interrupt=True, gate=g, gate_mask=0b10)
