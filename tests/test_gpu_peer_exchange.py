"""The peer transport of the order-pinned sum (SkillChainingAgent(group=..., ordered_sum=True, transport="peer")) on ONE
GPU: rank processes on cuda:0 map each other's operands through HIP IPC, and each sums them in rank order on the device. Held bit
for bit to the collective transport (all-gather + scg_apply_update_slots) in the same processes and to the oracle's shards summed in
rank order. Six or more exchanges per run reuse each parity buffer at least twice (a stale read of exchange e - 2 would show).
gloo carries only the one-off handle exchange and the collective twin; at most 3 rank processes hold the GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import sc_oracle
from util import HP, SCALE, chain_classifiers, oracle_block, random_states, random_weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 17


def _rank_setup(rank, world, port):
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    return dist


def _agent(m, n, n_opt, rank, world, transport, W0, states, mask, **kw):
    import torch.distributed as dist
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    ag = SkillChainingAgent(m, n, n_opt, device=0, seed=SEED, env_id_base=rank * n, group=dist.group.WORLD, ordered_sum=True,
                            transport=transport, **kw)
    sl = slice(rank * n, (rank + 1) * n)
    for name, v in zip(("x", "y", "vx", "vy"), states):
        getattr(ag.state, name).copy_(torch.as_tensor(v[sl].copy(), device="cuda:0"))
    ag.clf.copy_(torch.as_tensor(chain_classifiers(m, n_opt), device="cuda:0"))
    ag.enabled_mask = mask
    ag.W.copy_(torch.as_tensor(W0, device="cuda:0"))
    return ag


def _rank_main_small(rank, world, port, out_dir, block_envs, steps):
    dist = _rank_setup(rank, world, port)
    import skill_chaining_with_graphs_amd as scg
    m = scg.load_map("pinball_simple")
    n, n_opt = 300, 2
    states = random_states(m, world * n, 77, vmax=1.0)
    kw = dict(HP)
    if block_envs:
        kw["block_envs"] = block_envs
    W0 = random_weights(n_opt + 1, 4, std=0.05)
    peer = _agent(m, n, n_opt, rank, world, "peer", W0, states, 0b110, **kw)
    coll = _agent(m, n, n_opt, rank, world, "collective", W0, states, 0b110, **kw)
    assert peer.ctx.block_envs == coll.ctx.block_envs == (block_envs or 256)
    Ws = []
    for _ in range(steps):
        peer.step_batch()
        coll.step_batch()
        Ws.append(peer.W.cpu().numpy())
    torch.cuda.synchronize()
    assert peer.ctx.async_status(synchronize=True) == 0
    np.savez(os.path.join(out_dir, f"small{rank}.npz"), W=np.stack(Ws), x=peer.state.x.cpu().numpy(),
             W_coll=coll.W.cpu().numpy(), x_coll=coll.state.x.cpu().numpy(),
             opt=peer.state.option_id.cpu().numpy(), opt_coll=coll.state.option_id.cpu().numpy())
    dist.barrier()                                  # no rank frees its region while a peer may still read it
    dist.destroy_process_group()


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("block_envs", [None, 64])
def test_peer_transport_equals_the_collective_and_the_oracle(tmp_path, R, block_envs):
    import torch.multiprocessing as mp
    n, n_opt, steps = 300, 2, 7
    port = 29300 + (os.getpid() + 7 * R + (block_envs or 0)) % 190
    mp.spawn(_rank_main_small, args=(R, port, str(tmp_path), block_envs, steps), nprocs=R, join=True)
    res = [np.load(tmp_path / f"small{r}.npz") for r in range(R)]
    for r in range(R):
        assert np.array_equal(res[r]["W"], res[0]["W"]), f"rank {r}: weights differ from rank 0's"
        assert np.array_equal(res[r]["W_coll"], res[r]["W"][-1]), f"rank {r}: peer and collective transports differ"
        assert np.array_equal(res[r]["x"], res[r]["x_coll"]) and np.array_equal(res[r]["opt"], res[r]["opt_coll"])
    import skill_chaining_with_graphs_amd as scg
    m = scg.load_map("pinball_simple")
    with oracle_block(block_envs or 256):
        x, y, vx, vy = random_states(m, R * n, 77, vmax=1.0)
        clf = chain_classifiers(m, n_opt)
        W_o = random_weights(n_opt + 1, 4, std=0.05)
        orcs, sts = [], []
        for r in range(R):
            orcs.append(sc_oracle.Oracle(m, SCALE, n_envs=n, n_options=n_opt, seed=SEED, env_id_base=r * n, enabled_mask=0b110,
                                         n_threads=4, **HP))
            st = sc_oracle.new_state(n, m)
            sl = slice(r * n, (r + 1) * n)
            st["x"][:], st["y"][:], st["vx"][:], st["vy"][:] = x[sl], y[sl], vx[sl], vy[sl]
            sts.append(st)
        for t in range(steps):
            out = [orcs[r].step(sts[r], W_o, clf, t) for r in range(R)]
            g_sum, n_sum = out[0][0].copy(), out[0][1].copy()
            for r in range(1, R):
                g_sum = (g_sum + out[r][0]).astype(np.float32)          # float32 additions in rank order
                n_sum = n_sum + out[r][1]
            orcs[0].apply(W_o, g_sum, n_sum)
            assert np.array_equal(res[0]["W"][t], W_o), f"weights differ from the oracle's {R} shards at step {t}"
        for r in range(R):
            assert np.array_equal(res[r]["x"], sts[r]["x"])


def _rank_main_long(rank, world, port, out_dir, steps):
    dist = _rank_setup(rank, world, port)
    import skill_chaining_with_graphs_amd as scg
    m = scg.load_map("pinball_simple")
    n, n_opt = 8192, 5
    states = random_states(m, world * n, 5, vmax=1.0)
    W0 = random_weights(n_opt + 1, 6, std=0.05)
    peer = _agent(m, n, n_opt, rank, world, "peer", W0, states, 0b111110)
    coll = _agent(m, n, n_opt, rank, world, "collective", W0, states, 0b111110)
    for _ in range(steps):
        peer.step_batch()
        coll.step_batch()
    torch.cuda.synchronize()
    assert peer.ctx.async_status(synchronize=True) == 0
    keys = ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "qcache")
    np.savez(os.path.join(out_dir, f"long{rank}.npz"), W=peer.W.cpu().numpy(), W_coll=coll.W.cpu().numpy(),
             **{k: getattr(peer.state, k).cpu().numpy() for k in keys}, **{k + "_c": getattr(coll.state, k).cpu().numpy() for k in keys})
    dist.barrier()
    dist.destroy_process_group()


def test_peer_transport_long_run_at_the_headline_mix(tmp_path):
    """2 ranks x 8192 envs, 5 options, 20 learning step-batches: the peer transport ends where the collective one does."""
    import torch.multiprocessing as mp
    port = 29500 + os.getpid() % 190
    mp.spawn(_rank_main_long, args=(2, port, str(tmp_path), 20), nprocs=2, join=True)
    res = [np.load(tmp_path / f"long{r}.npz") for r in range(2)]
    assert np.array_equal(res[0]["W"], res[1]["W"])
    assert not np.array_equal(res[0]["W"], random_weights(6, 6, std=0.05))          # it learned something
    for r in range(2):
        assert np.array_equal(res[r]["W"], res[r]["W_coll"]), f"rank {r}: weights differ from the collective transport"
        for k in ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "qcache"):
            assert np.array_equal(res[r][k], res[r][k + "_c"]), f"rank {r}: {k} differs from the collective transport"


def _rank_main_void(rank, world, port, out_dir, fi_path):
    dist = _rank_setup(rank, world, port)
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd import ScgError
    m = scg.load_map("pinball_simple")
    n, T = 1024, 0x7e57                                  # (the injected fault needs a second block on the faulting rank)
    states = random_states(m, world * n, 5, vmax=1.0)
    kw = dict(HP, block_envs=256)
    if rank == 1:
        kw["library"] = fi_path                          # drops one hand-off of the step at t = 0x7e57, on this rank only
    ag = _agent(m, n, 1, rank, world, "peer", random_weights(2, 7, std=0.05), states, 0b10, **kw)
    ag.t = T - 2
    ag.step_batch(); ag.step_batch()
    torch.cuda.synchronize()
    assert ag.ctx.async_status(synchronize=True) == 0
    W_before = ag.W.clone()
    try:
        ag.step_batch()                                  # step t = T: void on rank 1
    except ScgError:
        pass                                             # (rank 1's exchange may already see its own failure: launched anyway)
    msg = ""
    try:
        ag.ctx.async_status(synchronize=True)
    except ScgError as e:
        msg = str(e)
    np.savez(os.path.join(out_dir, f"void{rank}.npz"), unchanged=np.array([bool(torch.equal(ag.W, W_before))]),
             msg=np.array([msg]), changed_before=np.array([not np.array_equal(W_before.cpu().numpy(), random_weights(2, 7, std=0.05))]))
    dist.barrier()
    dist.destroy_process_group()


def test_a_void_step_on_one_rank_leaves_the_weights_of_every_rank(tmp_path):
    import torch.multiprocessing as mp
    import skill_chaining_with_graphs_amd as scg
    fi = os.path.join(os.path.dirname(scg.LIB_PATH), "libscg_hip_faultinj.so")
    if not os.path.exists(fi):
        pytest.skip("fault-injection build missing (make -C skill-chaining-with-graphs_amd/csrc faultinj)")
    port = 29700 + os.getpid() % 190
    mp.spawn(_rank_main_void, args=(2, port, str(tmp_path), fi), nprocs=2, join=True)
    for r in range(2):
        res = np.load(tmp_path / f"void{r}.npz")
        assert bool(res["changed_before"][0]), f"rank {r}: the steps before the void one did not learn"
        assert bool(res["unchanged"][0]), f"rank {r}: a voided exchange touched W"
        assert "scg_step" in str(res["msg"][0]) and "an earlier launch failed" in str(res["msg"][0]), (r, str(res["msg"][0]))


def test_the_peer_wait_is_bounded_and_the_next_exchange_succeeds():
    """One process, two contexts as ranks 0 and 1 of one peer group (rank 1's region is found in-process). Rank 0 exchanges first
    while rank 1 has published nothing: the bounded wait gives up (SCG_ASYNC_PEER_TIMEOUT), W stays. After clearing, rank 1 makes
    exchange 0 and then both make exchange 1 concurrently (two streams): every weight equals the collective form's
    (grad_packed + apply_update_slots) on twin contexts. This is the designed status path of a bounded poll, not a fault."""
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd import ScgError
    from skill_chaining_with_graphs_amd.core import EnvState, ScgContext
    m = scg.load_map("pinball_simple")
    n, n_opt, mask = 300, 2, 0b110
    states = random_states(m, 2 * n, 77, vmax=1.0)
    clf = torch.as_tensor(chain_classifiers(m, n_opt), device="cuda:0").view(-1)
    W0 = random_weights(n_opt + 1, 4, std=0.05)

    def make(r):
        ctx = ScgContext(n, n_opt, m, seed=SEED, env_id_base=r * n, **HP)
        st = EnvState(n, ctx.device, m)
        for name, v in zip(("x", "y", "vx", "vy"), states):
            getattr(st, name).copy_(torch.as_tensor(v[r * n:(r + 1) * n].copy(), device="cuda:0"))
        return ctx, st, torch.as_tensor(W0, device="cuda:0").reshape(-1).clone()

    (A, stA, WA), (B, stB, WB) = make(0), make(1)
    hs = [A.peer_export(), B.peer_export()]
    assert B.peer_export() == hs[1]                                        # one region per context
    A.peer_open(2, 0, hs)
    B.peer_open(2, 1, hs)
    A.set_peer_timeout(0.05)
    A.step(stA, WA, clf, mask, 0, apply=False)
    WA_0 = WA.clone()
    A.peer_exchange_apply(WA)                                              # returns at once
    with pytest.raises(ScgError, match="peer wait"):
        A.async_status(synchronize=True)
    assert torch.equal(WA, WA_0), "a timed-out exchange touched W"
    A.clear_async_error()
    sB = torch.cuda.Stream()
    sB.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(sB):
        B.step(stB, WB, clf, mask, 0, apply=False)
        B.peer_exchange_apply(WB)                                          # rank 0 published exchange 0 already
    A.step(stA, WA, clf, mask, 1, apply=False)
    A.peer_exchange_apply(WA)                                              # waits for rank 1's exchange 1 ...
    with torch.cuda.stream(sB):
        B.step(stB, WB, clf, mask, 1, apply=False)                         # ... which runs on the other stream meanwhile
        B.peer_exchange_apply(WB)
    torch.cuda.synchronize()
    assert A.async_status(synchronize=True) == 0 and B.async_status(synchronize=True) == 0
    # the same history through the collective form
    (A2, stA2, WA2), (B2, stB2, WB2) = make(0), make(1)
    gA, gB = A2.grad_packed(), B2.grad_packed()
    A2.step(stA2, WA2, clf, mask, 0, apply=False); gA0 = gA.clone()
    B2.step(stB2, WB2, clf, mask, 0, apply=False); gB0 = gB.clone()
    B2.apply_update_slots(WB2, torch.stack([gA0, gB0]).contiguous())
    A2.step(stA2, WA2, clf, mask, 1, apply=False); gA1 = gA.clone()
    B2.step(stB2, WB2, clf, mask, 1, apply=False); gB1 = gB.clone()
    slots1 = torch.stack([gA1, gB1]).contiguous()
    A2.apply_update_slots(WA2, slots1)
    B2.apply_update_slots(WB2, slots1)
    torch.cuda.synchronize()
    assert not torch.equal(WA, WA_0)
    assert torch.equal(WA, WA2) and torch.equal(WB, WB2)
    for ctx in (A2, B2, A, B):                                             # B's region outlives A's reads of it
        ctx.close()
