"""The peer transport of the order-pinned sum (include/scg_abi.h "peer transport"), host side only: the new entry points
are exported by every build, the new status bit decodes, and the Python layer refuses what the transport cannot serve before it
touches a device. The exchange itself runs on the GPU: tests/test_gpu_peer_exchange.py."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEER_SYMBOLS = ("scg_peer_export", "scg_peer_open", "scg_peer_exchange_apply", "scg_set_peer_timeout")
CSRC = os.path.join(ROOT, "skill-chaining-with-graphs_amd", "csrc")


def test_every_library_build_exports_the_peer_entry_points(pkg):
    from skill_chaining_with_graphs_amd import _lib
    for b in _lib.BLOCK_ENVS_BUILDS:
        lib = _lib.load(b)
        for name in PEER_SYMBOLS:
            assert hasattr(lib, name), (b, name)
    fi = os.path.join(CSRC, "libscg_hip_faultinj.so")          # the fault-injection build the void test pairs with the product
    if os.path.exists(fi):
        lib = C.CDLL(fi)
        for name in PEER_SYMBOLS:
            assert hasattr(lib, name), ("faultinj", name)
    assert set(PEER_SYMBOLS) <= set(pkg.EXPORTED_SYMBOLS)


def test_peer_entry_points_check_their_arguments_without_a_device(pkg):
    lib = pkg.load_library()
    h = C.create_string_buffer(64)
    assert lib.scg_peer_export(None, h) == -1 and b"null" in lib.scg_last_error(None)
    assert lib.scg_peer_open(None, 2, 0, h) == -1
    assert lib.scg_peer_exchange_apply(None, None, None) == -1
    assert lib.scg_set_peer_timeout(None, C.c_double(1.0)) == -1


def test_peer_timeout_bit_decodes(pkg):
    from skill_chaining_with_graphs_amd import _lib
    lib = pkg.load_library()
    buf = C.create_string_buffer(256)
    assert _lib.ASYNC_PEER_TIMEOUT == 0x4
    rc = lib.scg_decode_async_word(0x4, buf, 256)
    assert rc == -5 and b"scg_peer_exchange_apply" in buf.value and b"peer wait" in buf.value and b"unchanged" in buf.value
    assert lib.scg_decode_async_word(0x4 | 0x2, buf, 256) == -5 and b"scg_step" in buf.value      # a void step is named first
    assert lib.scg_decode_async_word(0x80000000, buf, 256) == -5 and b"unknown" in buf.value


@pytest.mark.parametrize("kw", [dict(), dict(ordered_sum=True), dict(group=object()), dict(group=object(), ordered_sum=False)])
def test_peer_transport_needs_a_group_and_the_ordered_sum(pkg, kw, monkeypatch):
    from skill_chaining_with_graphs_amd import agent
    touched = []
    monkeypatch.setattr(agent, "ScgContext", lambda *a, **k: touched.append(1))
    monkeypatch.setattr(agent._dist, "allreduce_max_int", lambda *a, **k: touched.append(1))
    with pytest.raises(ValueError, match="transport='peer' needs group"):
        agent.SkillChainingAgent("pinball_simple", 64, 1, transport="peer", **kw)
    with pytest.raises(ValueError, match="transport must be"):
        agent.SkillChainingAgent("pinball_simple", 64, 1, transport="rccl")
    assert not touched


def _info(host="h", dev_id="gpu0", grid=10):
    return {"handle": b"\0" * 64, "host": host, "device": 0, "device_id": dev_id, "grid": grid}


def test_grid_budget_on_one_device():
    from skill_chaining_with_graphs_amd import auto_block_envs
    from skill_chaining_with_graphs_amd.dist import check_peer_layout
    g = -(-65536 // auto_block_envs(65536))                    # 256 workgroups per rank
    with pytest.raises(ValueError, match="below 256"):
        check_peer_layout([_info(grid=g), _info(grid=g)])
    with pytest.raises(ValueError, match="below 256"):
        check_peer_layout([_info(grid=128), _info(grid=128)])
    check_peer_layout([_info(grid=120), _info(grid=120)])                       # 2 x 30 720 envs at 256 per block
    check_peer_layout([_info(grid=g, dev_id="gpu0"), _info(grid=g, dev_id="gpu1")])    # one GPU each: no limit
    check_peer_layout([_info(grid=g)])                                           # one rank: nothing shares its GPU


def _gloo_rank(rank, world, port, hosts, out_dir):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import socket
    import torch.distributed as dist
    from skill_chaining_with_graphs_amd import dist as sdist
    socket.gethostname = lambda: hosts[rank]                   # faked host names

    class FakeCtx:                                             # exchange_peer_handles' view of a context (no device)
        device = torch.device("cpu")
        step_grid = 4
        opened = None

        def peer_export(self):
            return bytes([rank]) * 64

        def peer_open(self, n, r, handles):
            self.opened = (n, r, handles)

    dist.init_process_group("gloo", rank=rank, world_size=world)
    ctx = FakeCtx()
    try:
        sdist.exchange_peer_handles(ctx, dist.group.WORLD)
        res = "opened" if ctx.opened == (world, rank, [bytes([r]) * 64 for r in range(world)]) else f"bad {ctx.opened!r}"
    except ValueError as e:
        res = f"refused: {e}"
    with open(os.path.join(out_dir, f"r{rank}.txt"), "w") as f:
        f.write(res)
    dist.destroy_process_group()


@pytest.mark.parametrize("hosts,expect", [(("a", "a"), "opened"), (("a", "b"), "refused: transport='peer' needs every rank on one host")])
def test_exchange_peer_handles_over_gloo(tmp_path, hosts, expect):
    import torch.multiprocessing as mp
    port = 29500 + (os.getpid() + len(set(hosts))) % 150
    mp.spawn(_gloo_rank, args=(2, port, hosts, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        assert (tmp_path / f"r{r}.txt").read_text().startswith(expect)


def test_exchange_peer_handles_refuses_a_world_above_eight(tmp_path, monkeypatch):
    import torch.distributed as dist
    from skill_chaining_with_graphs_amd import dist as sdist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 9)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)

    class NoCtx:
        def peer_export(self):
            raise AssertionError("exported before the world size was checked")

    with pytest.raises(ValueError, match="at most 8 ranks"):
        sdist.exchange_peer_handles(NoCtx(), None)
    with pytest.raises(ValueError, match="at most 8 ranks"):
        sdist.check_peer_layout([_info(dev_id=f"gpu{r}") for r in range(9)])
