"""Shared-weights rehearsal on ONE GPU: R rank processes step the order-pinned shared-weights agent over the two transports,
transport="collective" (gloo all-gather through the host + scg_apply_update_slots) and transport="peer" (HIP IPC, the rank-order
sum on the device), at the same sizes. Prints one JSON line: env-steps/s over all ranks and the exchange as the step's
stream sees it (an event pair round the exchange call of every timed step-batch, rank 0).

    python tools/peer_rehearsal.py [--ranks 2] [--envs 30720] [--options 5] [--steps 200] [--warmup 20] [--transports collective,peer]

The launcher starts the R rank processes before anything has touched the GPU, each under its own `timeout -k`, and touches no
GPU itself."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rank_main(args):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = scg.load_map("pinball_simple")
    out = {}
    for transport in args.transports.split(","):
        ag = SkillChainingAgent(m, args.envs, args.options, device=0, seed=1, env_id_base=rank * args.envs, group=dist.group.WORLD,
                                ordered_sum=True, transport=transport, block_envs=args.block_envs)
        ag.domain.reset_random(seed=3 + rank, v_max=0.5)
        ag.init_weights(seed=2)
        ag.enabled_mask = 0
        for _ in range(args.warmup):
            ag.step_batch()
        torch.cuda.synchronize()
        dist.barrier()
        ag.time_allreduce(1)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ag.step_batch()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ex = ag.time_allreduce(0)
        ag.ctx.async_status(synchronize=True)
        dist.barrier()                                    # every rank done with the peers' regions before any is freed
        out[transport] = {"env_steps_per_s": world * args.envs * args.steps / dt, "step_us": dt / args.steps * 1e6,
                          "exchange_mean_us": ex["mean_us"], "exchange_max_us": ex["max_us"]}
        del ag
    if rank == 0:
        print("RESULT " + json.dumps(out), flush=True)
    dist.destroy_process_group()


def launch(args):
    port = 29400 + os.getpid() % 500
    procs = []
    for r in range(args.ranks):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(args.ranks), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True))
    outs = [p.communicate()[0] for p in procs]
    rcs = [p.returncode for p in procs]
    res = None
    for line in outs[0].splitlines():
        if line.startswith("RESULT "):
            res = json.loads(line[7:])
    rec = {"tool": "peer_rehearsal", "ranks": args.ranks, "envs_per_rank": args.envs, "options": args.options,
           "steps": args.steps, "warmup": args.warmup, "block_envs": args.block_envs, "one_gpu": True,
           "exit_codes": rcs, "result": res}
    print(json.dumps(rec))
    return 0 if res is not None and not any(rcs) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--envs", type=int, default=30720)
    ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--block-envs", type=int, default=256)
    ap.add_argument("--transports", default="collective,peer")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each rank process may run")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        rank_main(args)
        return 0
    return launch(args)


if __name__ == "__main__":
    sys.exit(main())
