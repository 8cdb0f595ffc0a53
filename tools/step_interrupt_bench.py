"""µs per learning step-batch: scg_step(LEARN | APPLY) against scg_step(LEARN | APPLY | INTERRUPT) (SPEC §12).

Root + 5 options (chain classifiers, all enabled), bench-like weights (std 1e-3), 4096 and 65 536 envs. Each side has its own
state and weights, is warmed up, and the two are timed alternately in rounds of K step-batches; the line per size gives the
medians over the rounds and, per side, the share of envs running an option at the end.

    python tools/step_interrupt_bench.py [--sizes 4096 65536] [--k 64] [--rounds 7]
"""
import argparse
import json

import rig


def bench(n, k, rounds, n_opt=5):
    import numpy as np
    import torch
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd.core import ScgContext
    m = scg.load_map("pinball_simple")
    ctx = ScgContext(n, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000)
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    clf = torch.as_tensor(rig.chain_classifiers(m, n_opt), device=ctx.device).view(-1)
    g = torch.Generator().manual_seed(3)
    W0 = (torch.randn((n_opt + 1) * 5 * 1296, generator=g) * 1e-3).to(ctx.device)
    sides = {name: {"st": rig.state_on(ctx, m, n), "W": W0.clone(), "t": 0, "int": name == "interrupt"} for name in ("plain", "interrupt")}

    def run(s):
        for _ in range(k):
            ctx.step(s["st"], s["W"], clf, mask, s["t"], learn=True, apply=True, interrupt=s["int"])
            s["t"] += 1

    for s in sides.values():                              # warm-up (first launches, allocator, code objects)
        run(s); run(s)
    us = {name: [] for name in sides}
    for _ in range(rounds):
        for name, s in sides.items():
            us[name].append(rig.timed(lambda: run(s), 1) * 1e6 / k)
    out = {"n_envs": n, "k": k, "options": n_opt}
    for name in sides:
        out[f"{name}_us_per_step"] = round(float(np.median(us[name])), 2)
        out[f"{name}_rounds_us"] = [round(v, 2) for v in us[name]]
    out["interrupt_cost_pct"] = round(100.0 * (out["interrupt_us_per_step"] / out["plain_us_per_step"] - 1.0), 1)
    out["option_running_share"] = {name: round(float((sides[name]["st"].option_id > 0).float().mean()), 4) for name in sides}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    for n in a.sizes:
        print(json.dumps(bench(n, a.k, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
