"""µs per acting step-batch: scg_rollout (K steps in one launch, SPEC §8) against K calls of scg_step(flags = 0).

Root + 5 options (chain classifiers, all enabled), bench-like weights (std 1e-3), 4096 and 65 536 envs, K = 64. Each side is
warmed up and synchronised, and the two are timed alternately (rounds of rollout, step loop, rollout, ...); the line per size
gives the median over the rounds.

    python tools/rollout_bench.py [--sizes 4096 65536] [--k 64] [--rounds 7] [--epw 2 4 8 16 32]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import skill_chaining_with_graphs_amd as scg  # noqa: E402
from skill_chaining_with_graphs_amd.core import EnvState, ScgContext  # noqa: E402


def chain_classifiers(m, n_options):
    """Option k's initiation set: a disc round the goal of radius 0.18 + 0.17 (k - 1) (each holds the one before)."""
    clf = np.zeros((n_options + 1, 8), np.float32)
    tx, ty, _ = m.target
    for k in range(1, n_options + 1):
        uc, vc, r = 2 * tx - 1, 2 * ty - 1, 2 * (0.18 + 0.17 * (k - 1))
        clf[k, :6] = [r * r - uc * uc - vc * vc, 2 * uc, 2 * vc, -1.0, 0.0, -1.0]
    return clf


def _state(ctx, m, n, seed=1):
    rng = np.random.default_rng(seed)
    st = EnvState(n, ctx.device, m)
    pos = m.sample_free(n, rng, margin=2.0)
    v = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    for t, a in zip((st.x, st.y, st.vx, st.vy), (pos[:, 0], pos[:, 1], v[:, 0], v[:, 1])):
        t.copy_(torch.as_tensor(np.ascontiguousarray(a, np.float32), device=ctx.device))
    return st


def _time(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def bench(n, k, rounds, n_opt=5, epw=None):
    m = scg.load_map("pinball_simple")
    ctx = ScgContext(n, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000)
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    clf = torch.as_tensor(chain_classifiers(m, n_opt), device=ctx.device).view(-1)
    g = torch.Generator().manual_seed(3)
    W = (torch.randn((n_opt + 1) * 5 * 1296, generator=g) * 1e-3).to(ctx.device)
    st_r, st_s = _state(ctx, m, n), _state(ctx, m, n)
    t = {"r": 0, "s": 0}

    def roll():
        if epw:                                           # pinned launch geometry (envs per wave) instead of scg_rollout's pick
            os.environ["SCG_ROLLOUT_EPW"] = str(epw)
        try:
            ctx.rollout(st_r, W, clf, mask, t["r"], k)
        finally:
            os.environ.pop("SCG_ROLLOUT_EPW", None)
        t["r"] += k

    def loop():
        for _ in range(k):
            ctx.step(st_s, W, clf, mask, t["s"], learn=False)
            t["s"] += 1

    roll(); loop(); roll(); loop()                        # warm-up (first launches, allocator, code objects)
    r_us, s_us = [], []
    for _ in range(rounds):
        r_us.append(_time(roll, 3) * 1e6 / k)
        s_us.append(_time(loop, 3) * 1e6 / k)
    r, s = float(np.median(r_us)), float(np.median(s_us))
    return {"n_envs": n, "k": k, "epw": epw or "auto", "options": n_opt, "rollout_us_per_step": round(r, 2), "step_loop_us_per_step": round(s, 2),
            "speedup": round(s / r, 2), "rollout_rounds_us": [round(v, 2) for v in r_us],
            "step_loop_rounds_us": [round(v, 2) for v in s_us]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epw", type=int, nargs="*", default=None,
                    help="also time the rollout at these pinned launch geometries (envs per wave: 2, 4, 8, 16, 32)")
    a = ap.parse_args()
    for n in a.sizes:
        print(json.dumps(bench(n, a.k, a.rounds)), flush=True)
        for epw in a.epw or []:
            print(json.dumps(bench(n, a.k, a.rounds, epw=epw)), flush=True)


if __name__ == "__main__":
    main()
