"""Cost of SPEC §13's frontier collection (scg_collect_frontier) against §7's two-launch scg_collect_examples, on one trace.

An agent of --envs envs with all five options enabled (five separate discs of radius 0.1, so that every node sees entries) runs
--warm step-batches with tracing on; then, on that one trace, every collector is called --reps times, alternating, each call
bracketed by its own event pair on the stream (the fill levels are reset outside the pairs, so every call appends the same rows):
  frontier_all   target = every node (goal + 5 options), cover = every option
  frontier_goal  target = the goal, cover = every option
  examples_goal  scg_collect_examples(bits = goal, no prev_in), not announced (two launches)
  examples_set1  scg_collect_examples(bits = set 1, prev_in), not announced (two launches)
Prints one JSON line. Kernel times without the event overhead: run it under rocprofv3 --kernel-trace --stats.

    python tools/frontier_cost.py [--envs 65536] [--warm 64] [--reps 200]
"""
import argparse
import json

import rig  # noqa: F401  (puts the repository root on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--map", default="pinball_simple")
    a = ap.parse_args()
    import numpy as np
    import torch
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    ag = SkillChainingAgent(a.map, a.envs, 5, seed=1)
    ag.enable_tracing(64)
    for k, (cx, cy) in enumerate([(0.2, 0.2), (0.5, 0.5), (0.2, 0.8), (0.8, 0.8), (0.5, 0.15)], start=1):
        ag.options[k].initiation_classifier.set_disc(cx, cy, 0.1)       # five separate sets: every node sees entries
        ag.enable_option(k)
    ag.init_weights(std=1e-3, seed=2)
    ag.domain.reset_random(seed=3, v_max=1.0)
    for _ in range(a.warm):
        ag.step_batch()
    ctx, dev, n_vf, cap = ag.ctx, ag.W.device, 6, 1 << 20
    xy = torch.zeros((n_vf, cap, 2), dtype=torch.float32, device=dev)
    lab = torch.zeros((n_vf, cap), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(n_vf, dtype=torch.int32, device=dev)
    exy, elab = torch.zeros((cap, 2), device=dev), torch.zeros(cap, dtype=torch.uint8, device=dev)
    ecnt, prev = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(a.envs, dtype=torch.uint8, device=dev)
    clf = ag.clf.view(-1)
    calls = {
        "frontier_all": lambda: ctx.collect_frontier(0b111111, 0b111110, clf, 24, 24, xy.view(-1), lab.view(-1), cnt),
        "frontier_goal": lambda: ctx.collect_frontier(0b1, 0b111110, clf, 24, 24, xy.view(-1), lab.view(-1), cnt),
        "examples_goal": lambda: ctx.collect_examples(1, None, 24, 24, exy.view(-1), elab, ecnt, rearm=False),
        "examples_set1": lambda: ctx.collect_examples(2, prev, 24, 24, exy.view(-1), elab, ecnt, rearm=False),
    }
    rows = {}
    for name, fn in calls.items():                     # warm-up, and the rows each call appends
        cnt.zero_(); ecnt.zero_(); prev.zero_()
        fn()
        torch.cuda.synchronize()
        rows[name] = cnt.tolist() if name.startswith("frontier") else int(ecnt.item())
    ev = {name: [] for name in calls}
    for _ in range(a.reps):
        for name, fn in calls.items():
            cnt.zero_(); ecnt.zero_(); prev.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            ev[name].append((e0, e1))
    torch.cuda.synchronize()
    out = {"envs": a.envs, "map": a.map, "warm": a.warm, "reps": a.reps, "device": torch.cuda.get_device_name(0), "rows": rows}
    for name, pairs in ev.items():
        t = np.array([x.elapsed_time(y) * 1e3 for x, y in pairs])
        out[name + "_us"] = {"median": round(float(np.median(t)), 2), "p10": round(float(np.percentile(t, 10)), 2),
                             "p90": round(float(np.percentile(t, 90)), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
