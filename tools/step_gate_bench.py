"""µs per learning step-batch: scg_step(LEARN | APPLY) against scg_step_gated(LEARN | APPLY) with every enabled option in the mask
(SPEC §26: one more launch, step_gate_kernel, between the step kernel and the reduce launch).

Root + 5 options, 4096 and 65 536 envs, on two workloads: `synthetic`, bench.py's (chain classifiers, every option enabled, W of
std 1e-3, random states), and `chain`, a discovered chain as tools/gate_learning_report.py trains it (warm-up, chain_skills(), more
step-batches; --chain-envs envs, its tables then seated on a context of the size timed), whose offer rate is what that report's
learners see. The table is the shipped gate of the W at the start: what the kernel does depends on the number of offers, not on
the table's values. Each side has its own state and weights, is warmed up, and the two are timed alternately in rounds of K
step-batches; the line per workload and size gives each side's median and min - max over the rounds, their ratio, and the offers
per env-step the gated side saw afterwards.

    python tools/step_gate_bench.py [--sizes 4096 65536] [--workloads synthetic chain] [--k 64] [--rounds 9] [--out FILE]
"""
import argparse
import json

import rig


def _clone(st):
    from skill_chaining_with_graphs_amd.core import EnvState
    c = object.__new__(EnvState)
    c.n = st.n
    for f in EnvState.FIELDS:
        setattr(c, f, getattr(st, f).clone())
    return c


def _chain_tables(a):
    """(map name, W, clf, enabled mask, parents, hyper-parameters) of a trained chain."""
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    hp = rig.discovery_hp(a.chain_envs)
    ag = SkillChainingAgent("pinball_simple", a.chain_envs, 5, seed=1, **hp)
    ag.enable_tracing(64)
    ag.rollout(3000)
    ag.chain_skills(steps_per_option=400, min_examples=3000, max_examples=40000, start_coverage=0.9)
    ag.rollout(1000)
    return ag.W.clone(), ag.clf.clone(), ag.enabled_mask, [int(v) for v in ag.ctx.parents], hp


def bench(workload, n, k, rounds, chain=None, n_opt=5):
    import numpy as np
    import torch
    from skill_chaining_with_graphs_amd import gatefit
    if workload == "synthetic":
        ag = rig.headline_agent(envs=n, options=n_opt)
    else:
        from skill_chaining_with_graphs_amd import SkillChainingAgent
        W, clf, enabled, parents, hp = chain
        ag = SkillChainingAgent("pinball_simple", n, n_opt, seed=1, **dict(hp, update_count_floor=n // 16))
        ag.W.copy_(W); ag.clf.copy_(clf)
        ag.enabled_mask = enabled
        ag.ctx.set_option_parents(parents)
        ag.domain.reset_random(seed=1000, v_max=1.0)
        ag.rollout(200)                                       # the envs spread over the episode
    torch.cuda.synchronize()
    ctx, mask = ag.ctx, ag.enabled_mask
    clf = ag.clf.view(-1)
    gate = gatefit.shipped_gate(ag.W).contiguous()
    sides = {name: {"st": _clone(ag.state), "W": ag.W.clone().view(-1), "t": int(ag.t), "mask": mask if name == "gated" else 0}
             for name in ("plain", "gated")}

    def run(s, steps=k):
        for _ in range(steps):
            ctx.step(s["st"], s["W"], clf, mask, s["t"], learn=True, apply=True, gate=gate, gate_mask=s["mask"])
            s["t"] += 1

    for s in sides.values():                                  # warm-up (first launches, allocator, code objects)
        run(s); run(s)
    us = {name: [] for name in sides}
    for _ in range(rounds):
        for name, s in sides.items():
            us[name].append(rig.timed(lambda: run(s), 1) * 1e6 / k)
    s, offers, steps = sides["gated"], 0, 32
    env = torch.arange(n, device=ctx.device, dtype=torch.int64)
    for _ in range(steps):                                    # offers = entries + fresh declines (a stay is no offer)
        prev, t = s["st"].option_id.clone(), s["t"]
        run(s, 1)
        now = s["st"].option_id
        due = ((env + t) % max(int(ctx.cfg.reoffer_period), 1)) == 0
        offers += int((((now > 0) & (now != prev)) | ((now < 0) & ((now != prev) | due | (s["st"].done != 0)))).sum())
    out = {"workload": workload, "n_envs": n, "k": k, "options": n_opt, "enabled_mask": mask}
    for name in sides:
        out[f"{name}_us_per_step"] = round(float(np.median(us[name])), 2)
        out[f"{name}_min_max_us"] = [round(min(us[name]), 2), round(max(us[name]), 2)]
    out["gated_over_plain"] = round(out["gated_us_per_step"] / out["plain_us_per_step"], 4)
    out["offers_per_env_step"] = round(offers / (steps * n), 4)
    out["option_running_share"] = round(float((s["st"].option_id > 0).float().mean()), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--workloads", nargs="+", default=["synthetic", "chain"])
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--chain-envs", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    chain = _chain_tables(a) if "chain" in a.workloads else None
    lines = []
    for w in a.workloads:
        for n in a.sizes:
            lines.append(json.dumps(bench(w, n, a.k, a.rounds, chain)))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
