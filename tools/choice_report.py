"""Does value-ranked option choice (SPEC §14) improve the greedy policy of a discovered skill tree? For each map and seed,
tools/skill_tree_report.py's protocol trains an agent (warm-up step-batches, grow_skill_tree(), more step-batches); then evaluate()
runs the same episodes with §4.2's lowest-numbered choice and with choose="value", and one line each reports success rate, mean
return, mean length and, per value function (root first), the step share, option entries, value-gate declines and overrides
(entries of an option that was not the lowest-numbered candidate). `offers` is measured on recorded episodes of the first
--record-envs envs under choose="value": the offers made, and the share of them whose candidate set held two or more options.

Discovery may again find a chain, where the rule has nothing to choose from. So each map also gets one hand-set sibling tree on
the first seed's trained weights: five overlapping discs (two lead to the goal, two into the first, one into the second), set
with set_option_parents and evaluated the same way.

    python tools/choice_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--envs 8192] [--options 5]
"""
import argparse, os
import rig

SIBLING_PARENTS = [0, 0, 0, 1, 1, 2]


def sibling_discs(m):
    """(cx, cy, radius) of options 1..5; (tx, ty) the target, s = +-1 pointing from it towards the map centre."""
    tx, ty = float(m.target[0]), float(m.target[1])
    sx, sy = (1.0 if tx < 0.5 else -1.0), (1.0 if ty < 0.5 else -1.0)
    return [(tx, ty, 0.30), (tx + 0.10 * sx, ty + 0.10 * sy, 0.35), (0.5, 0.5, 0.45), (tx, 0.5, 0.50), (0.5, 0.5, 0.75)]


def disc_weights(cx, cy, radius):
    import numpy as np
    uc, vc, r = 2 * cx - 1, 2 * cy - 1, 2 * radius
    w = np.zeros(8, np.float32)
    w[:6] = [r * r - uc * uc - vc * vc, 2 * uc, 2 * vc, -1.0, 0.0, -1.0]
    return w


def offer_shares(ag, traj):
    """(offers, those with |C| >= 2) over a recorded choose="value" evaluation. A row holds s' of its step (the begin row: the
    start state) and the ids written after it; a choice is made on every row that does not keep an option and does not end the
    episode (the begin row always), at that row's position. An offer is a choice with a candidate that is not a stay (§14)."""
    import sys
    import numpy as np
    import torch
    sys.path.append(os.path.join(rig.ROOT, "tests"))
    from option_rules import candidate_mask, membership     # tests/: SPEC §4.2's membership bits and §14's candidate set on the host
    n_vf, mask, parents = ag.n_vf, ag.enabled_mask, [int(p) for p in ag.ctx.parents]
    predict = lambda x, y, k: ag.ctx.classifier_predict(x, y, ag.clf[k].contiguous()).cpu().numpy()
    known = mask | ag.gest_mask
    period = int(ag.ctx.cfg.reoffer_period)
    offers = multi = 0
    for e in range(traj.n):
        r = traj.per_env(e)
        n = len(r["vf"])
        if n == 0:
            continue
        x, y = (torch.as_tensor(r[f], device=ag.W.device) for f in ("x", "y"))
        in_n = membership(predict, x, y, n_vf, known)
        C = candidate_mask(in_n, mask, parents, n_vf)
        j = np.arange(n)
        begin = j == 0
        choice = begin | (((r["vf"] == 0) | (r["term"] != 0)) & (r["done"] == 0))
        prev = np.concatenate([[0], r["option_id"][:-1].astype(np.int64)])
        member = (prev < 0) & (-prev < n_vf) & C[np.clip(-prev, 0, n_vf - 1), j]
        stay = choice & ~begin & member & (((j + e) % period) != 0)      # (row j is step counter j, env e its global id)
        offer = choice & C.any(axis=0) & ~stay
        offers += int(offer.sum())
        multi += int((offer & (C.sum(axis=0) >= 2)).sum())
    return offers, multi


def compare(ag, episodes, record_envs):
    plain = ag.evaluate(n_episodes=episodes)
    value = ag.evaluate(n_episodes=episodes, choose="value")
    traj, _ = ag.record_episodes(n_episodes=record_envs, choose="value")
    offers, multi = offer_shares(ag, traj)
    return [f"  lowest      {rig.fmt_eval(plain)}",
            f"  value       {rig.fmt_eval(value)} overrides {value['overrides']}",
            f"  offers      {offers} on {record_envs} recorded episodes, {multi} with two or more candidates "
            f"({multi / offers if offers else float('nan'):.3f})",
            "  delta       " + rig.delta_eval(plain, value)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400)
    ap.add_argument("--episodes", type=int, default=4096, help="episodes of each evaluate()")
    ap.add_argument("--record-envs", type=int, default=256, help="recorded episodes the offers are counted on")
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r11_choice_report_<map>.txt")
    a = ap.parse_args()
    import torch
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)
    TOTAL = a.warm + a.options * a.steps_per_option + a.after
    DISCOVERY = dict(steps_per_option=a.steps_per_option, min_examples=3000, max_examples=40000, start_coverage=0.9)

    for mp in a.maps:
        lines = [f"# choice_report map {mp} envs {a.envs} options {a.options} warm {a.warm} step-batches {TOTAL} episodes {a.episodes} "
                 f"discovery {DISCOVERY} hparams {HP}"]
        print(lines[0], flush=True)
        for i, seed in enumerate(a.seeds):
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            ag.rollout(a.warm)
            created = ag.grow_skill_tree(**DISCOVERY)
            ag.rollout(TOTAL - ag.t)
            out = [f"seed {seed} discovered: {len(created)} options, enabled mask {ag.enabled_mask:#x}, parents "
                   f"{[int(p) for p in ag.ctx.parents]}"] + compare(ag, a.episodes, a.record_envs)
            if i == 0 and a.options == 5:
                # the hand-set sibling tree on this agent's trained weights: every option starts from the root's, as a new option does
                ag.set_option_parents(SIBLING_PARENTS)
                for k, disc in enumerate(sibling_discs(ag.map), start=1):
                    ag.clf[k].copy_(torch.as_tensor(disc_weights(*disc)))
                    ag.enable_option(k)
                W = ag.W.view(ag.n_vf, -1)
                g = torch.Generator().manual_seed(seed)
                scale = float(W[0].abs().mean())
                W[1:] = W[0] + (scale * 0.05 * torch.randn(W[1:].shape, generator=g)).to(W.device)
                out += [f"seed {seed} hand-set sibling tree: parents {SIBLING_PARENTS}, discs {sibling_discs(ag.map)}, option weights = "
                        f"the root's + noise of 5 % of its mean magnitude"] + compare(ag, a.episodes, a.record_envs)
            for ln in out:
                print(ln, flush=True)
            lines += out
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r11_choice_report_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
