"""Does interruption (SPEC §11) improve the discovered chain's greedy policy? For each map and seed, tools/chain_evidence.py's
protocol trains an agent (warm-up step-batches, chain_skills(), more step-batches); then evaluate() runs the same episodes with
and without interruption and one line each reports success rate, mean return, mean length, and per value function (root
first) the step share, option entries, value-gate declines and interrupts.

Interruption is only guaranteed not to hurt with exact values; these are linear approximations, so the answer is empirical.

    python tools/interrupt_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2 3] [--envs 8192] [--options 5]
"""
import argparse, os
import rig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--episodes", type=int, default=4096, help="episodes of each evaluate()")
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r08_interrupt_report_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# interrupt_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} "
                 f"episodes {a.episodes} hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            ag.rollout(a.warm)
            created = ag.chain_skills(steps_per_option=400, min_examples=3000, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)
            plain = ag.evaluate(n_episodes=a.episodes)
            intr = ag.evaluate(n_episodes=a.episodes, interrupt=True)
            out = [f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}",
                   f"  plain       {rig.fmt_eval(plain)}",
                   f"  interrupt   {rig.fmt_eval(intr)}",
                   "  delta       " + rig.delta_eval(plain, intr)]
            for ln in out:
                print(ln, flush=True)
            lines += out
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r08_interrupt_report_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
