"""Does a learner that interrupts (SPEC §12) learn better chains? For each map and seed, two agents are trained with
tools/interrupt_report.py's protocol (warm-up step-batches, chain_skills(), more step-batches), one with the plain learning
rule and one with interrupt_learning=True (chain_skills' step-batches included). Both stop at the same env-step count: the
step-batches chain_skills() did not use are added to the last phase. Each learner's greedy policy is then evaluated on the
same episodes with and without interruption (SPEC §11); one line each reports success rate, mean return, mean length and,
per value function (root first), the step share, option entries, value-gate declines and (acting with interruption) interrupts.

    python tools/interrupt_learning_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--envs 8192] [--options 5]
"""
import argparse, os, time
import rig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400)
    ap.add_argument("--episodes", type=int, default=4096, help="episodes of each evaluate()")
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r09_interrupt_learning_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)
    TOTAL = a.warm + a.options * a.steps_per_option + a.after        # step-batches of every learner

    for mp in a.maps:
        lines = [f"# interrupt_learning_report map {mp} envs {a.envs} options {a.options} warm {a.warm} "
                 f"step-batches per learner {TOTAL} episodes {a.episodes} hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            res = {}
            for learner in ("plain", "interrupting"):
                t0 = time.time()
                ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, interrupt_learning=learner == "interrupting", **HP)
                ag.enable_tracing(64)
                ag.rollout(a.warm)
                created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=3000, max_examples=40000,
                                          start_coverage=0.9)
                chain_t = ag.t
                ag.rollout(TOTAL - ag.t)
                assert ag.t == TOTAL
                res[learner] = (ag.evaluate(n_episodes=a.episodes), ag.evaluate(n_episodes=a.episodes, interrupt=True))
                out = [f"seed {seed} {learner} learner: {len(created)} options, enabled mask {ag.enabled_mask:#x}, "
                       f"chain found by step-batch {chain_t}, {TOTAL} step-batches in {time.time() - t0:.0f} s",
                       f"  acting plain       {rig.fmt_eval(res[learner][0])}",
                       f"  acting interrupt   {rig.fmt_eval(res[learner][1])}"]
                for ln in out:
                    print(ln, flush=True)
                lines += out
                del ag
            out = [f"seed {seed} interrupting - plain learner, acting plain:     {rig.delta_eval(res['plain'][0], res['interrupting'][0])}",
                   f"seed {seed} interrupting - plain learner, acting interrupt: {rig.delta_eval(res['plain'][1], res['interrupting'][1])}"]
            for ln in out:
                print(ln, flush=True)
            lines += out
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r09_interrupt_learning_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
