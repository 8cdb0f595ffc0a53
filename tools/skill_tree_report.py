"""Does growing a skill tree (SPEC §13, grow_skill_tree) find better skills than growing a chain (chain_skills)? For each map and
seed, two agents are trained with tools/interrupt_learning_report.py's protocol and hyper-parameters (warm-up step-batches, the
discovery loop, more step-batches), one discovering with chain_skills() and one with grow_skill_tree(). Both stop at the same
env-step count: the step-batches discovery did not use are added to the last phase. Each greedy policy is then evaluated on the
same episodes; one line each reports the parents found, success rate, mean return, mean length and, per value function (root
first), the step share and option entries.

    python tools/skill_tree_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--envs 8192] [--options 5]
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
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r10_skill_tree_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)
    TOTAL = a.warm + a.options * a.steps_per_option + a.after        # step-batches of every learner
    DISCOVERY = dict(steps_per_option=a.steps_per_option, min_examples=3000, max_examples=40000, start_coverage=0.9)

    for mp in a.maps:
        lines = [f"# skill_tree_report map {mp} envs {a.envs} options {a.options} warm {a.warm} step-batches per learner {TOTAL} "
                 f"episodes {a.episodes} discovery {DISCOVERY} hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            res = {}
            for learner in ("chain", "tree"):
                t0 = time.time()
                ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
                ag.enable_tracing(64)
                ag.rollout(a.warm)
                grow = ag.chain_skills if learner == "chain" else ag.grow_skill_tree
                created = grow(**DISCOVERY)
                found_t = ag.t
                ag.rollout(TOTAL - ag.t)
                assert ag.t == TOTAL
                res[learner] = ag.evaluate(n_episodes=a.episodes)
                made = [(r["option"], r["parent"], r["examples"]) for r in created]
                out = [f"seed {seed} {learner}: {len(created)} options (option, parent, examples) {made}, enabled mask "
                       f"{ag.enabled_mask:#x}, parents {[int(p) for p in ag.ctx.parents]}, discovery done by step-batch {found_t}, "
                       f"{TOTAL} step-batches in {time.time() - t0:.0f} s"]
                if learner == "tree":
                    out.append(f"  node examples at each decision {[r['node_examples'] for r in created]}")
                out.append(f"  acting {rig.fmt_eval(res[learner], declines=False)}")
                for ln in out:
                    print(ln, flush=True)
                lines += out
                del ag
            out = [f"seed {seed} tree - chain: {rig.delta_eval(res['chain'], res['tree'])}"]
            print(out[0], flush=True)
            lines += out
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r10_skill_tree_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
