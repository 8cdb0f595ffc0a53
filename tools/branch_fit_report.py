"""Does fitting Q to all-action branch returns and acting greedily on it improve the policy (SPEC §20)? For each map and seed,
tools/branch_report.py's chain — warm-up step-batches, chain_skills(), more step-batches — then up to --rounds rounds of
{fit_values_to_branches(apply=True) on --episodes fresh episodes at --epsilon: --states fit rows and --held held-out rows per value
function, --replicates branch rollouts of each of the five first actions; evaluate() greedy on --eval-episodes episodes}.

Per round and value function one line of the report's HELD-OUT half: the rows fitted and held out; the RMSE of Q^old and Q^new
against the held-out branch means and se, the RMSE a perfect Q^pi would still show against them; agree_old / agree_new (the greedy
action of Q^old / Q^new is the best action by the held-out means), changed (the greedy action changed) and gain +- se: the mean of
gbar[a_new] - gbar[a_old], the one-step improvement the new greedy action brings under the policy that ran the branches, unbiased
because W_new never saw the held-out replicates. Before the first round and after each: evaluate(discounted=True), greedy, on
--eval-episodes episodes of one seed: success rate, mean return, mean length and mean discounted return.

    python tools/branch_fit_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--rounds 3] [--states 8192] [--held 2048]
"""
import argparse, os, sys, time
import rig


def fmt_fit(report):
    """One line per value function of a fit_values_to_branches() report: its held-out half."""
    out = ["    vf    fit   held   rmse_old   rmse_new        se  agree_old agree_new changed       gain +-      se   |delta|"]
    for k, r in report["vf"].items():
        if not r["n_fit"]:
            out.append(f"    vf {k:2d}      0  (no fit row)")
            continue
        h, g = r["held_out"], r["held_out"]["greedy"]
        out.append(f"    vf {k:2d} {r['n_fit']:6d} {r['n_held']:6d} {h['old']['rmse']:10.2f} {h['new']['rmse']:10.2f} {h['target_se']:9.2f} "
                   f"{g['agreement_old']:10.3f} {g['agreement_new']:9.3f} {g['changed']:7.3f} {g['one_step_gain']:10.2f} +- "
                   f"{g['one_step_gain_se']:7.2f} {r['delta_norm']:9.2f}")
    return out


def fmt_policy(tag, r):
    return (f"  {tag:<14s} success {r['success_rate']:.4f} return {r['mean_return']:9.2f} length {r['mean_length']:7.1f} "
            f"discounted {r['mean_discounted_return']:9.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=4096, help="fresh recorded episodes per round (even envs fitted, odd held out)")
    ap.add_argument("--epsilon", type=float, default=0.1); ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--states", type=int, default=8192); ap.add_argument("--held", type=int, default=2048)
    ap.add_argument("--replicates", type=int, default=8)
    ap.add_argument("--eval-episodes", type=int, default=4096)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r26_branch_fit_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# branch_fit_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} rounds {a.rounds} "
                 f"episodes {a.episodes} epsilon {a.epsilon} ridge {a.ridge} states {a.states} held {a.held} replicates {a.replicates} "
                 f"eval_episodes {a.eval_episodes} hparams {HP}"]
        print(lines[0], flush=True)

        def say(ln):
            print(ln, flush=True)
            lines.append(ln)

        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            t_seed = time.time()
            note = lambda what: print(f"  (seed {seed}: {what}, {time.time() - t_seed:.0f} s)", file=sys.stderr, flush=True)
            ag.rollout(a.warm)
            created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)
            note("chain trained")
            say(f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}")
            say(fmt_policy("before", ag.evaluate(a.eval_episodes, seed=seed + 200, discounted=True)))
            for rnd in range(1, a.rounds + 1):
                t0 = time.time()
                rep, _ = ag.fit_values_to_branches(n_states=a.states, n_held=a.held, replicates=a.replicates, ridge=a.ridge,
                                                   epsilon=a.epsilon, seed=seed + 100 * rnd, n_episodes=a.episodes, apply=True)
                n_branch = sum(r["n_fit"] + r["n_held"] for r in rep["vf"].values()) * 5 * a.replicates
                note(f"round {rnd} fitted")
                say(f"  round {rnd}: {n_branch} branch episodes, fit and solve in {time.time() - t0:.1f} s; held-out rows:")
                for ln in fmt_fit(rep):
                    say(ln)
                say(fmt_policy(f"after round {rnd}", ag.evaluate(a.eval_episodes, seed=seed + 200, discounted=True)))
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r26_branch_fit_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
