"""Does a safeguard take the collapses out of the policy-improvement step (SPEC §21.4)? For each map and seed,
tools/branch_fit_report.py's chain — warm-up step-batches, chain_skills(), more step-batches — and then, from that one trained
agent, --rounds rounds each of two ways to take the step:

  safeguarded     improve_policy(lambdas, eval_epsilons, apply=True): the fit's W_new damped by each lambda, every candidate and the
                  current W evaluated at every epsilon in ONE population rollout on common random numbers, the best candidate at
                  eval_epsilons[0] applied only where its paired difference against W exceeds z standard errors
  unconditional   the same call with apply=False, then lambda = 1 (W_new itself) applied whatever the evaluation says: what
                  tools/branch_fit_report.py does

Per round: the candidate table (lambda, epsilon, success rate, mean return, mean length, mean discounted return, and the paired
difference of the discounted return against W at the same epsilon +- its standard error) and what was applied. Before the first
round and after each: evaluate(discounted=True), greedy, on --eval-episodes episodes of one seed, as branch_fit_report prints it.

    python tools/policy_step_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--rounds 3] [--out-dir profiles]
"""
import argparse, os, sys, time
import rig
from branch_fit_report import fmt_policy


def fmt_candidates(report):
    out = ["    lambda  eps  success     return   length  discounted   paired d(discounted) +-      se"]
    for r in report["candidates"]:
        s, p = r["summary"], r["paired"]["disc_final"]
        out.append(f"    {r['lambda']:6.2f} {r['epsilon']:4.2f} {s['success_rate']:8.4f} {s['mean_return']:10.2f} {s['mean_length']:8.1f} "
                   f"{s['mean_discounted_return']:11.2f} {p['mean_diff']:22.2f} +- {p['se']:7.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=4096); ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--states", type=int, default=8192); ap.add_argument("--held", type=int, default=2048)
    ap.add_argument("--replicates", type=int, default=8)
    ap.add_argument("--lambdas", type=float, nargs="+", default=[0.25, 0.5, 1.0])
    ap.add_argument("--eval-epsilons", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--criterion", default="discounted"); ap.add_argument("--z", type=float, default=2.0)
    ap.add_argument("--eval-episodes", type=int, default=4096)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r27_policy_step_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# policy_step_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} rounds {a.rounds} "
                 f"episodes {a.episodes} epsilon {a.epsilon} ridge {a.ridge} states {a.states} held {a.held} replicates {a.replicates} "
                 f"lambdas {a.lambdas} eval_epsilons {a.eval_epsilons} criterion {a.criterion} z {a.z} eval_episodes {a.eval_episodes} "
                 f"hparams {HP}"]
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
            W_trained = ag.W.clone()
            for mode in ("safeguarded", "unconditional"):
                ag.W.copy_(W_trained)                          # both ways start from the one trained table (the fits read nothing else
                say(f" {mode}:")                                # that a round changes: W is all that apply=True writes)
                say(fmt_policy("before", ag.evaluate(a.eval_episodes, seed=seed + 200, discounted=True)))
                for rnd in range(1, a.rounds + 1):
                    t0 = time.time()
                    rep, _ = ag.improve_policy(
                        lambdas=a.lambdas, eval_epsilons=a.eval_epsilons, criterion=a.criterion, z=a.z, n_eval=a.eval_episodes,
                        apply=(mode == "safeguarded"), n_states=a.states, n_held=a.held, replicates=a.replicates, ridge=a.ridge,
                        epsilon=a.epsilon, seed=seed + 100 * rnd, n_episodes=a.episodes)
                    if mode == "unconditional":                # the same fit again (one seed, one W_new), applied: lambda = 1
                        ag.fit_values_to_branches(apply=True, n_states=a.states, n_held=a.held, replicates=a.replicates,
                                                  ridge=a.ridge, epsilon=a.epsilon, seed=seed + 100 * rnd, n_episodes=a.episodes)
                        applied = "lambda 1.00 (unconditional)"
                    else:
                        applied = f"lambda {rep['chosen_lambda']:.2f} (accepted)" if rep["accepted"] else "nothing (W kept)"
                    note(f"{mode} round {rnd}")
                    say(f"  round {rnd}: fit, {len(rep['candidates'])} policies x {a.eval_episodes} episodes in one evaluation, {time.time() - t0:.1f} s; "
                        f"the rule would choose lambda {rep['chosen_lambda']:.2f}; applied: {applied}")
                    for ln in fmt_candidates(rep):
                        say(ln)
                    say(fmt_policy(f"after round {rnd}", ag.evaluate(a.eval_episodes, seed=seed + 200, discounted=True)))
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r27_policy_step_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
