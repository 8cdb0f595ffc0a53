"""Do lambda-return targets whose trace is cut at every non-greedy recorded action make the sweeps a descent (SPEC §28.4)? On
tools/lambda_fit_report.py's chains and kept records (its functions, not copies of them): fit_values_to_returns(lam=..., sweeps=...)
under both traces — "peng" (SPEC §27's uncut trace, here through trace_targets(cut=False), the same bits) and "watkins" (cut
wherever the recorded action is not the greedy action of the table bootstrapped from) — for every lambda of --lambdas, and lambda = 0
once, where the two coincide. Per arm, lambda, sweep and value function one line: the share of its sample rows whose trace is cut,
the mean horizon h of the root stream over them, the held-out RMSE and mean error of Q^new on §16's Monte-Carlo scale — THE RETURNS
OF THE RECORDING POLICY, on which targets that evaluate another (the greedy) policy are expected to score worse —, and the share of
rows whose greedy action changed against the sweep before's table.

Then W and every table act in ONE evaluate_policies population rollout per chain and epsilon (45 policies each at the defaults, of
the 64 a population holds), greedy and at epsilon = 0.1, on common random numbers, as in lambda_fit_report.py; and per arm, lambda
and epsilon the headline line `descent`: the mean discounted return of the tables of sweeps 1 .. S. A sequence that does not fall
is what "the sweeps are a descent" would look like.

    python tools/trace_fit_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--out-dir profiles]
"""
import os, sys, time
import rig
import lambda_fit_report as LF


def fmt_sweep(arm, lam, s, sweep):
    out = []
    for k, r in sweep["vf"].items():
        mc = r["mc"]["held_out"]
        changed = "        -" if r["a_changed"] is None else f"{r['a_changed']:9.4f}"
        out.append(f"    {arm:>7} {lam:6.2f} {s:5d} {k:3d} {r['fit']['old']['n']:7d} {mc['old']['n']:7d} {r['cut_share']:9.4f} {r['horizon']:9.2f} "
                   f"{mc['old']['rmse']:9.2f} {mc['new']['rmse']:9.2f} {mc['new']['mean_error']:9.2f} {changed}")
    return out


def main():
    a = LF.chain_args([0.5, 0.8, 0.9, 0.95, 1.0], "r34_trace_fit").parse_args()
    HP = rig.discovery_hp(a.envs)
    arms = [("peng", 0.0)] + [(arm, lam) for arm in ("peng", "watkins") for lam in a.lambdas if lam != 0.0]

    for mp in a.maps:
        first = (f"# trace_fit_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} episodes {a.episodes} "
                 f"epsilon {a.epsilon} ridge {a.ridge} lambdas {a.lambdas} (and 0 once) sweeps {a.sweeps} eval_epsilons {a.eval_epsilons} "
                 f"eval_episodes {a.eval_episodes} hparams {HP}")
        say = LF.writer(os.path.join(a.out_dir, f"r34_trace_fit_{mp}.txt") if a.out_dir else None, first)
        for seed in a.seeds:
            ag, traj = LF.trained_chain(a, mp, seed, HP, say)
            say("  mc_*: held-out error against the Monte-Carlo returns of the RECORDING policy (epsilon-greedy on W)")
            say("        arm lambda sweep  vf   n_fit  n_held cut_share   horizon    mc_old    mc_new  bias_new a_changed")
            tables, labels = [ag.W.clone()], ["W"]
            for arm, lam in arms:
                t0 = time.time()
                rep, _ = ag.fit_values_to_returns(trajectory=traj, epsilon=a.epsilon, seed=seed + 100, ridge=a.ridge, lam=[lam] * ag.n_vf,
                                                  sweeps=a.sweeps, trace=arm)
                for s, sweep in enumerate(rep["sweeps"], 1):
                    for ln in fmt_sweep(arm, lam, s, sweep):
                        say(ln)
                    tables.append(sweep["W"])
                    labels.append(f"{arm}/{lam:.2f}/{s}")
                print(f"  ({arm} lambda {lam}: {a.sweeps} sweeps, {time.time() - t0:.0f} s)", file=sys.stderr, flush=True)
            summaries = LF.evaluate_tables(ag, a, seed, tables, labels, say, width=15, per_epsilon=True)
            n_eps = len(a.eval_epsilons)
            say(f"  the headline: mean discounted return of the tables of sweeps 1 .. {a.sweeps} (W: "
                + ", ".join(f"{summaries[e]['mean_discounted_return']:.2f} at epsilon {eps:.2f}" for e, eps in enumerate(a.eval_epsilons)) + ")")
            for i, (arm, lam) in enumerate(arms):
                for e, eps in enumerate(a.eval_epsilons):
                    vals = [summaries[(1 + i * a.sweeps + s) * n_eps + e]["mean_discounted_return"] for s in range(a.sweeps)]
                    say(f"  descent {arm:>7} {lam:4.2f} {eps:4.2f} " + " ".join(f"{v:10.2f}" for v in vals))
            del ag


if __name__ == "__main__":
    main()
