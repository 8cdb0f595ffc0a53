"""Does some lambda < 1 get under the Monte-Carlo fit (SPEC §27.4)? For each map and seed, tools/value_fit_report.py's chain —
warm-up step-batches, chain_skills(), more step-batches — then ONE kept record of --episodes episodes at --epsilon, and on it
fit_values_to_returns(lam=..., sweeps=...) for every lambda of --lambdas (lambda = 1 is §16's Monte-Carlo fit, lambda = 0 fitted
one-step evaluation). Per lambda and sweep one line per value function: the held-out RMSE and mean error of Q^old and Q^new against
the MONTE-CARLO targets of returns_to_go (every lambda on §16's scale) and against the lambda-targets the sweep regressed, and
|Delta|.

Then every table — W itself and each (lambda, sweep)'s W_new — acts in ONE evaluate_policies population rollout per chain, greedy
and at epsilon = 0.1, on common random numbers: success rate, mean length, discounted return, and the paired difference of the
discounted return and of the success rate against W at the same epsilon +- its standard error.

    python tools/lambda_fit_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--out-dir profiles]
"""
import argparse, os, sys, time
import rig


def fmt_sweep(lam, s, sweep):
    out = []
    for k, r in sweep["vf"].items():
        h, mc = r["held_out"], r["mc"]["held_out"]
        out.append(f"    {lam:6.2f} {s:5d} {k:3d} {r['fit']['old']['n']:7d} {h['old']['n']:7d} {mc['old']['rmse']:9.2f} {mc['new']['rmse']:9.2f} "
                   f"{mc['old']['mean_error']:9.2f} {mc['new']['mean_error']:9.2f} {h['old']['rmse']:10.2f} {h['new']['rmse']:10.2f} {r['delta_norm']:9.3f}")
    return out


def chain_args(lambdas, tag):
    """The arguments of this report (tools/trace_fit_report.py takes the same ones)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--episodes", type=int, default=4096, help="recorded episodes of the kept record (half fitted, half held out)")
    ap.add_argument("--epsilon", type=float, default=0.1); ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--lambdas", type=float, nargs="+", default=lambdas)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--eval-epsilons", type=float, nargs="+", default=[0.0, 0.1]); ap.add_argument("--eval-episodes", type=int, default=4096)
    ap.add_argument("--out-dir", default=None, help=f"also write one report per map: <dir>/{tag}_<map>.txt")
    return ap


def writer(path, first):
    """say(line): print it, keep it, and rewrite `path` (None: no file) — a run that is cut short leaves what it had."""
    lines = [first]
    print(first, flush=True)
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)

    def say(ln):
        print(ln, flush=True)
        lines.append(ln)
        if path:
            with open(path, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    return say


def trained_chain(a, mp, seed, HP, say):
    """tools/value_fit_report.py's chain on map `mp`, and ONE kept record of a.episodes episodes at a.epsilon: (agent, trajectory)."""
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
    ag.enable_tracing(64)
    t_seed = time.time()
    ag.rollout(a.warm)
    created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
    ag.rollout(a.after)
    print(f"  (seed {seed}: chain trained, {time.time() - t_seed:.0f} s)", file=sys.stderr, flush=True)
    say(f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}")
    traj, summary = ag.record_episodes(n_episodes=a.episodes, epsilon=a.epsilon, seed=seed + 100)
    say(f"  the record: {a.episodes} episodes at epsilon {a.epsilon}, success {summary['success_rate']:.4f}, "
        f"{int(sum(traj.length(i) for i in range(traj.n)))} rows")
    return ag, traj


def evaluate_tables(ag, a, seed, tables, labels, say, width=6, per_epsilon=False):
    """Every table at every epsilon of a.eval_epsilons in ONE evaluate_policies run (per_epsilon: one run per epsilon, for more
    tables than half a population), a line per policy with its paired differences against tables[0] at the same epsilon. Returns
    the summaries, policy i * len(eval_epsilons) + e."""
    from skill_chaining_with_graphs_amd.evaluation import paired_differences
    n_eps = len(a.eval_epsilons)
    summaries, envs = [None] * (len(tables) * n_eps), [None] * (len(tables) * n_eps)
    for group in ([[e] for e in range(n_eps)] if per_epsilon else [list(range(n_eps))]):
        t0 = time.time()
        W_all = [w for w in tables for _ in group]
        sm, _, ev = ag.evaluate_policies(W_all, epsilons=[a.eval_epsilons[e] for _ in tables for e in group], n_episodes=a.eval_episodes,
                                         seed=seed + 200, per_env=True)
        say(f"  {len(W_all)} policies x {a.eval_episodes} episodes in one evaluation, {time.time() - t0:.1f} s")
        for n, (i, e) in enumerate((i, e) for i in range(len(tables)) for e in group):
            summaries[i * n_eps + e], envs[i * n_eps + e] = sm[n], ev[n]
    say(f"    {'table':>{width}}  eps  success   length  discounted   paired d(discounted) +-      se   paired d(success) +-      se")
    for i, (label, eps) in enumerate((lb, e) for lb in labels for e in a.eval_epsilons):
        s, p = summaries[i], paired_differences(envs[i], envs[i % n_eps])
        say(f"    {label:>{width}} {eps:4.2f} {s['success_rate']:8.4f} {s['mean_length']:8.1f} {s['mean_discounted_return']:11.2f} "
            f"{p['disc_final']['mean_diff']:22.2f} +- {p['disc_final']['se']:7.2f} {p['goal']['mean_diff']:19.4f} +- {p['goal']['se']:7.4f}")
    return summaries


def main():
    a = chain_args([0.0, 0.5, 0.8, 0.9, 0.95, 1.0], "r33_lambda_fit").parse_args()
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        first = (f"# lambda_fit_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} episodes {a.episodes} "
                 f"epsilon {a.epsilon} ridge {a.ridge} lambdas {a.lambdas} sweeps {a.sweeps} eval_epsilons {a.eval_epsilons} "
                 f"eval_episodes {a.eval_episodes} hparams {HP}")
        say = writer(os.path.join(a.out_dir, f"r33_lambda_fit_{mp}.txt") if a.out_dir else None, first)
        for seed in a.seeds:
            ag, traj = trained_chain(a, mp, seed, HP, say)
            say("    lambda sweep  vf   n_fit  n_held    mc_old    mc_new  bias_old  bias_new  lam_old_rm  lam_new_rm   |Delta|")
            tables, labels = [ag.W.clone()], ["W"]
            for lam in a.lambdas:
                t0 = time.time()
                rep, _ = ag.fit_values_to_returns(trajectory=traj, epsilon=a.epsilon, seed=seed + 100, ridge=a.ridge, lam=lam, sweeps=a.sweeps)
                for s, sweep in enumerate(rep["sweeps"], 1):
                    for ln in fmt_sweep(lam, s, sweep):
                        say(ln)
                    tables.append(sweep["W"])
                    labels.append(f"{lam:.2f}/{s}")
                print(f"  (lambda {lam}: {a.sweeps} sweeps, {time.time() - t0:.0f} s)", file=sys.stderr, flush=True)
            evaluate_tables(ag, a, seed, tables, labels, say)
            del ag


if __name__ == "__main__":
    main()
