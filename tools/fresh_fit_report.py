"""Does a fresh record per sweep make the fitted sweeps a descent (SPEC §30.4)? On tools/trace_fit_report.py's chains and kept
records (lambda_fit_report's functions, not copies of them): fit_values_to_returns(lam=..., sweeps=...) in four arms — the record
`kept` over the sweeps (§28's arm, here through pipeline="device": the same bits) or `fresh` (every sweep after the first records
--episodes new episodes under the table the sweep before handed on, SPEC §30.3), each under both traces, "peng" and "watkins" — for
every lambda of --lambdas, and lambda = 0 once per record arm, where the traces coincide. Per arm, lambda, sweep and value function
one line: the share of its sample rows whose trace is cut, the mean horizon of the root stream over them, the held-out RMSE and mean
error of Q^new against the Monte-Carlo returns of THE SWEEP'S OWN record, and the success rate of that record's episodes.

The kept arm's lines are trace_fit_report's, character for character: with --r34-dir every one of them must be found in
<dir>/r34_trace_fit_<map>.txt (the drift check), and the run ends where one is not. The fresh arm's sweep 1 runs on the kept record
and must equal the kept arm's by bits; its table is not evaluated twice.

Then W and every table act in ONE evaluate_policies population rollout per epsilon (64 policies at the defaults, a full
population), greedy and at epsilon = 0.1, on common random numbers; and per arm, lambda and epsilon the headline line `descent`.

    python tools/fresh_fit_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--out-dir profiles] [--r34-dir profiles]
"""
import os, sys, time
import rig
import lambda_fit_report as LF
import trace_fit_report as TF


def fmt_fresh(arm, lam, s, sweep):
    out = []
    for k, r in sweep["vf"].items():
        mc = r["mc"]["held_out"]
        out.append(f"    fresh/{arm:<7} {lam:6.2f} {s:5d} {k:3d} {r['fit']['old']['n']:7d} {mc['old']['n']:7d} {r['cut_share']:9.4f} {r['horizon']:9.2f} "
                   f"{mc['old']['rmse']:9.2f} {mc['new']['rmse']:9.2f} {mc['new']['mean_error']:9.2f} {sweep['episodes']['success_rate']:9.4f}")
    return out


def main():
    ap = LF.chain_args([0.5, 0.9, 0.95, 1.0], "r36_fresh_fit")
    ap.add_argument("--r34-dir", default=None, help="check the kept arm's lines against <dir>/r34_trace_fit_<map>.txt")
    a = ap.parse_args()
    import torch
    HP = rig.discovery_hp(a.envs)
    arms = [("peng", 0.0)] + [(arm, lam) for arm in ("peng", "watkins") for lam in a.lambdas if lam != 0.0]

    for mp in a.maps:
        first = (f"# fresh_fit_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} episodes {a.episodes} "
                 f"epsilon {a.epsilon} ridge {a.ridge} lambdas {a.lambdas} (and 0 once per record arm) sweeps {a.sweeps} "
                 f"eval_epsilons {a.eval_epsilons} eval_episodes {a.eval_episodes} hparams {HP}")
        say = LF.writer(os.path.join(a.out_dir, f"r36_fresh_fit_{mp}.txt") if a.out_dir else None, first)
        r34 = open(os.path.join(a.r34_dir, f"r34_trace_fit_{mp}.txt")).read().splitlines() if a.r34_dir else None
        for seed in a.seeds:
            ag, traj = LF.trained_chain(a, mp, seed, HP, say)
            kw = dict(trajectory=traj, n_episodes=a.episodes, epsilon=a.epsilon, seed=seed + 100, ridge=a.ridge, sweeps=a.sweeps)
            say("  mc_*: held-out error against the Monte-Carlo returns of the policy that made THE SWEEP'S record")
            say("        arm lambda sweep  vf   n_fit  n_held cut_share   horizon    mc_old    mc_new  bias_new a_changed   (kept)")
            say("    fresh/arm   lambda sweep  vf   n_fit  n_held cut_share   horizon    mc_old    mc_new  bias_new rec_succ")
            tables, labels, found = [ag.W.clone()], ["W"], 0
            first_sweep = {}
            for arm, lam in arms:
                t0 = time.time()
                rep, _ = ag.fit_values_to_returns(lam=[lam] * ag.n_vf, trace=arm, pipeline="device", **kw)
                for s, sweep in enumerate(rep["sweeps"], 1):
                    for ln in TF.fmt_sweep(arm, lam, s, sweep):
                        say(ln)
                        if r34 is not None:
                            if ln not in r34:
                                raise SystemExit(f"drift: the kept arm's line is not in r34_trace_fit_{mp}.txt:\n{ln}")
                            found += 1
                    tables.append(sweep["W"])
                    labels.append(f"kept/{arm}/{lam:.2f}/{s}")
                first_sweep[arm, lam] = rep["sweeps"][0]
                print(f"  (kept {arm} lambda {lam}: {a.sweeps} sweeps, {time.time() - t0:.0f} s)", file=sys.stderr, flush=True)
            if r34 is not None:
                say(f"  drift check: all {found} lines of the kept arm are in r34_trace_fit_{mp}.txt")
            for arm, lam in arms:
                t0 = time.time()
                rep, _ = ag.fit_values_to_returns(lam=[lam] * ag.n_vf, trace=arm, fresh=True, **kw)
                one, kept = rep["sweeps"][0], first_sweep[arm, lam]
                same_lines = TF.fmt_sweep(arm, lam, 1, kept) == TF.fmt_sweep(arm, lam, 1, one)      # (a_changed: None in both)
                if not torch.equal(one["W"].view(torch.int32), kept["W"].view(torch.int32)) or not same_lines:
                    raise SystemExit(f"the fresh arm's sweep 1 differs from the kept arm's ({arm}, lambda {lam})")
                for s, sweep in enumerate(rep["sweeps"], 1):
                    sweep = dict(sweep, episodes=sweep["episodes"] or {"success_rate": float("nan")})
                    for ln in fmt_fresh(arm, lam, s, sweep):
                        say(ln)
                    if s > 1:
                        tables.append(sweep["W"])
                        labels.append(f"fresh/{arm}/{lam:.2f}/{s}")
                print(f"  (fresh {arm} lambda {lam}: {a.sweeps} sweeps, {time.time() - t0:.0f} s)", file=sys.stderr, flush=True)
            say(f"  the fresh arm's sweep 1 equals the kept arm's by bits ({len(arms)} fits): its tables are the kept arm's")
            summaries = LF.evaluate_tables(ag, a, seed, tables, labels, say, width=21, per_epsilon=True)
            n_eps = len(a.eval_epsilons)
            say(f"  the headline: mean discounted return of the tables of sweeps 1 .. {a.sweeps} (W: "
                + ", ".join(f"{summaries[e]['mean_discounted_return']:.2f} at epsilon {eps:.2f}" for e, eps in enumerate(a.eval_epsilons)) + ")")
            at = {lb: i for i, lb in enumerate(labels)}
            for rec in ("kept", "fresh"):
                for arm, lam in arms:
                    for e, eps in enumerate(a.eval_epsilons):
                        idx = [at[f"{'kept' if s == 1 else rec}/{arm}/{lam:.2f}/{s}"] for s in range(1, a.sweeps + 1)]
                        vals = [summaries[i * n_eps + e]["mean_discounted_return"] for i in idx]
                        say(f"  descent {rec:>5} {arm:>7} {lam:4.2f} {eps:4.2f} " + " ".join(f"{v:10.2f}" for v in vals))
            del ag


if __name__ == "__main__":
    main()
