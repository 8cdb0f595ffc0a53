"""Is the maximisation bias of the bootstrap what keeps the sweeps from being a descent (SPEC §29.4)? On tools/lambda_fit_report.py's
chains and kept records (its functions, not copies of them): fit_values_to_returns(lam=..., sweeps=...) in two arms — `single` (SPEC
§27 / §28 as they stand: the targets bootstrap from the maximum of the table just fitted) and `double` (SPEC §29.2: two tables on two
folds of the fit half, each bootstrapping from the OTHER table's value of its own greedy action; the mean table is handed on) —
under both traces, for every lambda of --lambdas. Per arm, trace, lambda, sweep and value function one line: the cut share (what
the Watkins cut leaves of the trace), the held-out RMSE and mean error of Q^new on §16's Monte-Carlo scale, and for the double arm
`optimism`: the mean of vs - v over the value function's bootstrapped rows, the max's bias as the two tables estimate it (exactly 0
in sweep 1, where the two tables are one), and `n_boot`, the number of those rows in the record: over the two target sets the
gaps of a row on which both tables select the same action cancel exactly, so an `optimism` over a handful of rows is 0 or one
row's gap, not an estimate.

The single arm makes tools/trace_fit_report.py's calls: where <check-dir>/r34_trace_fit_<map>.txt was written with the same chain
arguments, every single-arm line it shares with that file (same trace, lambda, sweep, value function) is compared with it as text,
and the count is reported — the harness did not drift where all of them are found.

Then W and every table act in evaluate_policies population rollouts of --eval-episodes episodes each, one per trace and epsilon (41
policies at the defaults, of the 64 a population holds), greedy and at epsilon = 0.1, on common random numbers; and per arm, trace,
lambda and epsilon the headline line `descent`: the mean discounted return of the tables of sweeps 1 .. S.

    python tools/double_fit_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--out-dir profiles] [--check-dir profiles]
"""
import os, sys, time
import rig
import lambda_fit_report as LF
import trace_fit_report as TF

TRACES = ("peng", "watkins")


def fmt_sweep(arm, trace, lam, s, sweep):
    out = []
    for k, r in sweep["vf"].items():
        mc = r["mc"]["held_out"]
        opt = "         -       -" if "optimism" not in r else f"{r['optimism']:10.3f} {r['optimism_n']:7d}"
        out.append(f"    {arm:>6} {trace:>7} {lam:6.2f} {s:5d} {k:3d} {r['fit']['old']['n']:7d} {mc['old']['n']:7d} {r['cut_share']:9.4f} "
                   f"{mc['old']['rmse']:9.2f} {mc['new']['rmse']:9.2f} {mc['new']['mean_error']:9.2f} {opt}")
    return out


def earlier_lines(path, first):
    """(trace, lambda, sweep, vf) -> the stripped lines (one per seed) of an r34 report whose chain arguments (map .. ridge, sweeps,
    hparams) are `first`'s, else None."""
    if not path or not os.path.exists(path):
        return None
    with open(path) as fh:
        lines = fh.read().splitlines()
    cut = lambda ln: (ln.split(" map ", 1)[-1].split(" lambdas ")[0], ln.split(" sweeps ", 1)[-1].split(" eval_epsilons ")[0],
                      ln.split(" hparams ", 1)[-1])
    if not lines or cut(lines[0]) != cut(first):
        return None
    out = {}
    for ln in lines:
        if ln.startswith("    ") and ln.split()[0] in TRACES and len(ln.split()) == 12:
            out.setdefault(tuple(ln.split()[:4]), set()).add(ln.strip())
    return out


def main():
    ap = LF.chain_args([0.0, 0.5, 0.9, 0.95, 1.0], "r35_double_fit")
    ap.add_argument("--check-dir", default="profiles", help="where r34_trace_fit_<map>.txt lies (the single arm is compared with it)")
    a = ap.parse_args()
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        first = (f"# double_fit_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} episodes {a.episodes} "
                 f"epsilon {a.epsilon} ridge {a.ridge} lambdas {a.lambdas} sweeps {a.sweeps} eval_epsilons {a.eval_epsilons} "
                 f"eval_episodes {a.eval_episodes} hparams {HP}")
        say = LF.writer(os.path.join(a.out_dir, f"r35_double_fit_{mp}.txt") if a.out_dir else None, first)
        earlier = earlier_lines(os.path.join(a.check_dir, f"r34_trace_fit_{mp}.txt") if a.check_dir else None, first)
        for seed in a.seeds:
            ag, traj = LF.trained_chain(a, mp, seed, HP, say)
            say("  mc_*: held-out error against the Monte-Carlo returns of the RECORDING policy (epsilon-greedy on W); "
                "optimism: mean of vs - v over the n_boot bootstrapped rows")
            say("       arm   trace lambda sweep  vf   n_fit  n_held cut_share    mc_old    mc_new  bias_new   optimism  n_boot")
            found = shared = 0
            per_trace = {}
            for trace in TRACES:
                tables, labels = [ag.W.clone()], ["W"]
                for arm in ("single", "double"):
                    for lam in a.lambdas:
                        t0 = time.time()
                        rep, _ = ag.fit_values_to_returns(trajectory=traj, epsilon=a.epsilon, seed=seed + 100, ridge=a.ridge,
                                                          lam=[lam] * ag.n_vf, sweeps=a.sweeps, trace=trace, double=arm == "double")
                        for s, sweep in enumerate(rep["sweeps"], 1):
                            for ln in fmt_sweep(arm, trace, lam, s, sweep):
                                say(ln)
                            if arm == "single" and earlier is not None:
                                for ln in TF.fmt_sweep(trace, lam, s, sweep):      # (r34 holds lambda = 0 under "peng" only)
                                    key = tuple(ln.split()[:4])
                                    shared += key in earlier
                                    found += ln.strip() in earlier.get(key, ())
                            tables.append(sweep["W"])
                            labels.append(f"{arm}/{trace}/{lam:.2f}/{s}")
                        print(f"  ({arm} {trace} lambda {lam}: {a.sweeps} sweeps, {time.time() - t0:.0f} s)", file=sys.stderr, flush=True)
                per_trace[trace] = (tables, labels)
            if earlier is None:
                say("  drift check: no r34_trace_fit report with these chain arguments to compare the single arm with")
            else:
                say(f"  drift check: {found} of the {shared} single-arm lines shared with r34_trace_fit_{mp}.txt are found there as text")
            for trace, (tables, labels) in per_trace.items():
                summaries = LF.evaluate_tables(ag, a, seed, tables, labels, say, width=22, per_epsilon=True)
                n_eps = len(a.eval_epsilons)
                say(f"  the headline, trace {trace}: mean discounted return of the tables of sweeps 1 .. {a.sweeps} (W: "
                    + ", ".join(f"{summaries[e]['mean_discounted_return']:.2f} at epsilon {eps:.2f}" for e, eps in enumerate(a.eval_epsilons)) + ")")
                i = 0
                for arm in ("single", "double"):
                    for lam in a.lambdas:
                        for e, eps in enumerate(a.eval_epsilons):
                            vals = [summaries[(1 + i * a.sweeps + s) * n_eps + e]["mean_discounted_return"] for s in range(a.sweeps)]
                            say(f"  descent {arm:>6} {trace:>7} {lam:4.2f} {eps:4.2f} " + " ".join(f"{v:10.2f}" for v in vals))
                        i += 1
            del ag


if __name__ == "__main__":
    main()
