"""Does weighting the branch fit by the precision of its targets buy anything (SPEC §22)? For each map and seed,
tools/branch_fit_report.py's chain — warm-up step-batches, chain_skills(), more step-batches — then ONE record and ONE set of branch
rollouts (fit_values_to_branches(keep=True): --states fit rows and --held held-out rows per value function, --replicates rollouts of
each of the five first actions) and, from those same returns (branches=), three regressions: unweighted, "precision" (a weight per
state, 1 / (mean_a se2 + tau2)) and "precision_per_action" (a weight per state and action, five Grams). tau2 is --tau2, or each
value function's median of the variances (the default of valuefit.precision_weights); the value used is printed.

Per fit and value function one line of the HELD-OUT half, on ONE yardstick — unweighted statistics against the held-out branch means,
whatever the weighting: the RMSE of Q^old and Q^new and se, the RMSE a perfect Q^pi would still show; the effective sample size
(sum w)^2 / sum w^2 of the fit rows (per action: the smallest and the largest of the five); agree_new and the one-step gain +- se
as branch_fit_report prints them. Then ONE evaluate_policies run, greedy, on --eval-episodes episodes each, of W and of W + lambda
(W_new - W) for every lambda and fit — common random numbers, the paired difference of the discounted return against W +- se — and
what valuefit.choose_candidate would pick among each fit's candidates.

    python tools/weighted_fit_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--tau2 T] [--out-dir profiles]
"""
import argparse, os, sys, time
import rig

FITS = (None, "precision", "precision_per_action")


def fmt_fit(report):
    """One line per value function of a fit_values_to_branches() report: its held-out half and the fit rows' effective size."""
    out = ["    vf    fit   held       tau2        n_eff   rmse_old   rmse_new        se agree_new       gain +-      se   |delta|"]
    for k, r in report["vf"].items():
        if not r["n_fit"]:
            out.append(f"    vf {k:2d}      0  (no fit row)")
            continue
        h, g = r["held_out"], r["held_out"]["greedy"]
        n_eff = r.get("effective_n", float(r["n_fit"]))
        n_eff = f"{min(n_eff):6.0f}-{max(n_eff):<6.0f}" if isinstance(n_eff, list) else f"{n_eff:13.1f}"
        tau2 = f"{r['tau2']:10.2f}" if "tau2" in r else "         -"
        out.append(f"    vf {k:2d} {r['n_fit']:6d} {r['n_held']:6d} {tau2} {n_eff} {h['old']['rmse']:10.2f} {h['new']['rmse']:10.2f} "
                   f"{h['target_se']:9.2f} {g['agreement_new']:9.3f} {g['one_step_gain']:10.2f} +- {g['one_step_gain_se']:7.2f} "
                   f"{r['delta_norm']:9.2f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--episodes", type=int, default=4096); ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--states", type=int, default=8192); ap.add_argument("--held", type=int, default=2048)
    ap.add_argument("--replicates", type=int, default=8)
    ap.add_argument("--tau2", type=float, default=None, help="default: per value function, the median of the targets' variances")
    ap.add_argument("--lambdas", type=float, nargs="+", default=[0.25, 0.5, 1.0])
    ap.add_argument("--criterion", default="discounted"); ap.add_argument("--z", type=float, default=2.0)
    ap.add_argument("--eval-episodes", type=int, default=4096)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r28_weighted_fit_<map>.txt")
    a = ap.parse_args()
    import torch
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    from skill_chaining_with_graphs_amd.evaluation import paired_differences
    from skill_chaining_with_graphs_amd.valuefit import choose_candidate, damped_tables
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# weighted_fit_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} episodes {a.episodes} "
                 f"epsilon {a.epsilon} ridge {a.ridge} states {a.states} held {a.held} replicates {a.replicates} tau2 {a.tau2} "
                 f"lambdas {a.lambdas} criterion {a.criterion} z {a.z} eval_episodes {a.eval_episodes} hparams {HP}"]
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
            fit = dict(n_states=a.states, n_held=a.held, replicates=a.replicates, ridge=a.ridge, epsilon=a.epsilon, seed=seed + 100,
                       n_episodes=a.episodes)
            t0 = time.time()
            base, W_base = ag.fit_values_to_branches(keep=True, **fit)
            n_branch = sum(r["n_fit"] + r["n_held"] for r in base["vf"].values()) * 5 * a.replicates
            say(f"  one record, {n_branch} branch episodes, the unweighted fit and solve in {time.time() - t0:.1f} s; held-out rows per fit:")
            tables = {}
            for weighting in FITS:
                t0 = time.time()
                rep, W_new = (base, W_base) if weighting is None else ag.fit_values_to_branches(
                    weighting=weighting, tau2=a.tau2, branches=base, **fit)
                say(f"  fit {weighting or 'unweighted'}" + ("" if weighting is None else f" (from the same returns, {time.time() - t0:.1f} s)") + ":")
                for ln in fmt_fit(rep):
                    say(ln)
                tables[weighting] = W_new
                note(f"fit {weighting}")
            # one population run: W, then every fit's damped candidates
            shape = (ag.n_vf, 5, -1)
            cand = [damped_tables(ag.W.reshape(shape), tables[w].reshape(shape), a.lambdas) for w in FITS]
            summaries, _, envs = ag.evaluate_policies(torch.cat([ag.W.reshape(1, *shape)] + cand), 0.0, None, n_episodes=a.eval_episodes,
                                                      seed=seed + 200, per_env=True)
            say(f"  {len(summaries)} policies x {a.eval_episodes} episodes in one evaluation, greedy:")
            say("    fit                   lambda  success     return   length  discounted   paired d(discounted) +-      se")
            row = lambda name, lam, s, p: (f"    {name:<20s} {lam:6.2f} {s['success_rate']:8.4f} {s['mean_return']:10.2f} {s['mean_length']:8.1f} "
                                           f"{s['mean_discounted_return']:11.2f} {p['mean_diff']:22.2f} +- {p['se']:7.2f}")
            base_row = {"lambda": 0.0, "summary": summaries[0], "paired": paired_differences(envs[0], envs[0])}
            say(row("W", 0.0, summaries[0], base_row["paired"]["disc_final"]))
            for f, weighting in enumerate(FITS):
                rows = [base_row]
                for i, lam in enumerate(a.lambdas):
                    c = 1 + f * len(a.lambdas) + i
                    rows.append({"lambda": lam, "summary": summaries[c], "paired": paired_differences(envs[c], envs[0])})
                    say(row(weighting or "unweighted", lam, summaries[c], rows[-1]["paired"]["disc_final"]))
                pick = choose_candidate(rows, a.criterion, a.z)
                say(f"    {weighting or 'unweighted'}: choose_candidate picks lambda {pick['chosen_lambda']:.2f}"
                    f" ({'accepted' if pick['accepted'] else 'W kept'})")
            del ag, base
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r28_weighted_fit_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
