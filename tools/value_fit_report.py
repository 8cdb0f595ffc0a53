"""What happens when the values are right (SPEC §16)? For each map and seed, tools/chain_evidence.py's protocol trains an agent
(warm-up step-batches, chain_skills(), more step-batches). Then, before and after fit_values_to_returns(apply=True) — the best
linear fit of every Q_k to the returns its own policy realises — the same two measurements: gate_audit() on the offer states
of a recorded greedy evaluation (tools/gate_audit_report.py's way (b)) and evaluate(discounted=True). A second fit round
follows on the new policy's returns, because the policy changed with the weights, with the same measurements after it.

Per fit round one line per value function: fit samples, held-out samples, RMSE and mean error of Q^old and Q^new against the
Monte-Carlo targets on the fit half and on the held-out half (the held-out RMSE after the fit is the basis's floor at this
sample size), and |Delta|.

    python tools/value_fit_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--envs 8192] [--options 5] [--episodes 4096]
"""
import argparse, os
import rig
from gate_audit_report import fmt_audit, offer_states


def fmt_fit(report):
    """One line per value function of a fit_values_to_returns() report."""
    out = ["    vf      n_fit n_held   fit_old   fit_new  held_old  held_new  bias_old  bias_new   |Delta|"]
    for k, r in report["vf"].items():
        f, h = r["fit"], r["held_out"]
        out.append(f"    vf {k:2d} {f['old']['n']:7d} {h['old']['n']:6d} {f['old']['rmse']:9.2f} {f['new']['rmse']:9.2f} {h['old']['rmse']:9.2f} "
                   f"{h['new']['rmse']:9.2f} {h['old']['mean_error']:9.2f} {h['new']['mean_error']:9.2f} {r['delta_norm']:9.3f}")
    return out


def measure(ag, a, seed, name):
    """evaluate(discounted=True) and the gate audit on the offer states of a recorded greedy evaluation."""
    ev = ag.evaluate(n_episodes=a.states, discounted=True)
    out = [f"  {name:<11s} {rig.fmt_eval(ev)} discounted {ev['mean_discounted_return']:.2f}"]
    if ag.enabled_mask:
        traj, _ = ag.record_episodes(n_episodes=a.record_envs)
        states = offer_states(traj, a.states)
        if len(states[0]):
            met = ag.gate_audit(states=states, seed=seed)
            out += [f"  {name} gate audit on {len(states[0])} offer states: {met['overall']['n']} have a candidate"] + fmt_audit(met)
        else:
            out += [f"  {name} gate audit: no offer state on {a.record_envs} recorded greedy episodes"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--states", type=int, default=4096, help="episodes evaluated, and start states audited at most")
    ap.add_argument("--record-envs", type=int, default=256, help="recorded greedy episodes the offer states are taken from")
    ap.add_argument("--episodes", type=int, default=4096, help="recorded episodes of a fit (half fitted, half held out)")
    ap.add_argument("--epsilon", type=float, default=0.1); ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r22_value_fit_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# value_fit_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} states {a.states} "
                 f"episodes {a.episodes} epsilon {a.epsilon} ridge {a.ridge} hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            ag.rollout(a.warm)
            created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)
            out = [f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}"] + measure(ag, a, seed, "before")
            for rnd, name in ((1, "after"), (2, "after 2")):
                report, _ = ag.fit_values_to_returns(n_episodes=a.episodes, epsilon=a.epsilon, seed=seed + 100 * rnd, ridge=a.ridge, apply=True)
                out += [f"  fit round {rnd}: {a.episodes} episodes at epsilon {a.epsilon}, success {report['episodes']['success_rate']:.4f}"]
                out += fmt_fit(report) + measure(ag, a, seed, name)
            for ln in out:
                print(ln, flush=True)
            lines += out
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r22_value_fit_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
