"""Is the learner's fixed point any good, and does least-squares policy iteration improve the policy (SPEC §17)? For each map and
seed, tools/chain_evidence.py's protocol trains an agent (warm-up step-batches, chain_skills(), more step-batches). One set of
recorded episodes is then evaluated by fit_values_lstdq(rounds=R): round r's weights are those of the greedy policy of round
r - 1's, solved in closed form from the same samples. The agent is measured with the weights it trained, with the weights after
each round, and, for comparison, after one fit_values_to_returns() on the same episodes (tools/value_fit_report.py's fit): the
greedy evaluation (success, return, length, discounted return) and gate_audit() on the offer states of a recorded greedy
evaluation, by value_fit_report.measure.

Per round one line per value function: fit and held-out samples, the CONT / BOOT / END items, the held-out RMS of the frozen-policy
TD residual before and after the solve, the held-out RMSE and mean error against the Monte-Carlo targets before and after,
|Delta|, the solve's relative residual and the share of samples whose greedy next action changed from the round before.

    python tools/lstdq_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--envs 8192] [--options 5] [--episodes 4096] [--rounds 3]
"""
import argparse, os
import rig
from value_fit_report import fmt_fit, measure


def fmt_lstdq(rnd):
    """One line per value function of one round of a fit_values_lstdq() report."""
    out = ["    vf      n_fit n_held    CONT   BOOT    END    td_old    td_new    mc_old    mc_new  bias_old  bias_new   |Delta|  residual  a'_moved"]
    for k, r in rnd["vf"].items():
        f, h, kd = r["fit"], r["held_out"], r["kinds"]
        moved = "-" if r["a_changed"] is None else f"{r['a_changed']:.4f}"
        out.append(f"    vf {k:2d} {f['td']['old']['n']:7d} {h['td']['old']['n']:6d} {kd['CONT']:7d} {kd['BOOT']:6d} {kd['END']:6d} "
                   f"{h['td']['old']['rmse']:9.2f} {h['td']['new']['rmse']:9.2f} {h['mc']['old']['rmse']:9.2f} {h['mc']['new']['rmse']:9.2f} "
                   f"{h['mc']['old']['mean_error']:9.2f} {h['mc']['new']['mean_error']:9.2f} {r['delta_norm']:9.3f} {r['solve_residual']:9.2e} {moved:>9s}")
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
    ap.add_argument("--episodes", type=int, default=4096, help="recorded episodes of the fits (half fitted, half held out)")
    ap.add_argument("--epsilon", type=float, default=0.1); ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--rounds", type=int, default=3, help="rounds of least-squares policy iteration on the one sample set")
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r23_lstdq_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# lstdq_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} states {a.states} "
                 f"episodes {a.episodes} epsilon {a.epsilon} ridge {a.ridge} rounds {a.rounds} hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            ag.rollout(a.warm)
            created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)

            def emit(out):
                for ln in out:
                    print(ln, flush=True)
                lines.extend(out)

            emit([f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}"] + measure(ag, a, seed, "before"))
            trained = ag.W.clone()
            report, _ = ag.fit_values_lstdq(n_episodes=a.episodes, epsilon=a.epsilon, seed=seed + 100, ridge=a.ridge, rounds=a.rounds)
            solves = report["solve_seconds"]
            for r, rnd in enumerate(report["rounds"]):
                ag.W.copy_(rnd["W"])
                emit([f"  lstdq round {r + 1}: {a.episodes} episodes at epsilon {a.epsilon}, success {report['episodes']['success_rate']:.4f}, "
                      f"solves {sum(solves) / len(solves):.2f} s each"] + fmt_lstdq(rnd) + measure(ag, a, seed, f"lstdq {r + 1}"))
            ag.W.copy_(trained)                                # the comparison: one Monte-Carlo fit of the trained weights on the same episodes
            fit, _ = ag.fit_values_to_returns(n_episodes=a.episodes, epsilon=a.epsilon, seed=seed + 100, ridge=a.ridge, apply=True)
            emit([f"  mc fit: {a.episodes} episodes at epsilon {a.epsilon}, success {fit['episodes']['success_rate']:.4f}"]
                 + fmt_fit(fit) + measure(ag, a, seed, "mc fit"))
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r23_lstdq_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
