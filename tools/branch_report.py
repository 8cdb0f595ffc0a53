"""How much of a value function's error is noise, and is its greedy action the best one (SPEC §19)? For each map and seed,
tools/value_fit_report.py's chain — warm-up step-batches, chain_skills(), more step-batches — and ONE recorded trajectory of
--episodes episodes at --epsilon. On that record: fit_values_to_returns(trajectory=...) for §16's held-out RMSE before and after the
fit, and branch_audit(trajectory=...): from --states held-out rows per value function, --replicates branch rollouts of each of the
five first actions, resumed from the row's whole env state on fresh random streams. Nothing is applied to the agent.

Per value function one line: the states branched from, the held-out RMSE of Q^old and Q^new against the Monte-Carlo targets,
spread (the RMS within-state standard deviation of the return-to-go under the recorded action: the floor under any function of the
whole env state), rest = sqrt(max(RMSE_new^2 - spread^2, 0)) (what a better function of the state could still remove, if the floor
were a function of (x, y, vx, vy) alone), z2 and z2med (the record's own return against the replicates, mean and median of the
squared z-scores: for normal returns 1.4 and 0.5 at 8 replicates, where the resume is distributionally faithful; heavy-tailed),
var0 (states whose replicates all agree), and the action table: agree (a_W = argmax of the replicate means), gap (biased upwards by
the noise), gap_ho (the held-out, unbiased gain of a one-step improvement) and signif (states whose gap exceeds two standard errors).

    python tools/branch_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--episodes 4096] [--states 1024] [--replicates 8]
"""
import argparse, math, os, sys, time
import rig


def fmt_branch(fit, audit):
    """One line per value function of a fit_values_to_returns() report and a branch_audit() report on the same record."""
    out = ["    vf states  held_old  held_new    spread      rest       z2  z2med   var0   agree       gap    gap_ho signif"]
    for k, b in audit["vf"].items():
        if not b["n"]:
            out.append(f"    vf {k:2d}      0  (no held-out row)")
            continue
        h, s, t = fit["vf"][k]["held_out"], b["spread"], b["actions"]
        rest = math.sqrt(max(h["new"]["rmse"] ** 2 - s["spread_rmse"] ** 2, 0.0))
        out.append(f"    vf {k:2d} {b['n']:6d} {h['old']['rmse']:9.2f} {h['new']['rmse']:9.2f} {s['spread_rmse']:9.2f} {rest:9.2f} "
                   f"{s['recorded_z2']:8.2f} {s['recorded_z2_median']:6.2f} {s['zero_variance']:6.3f} {t['greedy_agreement']:7.3f} {t['gap']:9.2f} {t['gap_holdout']:9.2f} "
                   f"{t['significant']:6.3f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--episodes", type=int, default=4096, help="recorded episodes (half fitted, half held out)")
    ap.add_argument("--epsilon", type=float, default=0.1); ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--states", type=int, default=1024, help="held-out rows branched from, at most, per value function")
    ap.add_argument("--replicates", type=int, default=8)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r25_branch_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# branch_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} episodes {a.episodes} "
                 f"epsilon {a.epsilon} ridge {a.ridge} states {a.states} replicates {a.replicates} hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            note = lambda what: print(f"  (seed {seed}: {what}, {time.time() - t_seed:.0f} s)", file=sys.stderr, flush=True)
            t_seed = time.time()
            ag.rollout(a.warm)
            created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)
            note("chain trained")
            traj, summary = ag.record_episodes(a.episodes, epsilon=a.epsilon, seed=seed + 100)
            note("episodes recorded")
            fit, _ = ag.fit_values_to_returns(epsilon=a.epsilon, seed=seed + 100, ridge=a.ridge, trajectory=traj)
            note("values fitted")
            t0 = time.time()
            audit = ag.branch_audit(trajectory=traj, n_states=a.states, replicates=a.replicates, actions="all", epsilon=a.epsilon,
                                    seed=seed + 100)
            note("branches run")
            n_branch = sum(b["n"] for b in audit["vf"].values()) * 5 * a.replicates
            out = [f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}; one record of {a.episodes} episodes at epsilon "
                   f"{a.epsilon}, success {summary['success_rate']:.4f}, {int(traj.to_numpy()['offsets'][-1])} rows; {n_branch} branch "
                   f"episodes in {time.time() - t0:.1f} s"] + fmt_branch(fit, audit)
            for ln in out:
                print(ln, flush=True)
            lines += out
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r25_branch_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
