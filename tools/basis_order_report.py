"""Would a richer basis hold the return (SPEC §18)? For each map and seed, tools/value_fit_report.py's chain — warm-up
step-batches, chain_skills(), more step-batches — and ONE recorded trajectory of --episodes episodes at --epsilon. That record is
fitted at every order of --orders by fit_values_to_returns(order=p, trajectory=...): the same samples, targets and fit / held-out
split, the residual y - Q^old regressed on the (p + 1)^4 features of order p, the agent's own order-5 values as Q^old. Nothing is
applied: the agent acts at order 5 throughout.

Per value function and order one line: fit and held-out samples, RMSE of Q^old and Q^new on the fit half and on the held-out half,
the held-out mean error old and new, |Delta|. The held-out RMSE is the number that counts; a fit RMSE that falls with the order
while the held-out RMSE does not is over-fitting at this sample size.

    python tools/basis_order_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--orders 3 5 7] [--episodes 4096]
"""
import argparse, os, sys, time
import rig


def fmt_orders(reports):
    """One line per value function and order of fit_values_to_returns(order=p) reports on one record."""
    out = ["    vf order features   n_fit n_held   fit_old   fit_new  held_old  held_new  bias_old  bias_new   |Delta|"]
    for k in sorted({k for r in reports for k in r["vf"]}):
        for r in reports:
            v = r["vf"][k]
            f, h = v["fit"], v["held_out"]
            out.append(f"    vf {k:2d} {r['order']:5d} {r['features']:8d} {f['old']['n']:7d} {h['old']['n']:6d} {f['old']['rmse']:9.2f} "
                       f"{f['new']['rmse']:9.2f} {h['old']['rmse']:9.2f} {h['new']['rmse']:9.2f} {h['old']['mean_error']:9.2f} "
                       f"{h['new']['mean_error']:9.2f} {v['delta_norm']:9.3f}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--orders", type=int, nargs="+", default=[3, 5, 7])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--episodes", type=int, default=4096, help="recorded episodes (half fitted, half held out)")
    ap.add_argument("--epsilon", type=float, default=0.1); ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r24_basis_order_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# basis_order_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} episodes {a.episodes} "
                 f"epsilon {a.epsilon} ridge {a.ridge} orders {a.orders} hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            note = lambda what: print(f"  (seed {seed}: {what}, {time.time() - t_seed:.0f} s)", file=sys.stderr, flush=True)
            t_seed = time.time()
            ag.rollout(a.warm)
            note("warm-up done")
            created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)
            note("chain trained")
            traj, summary = ag.record_episodes(a.episodes, epsilon=a.epsilon, seed=seed + 100)
            note("episodes recorded")
            out = [f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}; one record of {a.episodes} episodes at epsilon "
                   f"{a.epsilon}, success {summary['success_rate']:.4f}, {int(traj.to_numpy()['offsets'][-1])} rows"]
            reports = []
            for p in a.orders:
                t0 = time.time()
                rep, _ = ag.fit_values_to_returns(epsilon=a.epsilon, seed=seed + 100, ridge=a.ridge, order=p, trajectory=traj)
                reports.append(rep)
                out.append(f"  order {p}: {rep['features']} features, fitted in {time.time() - t0:.1f} s")
            out += fmt_orders(reports)
            for ln in out:
                print(ln, flush=True)
            lines += out
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r24_basis_order_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
