"""Does the initiation classifier's capacity cost held-out accuracy (SPEC §23.4)? For each map and seed, tools/gate_audit_report.py's
protocol trains an agent and discovers its chain; then, per enabled option k, greedy trials of k label two state sets of --states
states — (a) free positions at rest, (b) full states with their velocities, drawn from the rows of recorded epsilon = 0.1 episodes on
which the episode went on — and on each set these classifiers are fitted on the even-indexed states and judged on the odd-indexed
ones: the shipped in_k (SPEC §4.1, as discovered: not refitted), SPEC §6's quadratic refitted on the same labels from the shipped row
(scg_fit_initiation), and SkillChainingAgent.fit_initiation_fourier with "position" features at the orders 3 / 5 / 7 and "state"
features at the orders 3 / 5. One line per classifier: held-out accuracy, precision, recall, log-loss (the quadratics' from
ScgContext.classifier_logits, SPEC §24.2), the fit half's accuracy, and the fit's iterations and reason. Nothing acts with a fitted
classifier: every trial ran with the shipped in_k.

    python tools/initiation_capacity_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--envs 8192] [--options 5] [--states 8192]
                                               [--out-dir profiles]
"""
import argparse
import os

import rig

FOURIER = (("position", 3), ("position", 5), ("position", 7), ("state", 3), ("state", 5))


def episode_states(traj, limit, seed):
    """(x, y, vx, vy) of `limit` recorded rows on which the episode went on, drawn without replacement with `seed` (all, if fewer)."""
    import numpy as np
    r = traj.to_numpy()
    at = np.nonzero(r["done"] == 0)[0]
    if len(at) > limit:
        at = np.sort(np.random.default_rng(seed).choice(at, limit, replace=False))
    return tuple(np.ascontiguousarray(r[f][at], np.float32) for f in ("x", "y", "vx", "vy"))


def fmt_row(name, held, fit, extra=""):
    ll = f"{held['log_loss']:8.4f}" if held["log_loss"] == held["log_loss"] else "       -"
    return (f"      {name:<22} acc {held['accuracy']:6.4f}  prec {held['precision']:6.4f}  rec {held['recall']:6.4f}  log-loss {ll}  "
            f"fit-half acc {fit['accuracy']:6.4f}  {extra}")


def quadratic_refit(ag, k, rep, iters, lr, l2):
    """SPEC §6's fit of one row on the even-indexed states' labels, from the shipped row, on the trial context
    (initfit.refit_quadratic): (held-out, fit-half) classification_stats of the refitted quadratic. clf is not written."""
    import torch
    from skill_chaining_with_graphs_amd import _lib, initfit
    xs, ys = rep["states"][0], rep["states"][1]
    ok = (rep["trials"].outcome == _lib.TRIAL_SUCCESS)
    w = initfit.refit_quadratic(ag._trial_ctx, ag.clf[k], torch.stack((xs[0::2], ys[0::2]), 1), ok[0::2], iters, lr, l2)
    return quadratic_stats(ag, w, xs, ys, ok.cpu().numpy())


def quadratic_stats(ag, w8, xs, ys, ok):
    """(held-out, fit-half) classification_stats of the row w8 on the states (xs, ys), its log-loss from its logits (SPEC §24.2)."""
    from skill_chaining_with_graphs_amd import initfit
    tc = ag._trial_ctx
    w8 = w8.contiguous()
    pred = tc.classifier_predict(xs, ys, w8).cpu().numpy()
    z = tc.classifier_logits(xs, ys, w8).cpu().numpy()
    return initfit.classification_stats(pred[1::2], ok[1::2], z[1::2]), initfit.classification_stats(pred[0::2], ok[0::2], z[0::2])


def option_lines(ag, k, states, a):
    from skill_chaining_with_graphs_amd import initfit
    rep = ag.initiation_report(k, states, n_states=a.states, seed=a.label_seed)
    ok = rep["trials"].outcome.cpu().numpy() == 1
    out = [f"    option {k}: {rep['n']} states, {int(ok.sum())} successes ({ok.mean():.4f}); outcomes {rep['outcomes']}"]
    if ok[0::2].all() or not ok[0::2].any():
        return out + ["      the fit half holds one class only: nothing to fit"]
    out.append(fmt_row("shipped in_k", *quadratic_stats(ag, ag.clf[k], rep["states"][0], rep["states"][1], ok)))
    held, fit = quadratic_refit(ag, k, rep, a.iters, a.lr, a.l2)
    out.append(fmt_row("quadratic refitted", held, fit, f"({a.iters} iterations of scg_fit_initiation)"))
    for features, order in FOURIER:
        clf, r = ag.fit_initiation_fourier(k, order=order, features=features, ridge=a.ridge, trials=rep)
        out.append(fmt_row(f"{features} order {order}", r["held_out"]["fourier"], r["fit"]["fourier"],
                           f"({r['iterations']} iterations, {r['reason']}, {int(initfit.feature_mask(order, features).sum())} weights)"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--states", type=int, default=8192); ap.add_argument("--record-envs", type=int, default=256)
    ap.add_argument("--label-seed", type=int, default=0); ap.add_argument("--ridge", type=float, default=1e-3)
    ap.add_argument("--iters", type=int, default=400); ap.add_argument("--lr", type=float, default=3.0); ap.add_argument("--l2", type=float, default=1e-4)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r29_initiation_capacity_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)
    for mp in a.maps:
        lines = [f"# initiation_capacity_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} states {a.states} "
                 f"ridge {a.ridge} held-out = the odd-indexed states; hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            ag.rollout(a.warm)
            created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)
            out = [f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}; fit accuracies of chain_skills "
                   f"{[round(float(c.get('accuracy', float('nan'))), 3) for c in created]}"]
            enabled = [k for k in range(1, a.options + 1) if (ag.enabled_mask >> k) & 1]
            traj, _ = ag.record_episodes(n_episodes=a.record_envs, epsilon=0.1)
            met = episode_states(traj, a.states, seed)
            for title, states in ((f"(a) {a.states} free positions at rest", None),
                                  (f"(b) {len(met[0])} states of {a.record_envs} recorded epsilon = 0.1 episodes, with velocities", met)):
                out.append(f"  {title}")
                for k in enabled:
                    out += option_lines(ag, k, states, a)
            for ln in out:
                print(ln, flush=True)
            lines += out
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r29_initiation_capacity_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
