"""Does acting with refitted initiation classifiers change what a discovered chain does (SPEC §24.3)? For each map and seed,
tools/policy_step_report.py's chain — warm-up step-batches, chain_skills(), more step-batches — and then ONE
improve_initiation(apply=False) step from that trained agent: every enabled option's row refitted on trial labels, the shipped table,
each single-row candidate and the table of all refitted rows evaluated at every epsilon in ONE population rollout on common random
numbers under the agent's W, and the decision of §21.4's rule at eval_epsilons[0].

Per option: the held-out (odd-indexed states) accuracy, precision, recall and log-loss of the shipped and the refitted row. Per
candidate and epsilon: success rate, mean return, mean length, mean discounted return, the paired difference of the discounted
return against the shipped table at the same epsilon +- its standard error, and per value function the entries and the share of
the steps. Then the fixed-point lines: each option's trial success rate under the shipped table and under the table of all
refitted rows, on the same states.

    python tools/initiation_step_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--out-dir profiles]
"""
import argparse, os, sys, time
import rig


def fmt_options(report):
    out = []
    for o in report["options"]:
        head = f"    option {o['option']}: {o['n']} states, {o['successes']} successes; outcomes {o['outcomes']}"
        if o["skipped"]:
            out.append(f"{head}; skipped: {o['skipped']}")
            continue
        out.append(head)
        for who in ("shipped", "refitted"):
            s = o[who]
            out.append(f"      {who:<9s} held-out acc {s['accuracy']:6.4f}  prec {s['precision']:6.4f}  rec {s['recall']:6.4f}  log-loss {s['log_loss']:8.4f}")
    return out


def fmt_candidates(report):
    out = ["    table     eps  success     return   length  discounted   paired d(discounted) +-      se   entries per VF / share of the steps"]
    for r in report["candidates"]:
        s, p = r["summary"], r["paired"]["disc_final"]
        out.append(f"    {r['label']:<8s} {r['epsilon']:4.2f} {s['success_rate']:8.4f} {s['mean_return']:10.2f} {s['mean_length']:8.1f} "
                   f"{s['mean_discounted_return']:11.2f} {p['mean_diff']:22.2f} +- {p['se']:7.2f}   {s['entries']} / "
                   f"{[round(v, 3) for v in s['steps_share']]}")
    return out


def fmt_fixed_point(report):
    if not report["fixed_point"]:
        return ["    fixed point: no row was refitted"]
    out = []
    for f in report["fixed_point"]:
        out.append(f"    fixed point, option {f['option']}: trial success {f['shipped']['success_rate']:.4f} under the shipped table, "
                   f"{f['refitted']['success_rate']:.4f} under table '{f['table']}' (outcomes {f['refitted']['outcomes']})")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--states", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=400); ap.add_argument("--lr", type=float, default=3.0); ap.add_argument("--l2", type=float, default=1e-4)
    ap.add_argument("--eval-epsilons", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--criterion", default="discounted"); ap.add_argument("--z", type=float, default=2.0)
    ap.add_argument("--eval-episodes", type=int, default=4096)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r30_initiation_step_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# initiation_step_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} states {a.states} "
                 f"iters {a.iters} lr {a.lr} l2 {a.l2} eval_epsilons {a.eval_epsilons} criterion {a.criterion} z {a.z} "
                 f"eval_episodes {a.eval_episodes} hparams {HP}"]
        print(lines[0], flush=True)

        def say(ln):
            print(ln, flush=True)
            lines.append(ln)

        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            t_seed = time.time()
            ag.rollout(a.warm)
            created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)
            print(f"  (seed {seed}: chain trained, {time.time() - t_seed:.0f} s)", file=sys.stderr, flush=True)
            say(f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}")
            if not ag.enabled_mask & ~1:
                say("  no option is enabled: nothing to refit")
                continue
            t0 = time.time()
            rep, _ = ag.improve_initiation(n_states=a.states, iters=a.iters, lr=a.lr, l2=a.l2, eval_epsilons=a.eval_epsilons,
                                           criterion=a.criterion, z=a.z, n_eval=a.eval_episodes, seed=seed + 100)
            n_tab = len(rep["candidates"]) // len(a.eval_epsilons)
            say(f"  one step: {n_tab} tables x {len(a.eval_epsilons)} epsilons x {a.eval_episodes} episodes in one evaluation, {time.time() - t0:.1f} s; "
                f"the rule chooses '{rep['chosen']}' ({'accepted' if rep['accepted'] else 'the shipped table is kept'})")
            for ln in fmt_options(rep) + fmt_candidates(rep) + fmt_fixed_point(rep):
                say(ln)
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r30_initiation_step_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
