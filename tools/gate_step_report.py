"""Do the options get used once the value gate compares something else (SPEC §25.4)? For each map and seed,
tools/policy_step_report.py's chain — warm-up step-batches, chain_skills(), more step-batches — and then ONE improve_gate() step
from that trained agent: fit_gate's regression of "what entering is worth" on the offer states of a recorded evaluation, and the
candidate gate tables — SPEC §4.2's own comparison ("shipped"), "always", "never", each fitted option's row alone, "all" — evaluated
greedy and at epsilon = 0.1 in ONE population rollout on common random numbers.

Per chain: the fit's held-out lines per option (states, RMSE of u_k . phi against the branch difference, the agreement of its sign
and of the shipped gate with "entering paid"), then per candidate and epsilon the success rate, the mean return, length and
discounted return, the paired difference of the discounted return against "shipped" +- its standard error, and per option the
entries, the declines and the share of steps it ran: whether the options get used is the point. The last line is what
initfit.choose_table decides at the first epsilon.

    python tools/gate_step_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--out-dir profiles]
"""
import argparse, os, sys, time
import rig


def fmt_fit(fit):
    out = [f"    fit: {fit['n_states']} offer states x {fit['replicates']} paired branches at epsilon {fit['epsilon']:.2f}, ridge {fit['ridge']:g}",
           "    option      n  n_fit n_held fitted  mean_delta       rmse  agree(fitted) agree(shipped)"]
    for r in fit["options"]:
        out.append(f"    {r['option']:6d} {r['n']:6d} {r['n_fit']:6d} {r['n_held']:6d} {str(r['fitted']):>6} {r['mean_delta']:11.2f} {r['rmse']:10.2f} "
                   f"{r['agreement_fitted']:14.3f} {r['agreement_shipped']:14.3f}")
    return out


def fmt_candidates(report):
    out = ["     label  eps  success     return   length  discounted   paired d(discounted) +-      se   per option k >= 1: entries / declines / steps_share"]
    for r in report["candidates"]:
        s, p = r["summary"], r["paired"]["disc_final"]
        per = "  ".join(f"{k}: {s['entries'][k]}/{s['declines'][k]}/{s['steps_share'][k]:.3f}" for k in range(1, len(s["entries"])))
        out.append(f"    {r['label']:>7} {r['epsilon']:4.2f} {s['success_rate']:8.4f} {s['mean_return']:10.2f} {s['mean_length']:8.1f} "
                   f"{s['mean_discounted_return']:11.2f} {p['mean_diff']:22.2f} +- {p['se']:7.2f}   {per}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--record-envs", type=int, default=256); ap.add_argument("--states", type=int, default=4096)
    ap.add_argument("--replicates", type=int, default=4); ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--ridge", type=float, default=1e-3); ap.add_argument("--min-offers", type=int, default=256)
    ap.add_argument("--eval-epsilons", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--criterion", default="discounted"); ap.add_argument("--z", type=float, default=2.0)
    ap.add_argument("--eval-episodes", type=int, default=4096)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r31_gate_step_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# gate_step_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} record_envs {a.record_envs} "
                 f"states {a.states} replicates {a.replicates} epsilon {a.epsilon} ridge {a.ridge} min_offers {a.min_offers} "
                 f"eval_epsilons {a.eval_epsilons} criterion {a.criterion} z {a.z} eval_episodes {a.eval_episodes} hparams {HP}"]
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
            if not created:
                say("  no option: nothing to gate")
                continue
            t0 = time.time()
            rep, _ = ag.improve_gate(eval_epsilons=a.eval_epsilons, criterion=a.criterion, z=a.z, n_eval=a.eval_episodes,
                                     n_record=a.record_envs, n_states=a.states, replicates=a.replicates, epsilon=a.epsilon,
                                     ridge=a.ridge, min_offers=a.min_offers, seed=seed + 100)
            say(f"  one improve_gate step: {len(rep['candidates'])} policies x {a.eval_episodes} episodes in one evaluation, {time.time() - t0:.1f} s")
            for ln in fmt_fit(rep["fit"]) + fmt_candidates(rep):
                say(ln)
            say(f"  the rule chooses: {rep['chosen']} ({'accepted' if rep['accepted'] else 'the shipped gate is kept'})")
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r31_gate_step_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
