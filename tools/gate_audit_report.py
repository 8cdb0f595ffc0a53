"""Does the value gate decide right (SPEC §15)? For each map and seed, tools/chain_evidence.py's protocol trains an agent
(warm-up step-batches, chain_skills(), more step-batches); then gate_audit() runs, from each of up to --states start states, one
greedy episode FORCED to enter the state's lowest-numbered candidate option and one forced to decline it, with the same random
numbers afterwards, and compares the two realised discounted task returns with each other and with what V_k and V_0 promised.
The states are drawn two ways: (a) free positions at rest; (b) states where offers actually happen: rows of a recorded greedy
evaluation on which the root ran, the episode went on and an option was offered or stayed out of (vf = 0, done = 0,
option_id != 0), with their velocities.

One line per option and one for all: states audited, the gate's enter rate, mean V_k and V_0, mean realised G_enter and G_decline,
their mean difference, the share of states where the gate's decision equals G_enter >= G_decline, the mean return the gate's
decision gives away, the calibration errors mean(V_k - G_enter) and mean(V_0 - G_decline), and both branches' goal rates.

    python tools/gate_audit_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--envs 8192] [--options 5] [--states 4096]
"""
import argparse, os
import rig

COLS = (("n", "n", "{:6d}"), ("enter_rate", "enter", "{:6.3f}"), ("mean_v_k", "V_k", "{:9.2f}"), ("mean_v_0", "V_0", "{:9.2f}"),
        ("mean_g_enter", "G_enter", "{:9.2f}"), ("mean_g_decline", "G_decl", "{:9.2f}"), ("mean_advantage", "adv", "{:9.2f}"),
        ("agreement", "agree", "{:6.3f}"), ("regret", "regret", "{:8.2f}"), ("calib_enter", "V_k-G_e", "{:9.2f}"),
        ("calib_decline", "V_0-G_d", "{:9.2f}"), ("goal_rate_enter", "goal_e", "{:6.3f}"), ("goal_rate_decline", "goal_d", "{:6.3f}"))


def fmt_audit(res):
    """The table of a gate_audit() result: a header, one line per option, one for all."""
    width = [len(fmt.format(0)) for _, _, fmt in COLS]
    out = ["    option " + " ".join(h.rjust(w) for (_, h, _), w in zip(COLS, width))]
    for name, row in [(str(k), r) for k, r in res["options"].items()] + [("all", res["overall"])]:
        out.append(f"    {name:>6} " + " ".join(fmt.format(row[key]) for key, _, fmt in COLS))
    return out


def offer_states(traj, limit):
    """(x, y, vx, vy) of the recorded rows where the root ran, the episode went on and an option was offered or stayed out of:
    the first `limit` of them in env order (trajectory.offer_states has the selection; Trajectory.offer_states is this)."""
    from skill_chaining_with_graphs_amd.trajectory import offer_states as select
    return select(traj.to_numpy(), limit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--states", type=int, default=4096, help="start states audited, at most, per way of drawing them")
    ap.add_argument("--record-envs", type=int, default=256, help="recorded greedy episodes the offer states are taken from")
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r20_gate_audit_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)

    for mp in a.maps:
        lines = [f"# gate_audit_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} states {a.states} "
                 f"greedy hparams {HP}"]
        print(lines[0], flush=True)
        for seed in a.seeds:
            ag = SkillChainingAgent(mp, a.envs, a.options, seed=seed, **HP)
            ag.enable_tracing(64)
            ag.rollout(a.warm)
            created = ag.chain_skills(steps_per_option=a.steps_per_option, min_examples=a.min_examples, max_examples=40000, start_coverage=0.9)
            ag.rollout(a.after)
            out = [f"seed {seed}: {len(created)} options, enabled mask {ag.enabled_mask:#x}",
                   f"  greedy      {rig.fmt_eval(ag.evaluate(n_episodes=a.states))}"]
            if created:
                rest = ag.gate_audit(n_states=a.states, seed=seed)
                out += [f"  (a) {a.states} free positions at rest: {rest['overall']['n']} have a candidate"] + fmt_audit(rest)
                traj, _ = ag.record_episodes(n_episodes=a.record_envs)
                states = offer_states(traj, a.states)
                if len(states[0]):
                    met = ag.gate_audit(states=states, seed=seed)
                    out += [f"  (b) {len(states[0])} offer states of {a.record_envs} recorded greedy episodes: "
                            f"{met['overall']['n']} have a candidate"] + fmt_audit(met)
                else:
                    out += [f"  (b) no offer state on {a.record_envs} recorded greedy episodes"]
            for ln in out:
                print(ln, flush=True)
            lines += out
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r20_gate_audit_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
