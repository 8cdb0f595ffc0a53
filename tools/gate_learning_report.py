"""Does a learner that TRAINS under another gate end elsewhere (SPEC §26.3)? For each map and seed, tools/policy_step_report.py's
chain — warm-up step-batches, chain_skills(), more step-batches — and then, from that one trained agent (its state_dict, restored
for every arm), --train learning step-batches per arm:

  shipped   the plain learner: SPEC §4.2's comparison on the W that is being learned
  always    set_learner_gate(gatefit.always_enter, every created option): every offer is entered
  fitted    fit_gate() at the start and again at half time; set_learner_gate(advantage_gate rows of the fitted options, those
            options only): the fitted options enter where u_k . phi(s_next) >= 0, every other option keeps §4.2's comparison

Every arm runs the same number of env-steps from the same tables (the fits run on evaluation contexts of their own). Per arm,
during training and per option: offers (entries + fresh declines; a stay is no offer), entries, and the share of env-steps the
option ran. After training: evaluate() at epsilon 0 and 0.1 on --eval-episodes episodes, under §4.2's own gate on the final W and
under the gate the arm trained with (the table's rows for the masked options, shipped_gate(W) for the others): success rate,
return, length, discounted return and the per-option step share.

    python tools/gate_learning_report.py [--maps pinball_simple pinball_maze] [--seeds 1 2] [--train 4000] [--out-dir profiles]
"""
import argparse, os, sys, time
import rig


def train(ag, steps, n_vf, reoffer):
    """`steps` learning step-batches; [3][n_vf] counts: offers, entries, env-steps run per option."""
    import torch
    dev = ag.ctx.device
    cnt = torch.zeros((3, n_vf), dtype=torch.int64, device=dev)
    env = torch.arange(ag.n_envs, device=dev, dtype=torch.int64) + int(ag.ctx.cfg.env_id_base)
    ks = torch.arange(n_vf, device=dev).view(-1, 1)
    for _ in range(steps):
        prev, t = ag.state.option_id.clone(), int(ag.t)
        ag.step_batch()
        now, done = ag.state.option_id, ag.state.done
        due = ((env + t) % max(reoffer, 1)) == 0
        entered = (now > 0) & (now != prev)
        fresh = (now < 0) & ((now != prev) | due | (done != 0))           # a decline of this step (a stay keeps its id and is not due)
        cnt[1] += ((now == ks) & entered).sum(1)
        cnt[0] += ((now == ks) & entered).sum(1) + ((-now == ks) & fresh).sum(1)
        cnt[2] += (prev == ks).sum(1)
    return cnt.cpu().numpy()


def fmt_train(cnt, steps, n):
    per = "  ".join(f"{k}: {cnt[0][k]}/{cnt[1][k]}/{cnt[2][k] / (steps * n):.3f}" for k in range(1, cnt.shape[1]))
    return f"    training, per option k >= 1: offers / entries / step share   {per}   (options' share {cnt[2][1:].sum() / (steps * n):.3f})"


def fmt_eval(label, eps, s):
    share = " ".join(f"{v:.3f}" for v in s["steps_share"][1:])
    return (f"    {label:>14} eps {eps:4.2f} success {s['success_rate']:.4f} return {s['mean_return']:9.2f} length {s['mean_length']:7.1f} "
            f"discounted {s['mean_discounted_return']:9.2f}  options' share {sum(s['steps_share'][1:]):.3f} [{share}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", nargs="+", default=["pinball_simple", "pinball_maze"])
    ap.add_argument("--envs", type=int, default=8192); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--steps-per-option", type=int, default=400); ap.add_argument("--min-examples", type=int, default=3000)
    ap.add_argument("--train", type=int, default=4000, help="learning step-batches per arm")
    ap.add_argument("--record-envs", type=int, default=256); ap.add_argument("--states", type=int, default=4096)
    ap.add_argument("--replicates", type=int, default=4); ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--ridge", type=float, default=1e-3); ap.add_argument("--min-offers", type=int, default=256)
    ap.add_argument("--eval-epsilons", type=float, nargs="+", default=[0.0, 0.1])
    ap.add_argument("--eval-episodes", type=int, default=4096)
    ap.add_argument("--out-dir", default=None, help="also write one report per map: <dir>/r32_gate_learning_<map>.txt")
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent, gatefit
    HP = rig.discovery_hp(a.envs)
    n_vf = a.options + 1

    for mp in a.maps:
        lines = [f"# gate_learning_report map {mp} envs {a.envs} options {a.options} warm {a.warm} after {a.after} train {a.train} "
                 f"record_envs {a.record_envs} states {a.states} replicates {a.replicates} epsilon {a.epsilon} ridge {a.ridge} "
                 f"min_offers {a.min_offers} eval_epsilons {a.eval_epsilons} eval_episodes {a.eval_episodes} hparams {HP}"]
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
            if not created:
                say("  no option: nothing to gate")
                continue
            opts = [k for k in range(1, n_vf) if (ag.enabled_mask >> k) & 1]
            trained = ag.state_dict()

            def fit():
                rep, u = ag.fit_gate(n_record=a.record_envs, n_states=a.states, replicates=a.replicates, epsilon=a.epsilon,
                                     ridge=a.ridge, min_offers=a.min_offers, seed=seed + 100)
                if u:
                    ag.set_learner_gate(gatefit.advantage_gate(gatefit.always_enter(n_vf), u), options=sorted(u))
                else:                                          # nothing fitted: the plain learner
                    ag.set_learner_gate(None)
                return sorted(int(k) for k in u)

            for arm in ("shipped", "always", "fitted"):
                ag.load_state_dict(trained)
                ag.set_learner_gate(None)
                halves = [a.train // 2, a.train - a.train // 2]
                fitted = []
                if arm == "always":
                    ag.set_learner_gate(gatefit.always_enter(n_vf), options=opts)
                cnt = 0
                for h, steps in enumerate(halves):
                    if arm == "fitted":
                        fitted.append(fit())
                    cnt = cnt + train(ag, steps, n_vf, HP["reoffer_period"])
                note(f"arm {arm} trained")
                say(f"  arm {arm}: {a.train} learning step-batches" + (f", fitted options at the start {fitted[0]}, at half time {fitted[1]}" if arm == "fitted" else "")
                    + f", gate mask {ag.learner_gate_mask:#x}")
                say(fmt_train(cnt, a.train, a.envs))
                own = None
                if ag.learner_gate is not None and ag.learner_gate_mask:
                    own = gatefit.shipped_gate(ag.W)
                    for k in range(1, n_vf):
                        if (ag.learner_gate_mask >> k) & 1:
                            own[k] = ag.learner_gate[k]
                for eps in a.eval_epsilons:
                    say(fmt_eval("§4.2's gate", eps, ag.evaluate(a.eval_episodes, epsilon=eps, seed=seed + 200, discounted=True, gate=None)))
                    if own is not None:
                        say(fmt_eval("its own gate", eps, ag.evaluate(a.eval_episodes, epsilon=eps, seed=seed + 200, discounted=True, gate=own)))
                note(f"arm {arm} evaluated")
            del ag
        if a.out_dir:
            os.makedirs(a.out_dir, exist_ok=True)
            with open(os.path.join(a.out_dir, f"r32_gate_learning_{mp}.txt"), "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
