"""Does each discovered initiation set hold the states its option succeeds from? (SkillChainingAgent.initiation_report)

Runs the discovery of tools/chain_evidence.py once (warm-up step-batches, chain_skills(), more step-batches), then for every
created option k trials of k (greedy, SPEC §9) from n_states free positions at rest, and prints per option: the classifier's
prediction in_k(s0) against trial success (TP / FP / FN / TN, precision, recall, the success rate inside and outside the
predicted set) and the outcome histogram. A low success rate INSIDE the predicted set with a high recall points at the option's
policy; successes OUTSIDE it (FN) or a low precision at the classifier.

    python tools/initiation_report.py [--envs 8192] [--options 5] [--seed 1] [--n-states 8192]
"""
import argparse, json
import rig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default="pinball_simple"); ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--options", type=int, default=5); ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--n-states", type=int, default=8192)
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)
    print(f"# initiation_report map {a.map} envs {a.envs} options {a.options} seed {a.seed} warm {a.warm} after {a.after} "
          f"n_states {a.n_states} hparams {HP}", flush=True)
    ag = SkillChainingAgent(a.map, a.envs, a.options, seed=a.seed, **HP)
    ag.enable_tracing(64)
    ag.rollout(a.warm)
    created = ag.chain_skills(steps_per_option=400, min_examples=3000, max_examples=40000, start_coverage=0.9)
    ag.rollout(a.after)
    for r in created:
        print("created", {k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}, flush=True)
    ev = ag.evaluate(n_episodes=4096)
    print("evaluate", json.dumps({k: ([round(x, 4) for x in v] if isinstance(v, list) else round(v, 4)) for k, v in ev.items()}), flush=True)
    for r in created:
        k = r["option"]
        rep = ag.initiation_report(k, n_states=a.n_states, seed=a.seed)
        s = rep["trials"].summary().get(k, {})
        row = {f: (round(v, 4) if isinstance(v, float) else v) for f, v in rep.items() if f not in ("trials", "predicted", "states")}
        row["mean_steps_success"] = round(s.get("mean_steps_success", float("nan")), 2)
        row["mean_disc_ret"] = round(s.get("mean_disc_ret", float("nan")), 2)
        print("report", json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
