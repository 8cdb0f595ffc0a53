"""Diagnostic: does the batched root Q-learning actually learn Pinball? Prints goal arrivals per 1000 env-steps during training
and, beside them, the greedy policy's success rate and mean episode length from SkillChainingAgent.evaluate() (SPEC §8)."""
import argparse
import rig  # noqa: F401  (puts the repository root on sys.path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default="pinball_simple"); ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--alpha", type=float, default=0.02); ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--gamma", type=float, default=0.99); ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--chunk", type=int, default=500); ap.add_argument("--maxep", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--eval-episodes", type=int, default=4096, help="episodes of each evaluate() (0: no evaluation column)")
    a = ap.parse_args()
    import torch
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    ag = SkillChainingAgent(a.map, a.envs, 0, seed=a.seed, alpha=a.alpha, epsilon=a.eps, gamma=a.gamma, max_episode_steps=a.maxep)
    print(f"# learning_curve map {a.map} envs {a.envs} alpha {a.alpha} eps {a.eps} gamma {a.gamma} seed {a.seed}", flush=True)
    for it in range(a.iters):
        goals = torch.zeros((), device="cuda"); touts = torch.zeros((), device="cuda")
        for _ in range(a.chunk):
            ag.step_batch()
            goals += (ag.state.done == 1).sum(); touts += (ag.state.done == 2).sum()
        g, t = int(goals), int(touts)
        ev = ""
        if a.eval_episodes:
            r = ag.evaluate(n_episodes=a.eval_episodes)
            ev = f"  eval success {r['success_rate']:6.3f}  mean length {r['mean_length']:7.1f}"
        print(f"iter {it:3d}  goals/1k env-steps {1000*g/(a.chunk*a.envs):7.3f}  timeouts {t:6d}  |W|max {float(ag.W.abs().max()):9.3f}{ev}", flush=True)


if __name__ == "__main__":
    main()
