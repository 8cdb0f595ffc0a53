"""Recorded episodes of a discovered chain (SkillChainingAgent.record_episodes, SPEC §10): where the agent enters an option,
where the value gate turns it away, where and why each option ends, which path the ball takes.

Discovers a chain as tools/initiation_report.py does (warm-up step-batches, chain_skills(), more step-batches), or loads a
checkpoint saved with SkillChainingAgent.save (--load; the map, env count and option count must match it), then records
--episodes greedy episodes (from drawn start states, or with --free-starts from free positions at rest) and prints one line per
episode, e.g. `root×12 → 3×40 SUCCESS → 2×31 SUCCESS → 1×9 EPISODE_END(goal)` (the count includes the begin row; a declined
offer stays in the root's run; `out` counts the episode's rows with a negative option id: steps that end outside an option
whose set holds the next state, declined by the value gate or not re-offered yet), then Trajectory.summary(). --out writes every row to an .npz
(Trajectory.to_numpy(): the fields concatenated over episodes, `offsets` per episode). --interrupt records interrupting
episodes (SPEC §11): a running option is cut short where the root's value is higher, shown as `INTERRUPTED`.

    python tools/trajectories.py [--envs 8192] [--options 5] [--seed 1] [--episodes 64] [--load ckpt.pt] [--out traj.npz]
                                [--interrupt]
"""
import argparse, json
import rig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default="pinball_simple"); ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--options", type=int, default=5); ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warm", type=int, default=3000); ap.add_argument("--after", type=int, default=1000)
    ap.add_argument("--episodes", type=int, default=64); ap.add_argument("--free-starts", action="store_true")
    ap.add_argument("--load", default=None); ap.add_argument("--out", default=None)
    ap.add_argument("--print", type=int, default=32, help="episode lines to print")
    ap.add_argument("--interrupt", action="store_true", help="interrupting episodes (SPEC §11)")
    a = ap.parse_args()
    import numpy as np
    from skill_chaining_with_graphs_amd import SkillChainingAgent
    HP = rig.discovery_hp(a.envs)
    print(f"# trajectories map {a.map} envs {a.envs} options {a.options} seed {a.seed} warm {a.warm} after {a.after} "
          f"episodes {a.episodes} free_starts {a.free_starts} load {a.load} interrupt {a.interrupt} hparams {HP}", flush=True)
    ag = SkillChainingAgent(a.map, a.envs, a.options, seed=a.seed, **HP)
    if a.load:
        ag.load(a.load)
    else:
        ag.enable_tracing(64)
        ag.rollout(a.warm)
        created = ag.chain_skills(steps_per_option=400, min_examples=3000, max_examples=40000, start_coverage=0.9)
        ag.rollout(a.after)
        for r in created:
            print("created", {k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}, flush=True)
    states = None
    if a.free_starts:
        pos = ag.map.sample_free(a.episodes, np.random.default_rng(a.seed))
        states = (pos[:, 0], pos[:, 1])
    tr, ev = ag.record_episodes(n_episodes=a.episodes, states=states, seed=a.seed, interrupt=a.interrupt)
    print("evaluate", json.dumps({k: ([round(x, 4) for x in v] if isinstance(v, list) else round(v, 4)) for k, v in ev.items()}),
          flush=True)
    for i in range(min(a.print, tr.n)):
        e = tr.per_env(i)
        print(f"episode {i:4d} start ({e['x'][0]:.3f}, {e['y'][0]:.3f}) out {int(np.sum(e['option_id'] < 0))}: "
              f"{tr.describe(i)}", flush=True)
    s = tr.summary()
    print("summary", json.dumps({k: ([round(x, 3) if isinstance(x, float) else x for x in v] if isinstance(v, list) else
                                     (round(v, 4) if isinstance(v, float) else v)) for k, v in s.items()}), flush=True)
    if a.out:
        np.savez_compressed(a.out, **tr.to_numpy())
        print("wrote", a.out, flush=True)


if __name__ == "__main__":
    main()
