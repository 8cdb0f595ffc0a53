"""Long determinism check: two agents with the same seeds stepped side by side must agree bit for bit (W, states, qcache) however
long the run is — short parity rollouts would not see a rare race. Prints the first step-batch at which they differ, if any.
   python tools/determinism_soak.py [steps]"""
import argparse, sys
import rig
from bench import HP


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("steps", type=int, nargs="?", default=3000)
    steps = ap.parse_args().steps
    import torch
    cases = [("8192 envs, root only, alpha 0.02 (the warm-up of tools/chain_evidence.py)", 8192, 0, dict(alpha=0.02, epsilon=0.05, gamma=0.99, max_episode_steps=2000, max_option_steps=200, r_option_success=10000.0)),
             ("65536 envs, root + 5 options (the bench workload)", 65536, 5, dict(HP)),
             ("5000 envs, root + 3 options, ragged last block", 5000, 3, dict(HP, alpha=0.01))]
    bad = 0
    for name, n, nopt, hp in cases:
        ags = [rig.headline_agent(n, nopt, seed=1, hp=hp, reset_seed=1001) for _ in range(2)]
        first = None
        for t in range(steps):
            for ag in ags:
                ag.step_batch()
            if (t + 1) % 100 == 0 or t == steps - 1:
                same = torch.equal(ags[0].W, ags[1].W) and all(torch.equal(getattr(ags[0].state, k), getattr(ags[1].state, k))
                                                                for k in ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "qcache", "action"))
                if not same:
                    first = t + 1
                    break
        goals = int((ags[0].state.done == 1).sum())
        print(f"{name}: {steps} step-batches x 2 agents: " + ("bit-identical throughout" if first is None else f"DIFFER by step-batch {first}")
              + f"; async status {ags[0].ctx.async_status(True)}; goals in the last step-batch {goals}", flush=True)
        bad += first is not None
        del ags
        torch.cuda.empty_cache()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
