"""Option trials (SPEC §9, one scg_option_trials launch) against the composition they equal: Q_k(s0, .) per option, then acting
scg_step(flags = 0) calls until the longest trial has ended.

Workload: root + a 5-option chain (chain classifiers, all enabled), bench-like weights (std 1e-3), 65 536 start states (random
free positions and velocities), option k = 1 + (i mod 5) for entry i, max_option_steps = 250. The two sides are warmed up and
timed alternately; the line gives the medians over the rounds (ms per batch of trials) and the step count of the longest trial.

With --record ROWS the trials are also timed with every step recorded (SPEC §10, ROWS rows per entry), in the same alternation.

    python tools/trial_bench.py [--n 65536] [--rounds 5] [--max-option-steps 250] [--record 250]
"""
import argparse
import json

import rig


def bench(n, rounds, max_opt, n_opt=5, rows=0):
    import numpy as np
    import torch
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd.core import EnvState, ScgContext
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    from skill_chaining_with_graphs_amd.trials import TrialResult
    _time = lambda fn: rig.timed(fn, 1)
    m = scg.load_map("pinball_simple")
    ctx = ScgContext(n, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000, max_option_steps=max_opt)
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    clf = torch.as_tensor(rig.chain_classifiers(m, n_opt), device=ctx.device).view(-1)
    g = torch.Generator().manual_seed(3)
    W = (torch.randn((n_opt + 1) * 5 * 1296, generator=g) * 1e-3).to(ctx.device)
    rng = np.random.default_rng(1)
    pos = m.sample_free(n, rng, margin=2.0)
    v = rng.uniform(-1.0, 1.0, (n, 2)).astype(np.float32)
    s0 = [torch.as_tensor(np.ascontiguousarray(a, np.float32), device=ctx.device) for a in (pos[:, 0], pos[:, 1], v[:, 0], v[:, 1])]
    opt = torch.as_tensor(1 + np.arange(n) % n_opt, dtype=torch.int32, device=ctx.device)
    res = TrialResult(n, opt, ctx.device)
    trials = lambda: ctx.option_trials(*s0, opt, W, clf, mask, 0, res)
    trials()
    torch.cuda.synchronize()
    longest = int(res.steps.max())
    st = EnvState(n, ctx.device, m)
    Wv = W.view(n_opt + 1, -1)

    def loop():                                           # the composition: prepare the envs, then `longest` acting steps
        for t, a in zip(st.state(), s0):
            t.copy_(a)
        st.option_id.copy_(opt); st.opt_steps.zero_(); st.ep_steps.zero_()
        for k in range(1, n_opt + 1):
            q = ctx.q_values(s0, Wv[k].contiguous())
            sel = opt == k
            st.qcache.view(5, n)[:, sel] = q[:, sel]
        ctx.invalidate_order()
        for t in range(longest):
            ctx.step(st, W, clf, mask, t, learn=False)

    loop()
    rec = Trajectory(n, rows, 0, ctx.device) if rows else None
    res_rec = TrialResult(n, opt, ctx.device)
    trials_rec = lambda: ctx.option_trials(*s0, opt, W, clf, mask, 0, res_rec, record=rec)
    if rec is not None:
        trials_rec()
    tr, lp, rr = [], [], []
    for _ in range(rounds):
        tr.append(_time(trials) * 1e3)
        lp.append(_time(loop) * 1e3)
        if rec is not None:
            rr.append(_time(trials_rec) * 1e3)
    a, b = float(np.median(tr)), float(np.median(lp))
    hist = np.bincount(res.outcome.cpu().numpy(), minlength=5)[1:].tolist()
    out = {"n": n, "options": n_opt, "max_option_steps": max_opt, "longest_trial_steps": longest,
            "mean_steps": round(float(res.steps.double().mean()), 2), "outcomes_succ_end_left_timeout": hist,
            "trials_ms": round(a, 3), "step_loop_ms": round(b, 3), "speedup": round(b / a, 2),
            "trials_rounds_ms": [round(x, 3) for x in tr], "step_loop_rounds_ms": [round(x, 3) for x in lp]}
    if rec is not None:
        c = float(np.median(rr))
        out.update({"record_rows": rows, "trials_record_ms": round(c, 3), "record_cost_pct": round(100.0 * (c / a - 1.0), 1),
                    "trials_record_rounds_ms": [round(x, 3) for x in rr]})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-option-steps", type=int, default=250)
    ap.add_argument("--record", type=int, default=0, help="also time the trials recorded with this many rows per entry")
    a = ap.parse_args()
    print(json.dumps(bench(a.n, a.rounds, a.max_option_steps, rows=a.record)), flush=True)


if __name__ == "__main__":
    main()
