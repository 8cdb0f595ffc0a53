"""What SPEC §27's two kernels cost against the paths they replace, on one recorded set of episodes of the headline workload (its
chain classifiers, all options on, random weights: the rows' value functions are mixed as a chain mixes them). Arms interleaved round
by round as tools/gram_bench.py times its arms, every arm ending in a device synchronise.

  row values, on the record's first --rows rows, the row's table its vf (6 tables):
    row_values          ScgContext.row_values, v and a copied to the host (where the replaced path leaves them)
    row_values_device   the same without the copy
    q_values_host_max   what agent.py does today: per table its rows in chunks of the context's n_envs through
                        ScgContext.q_values, each chunk copied to the host, valuefit.greedy_max there (the rows are gathered per
                        table on the device before the clock starts)
  the scan, on the whole record at lambda = 1:
    lambda_returns         the flat record uploaded, ScgContext.lambda_returns, y0 and yk copied back
    lambda_returns_device  the kernel alone on uploaded arrays
    returns_to_go          valuefit.returns_to_go on the same flat record (host)

  --trace: SPEC §28's scan instead of the above, on the same record, every arm the kernel alone on uploaded arrays at lambda = 0.9
  (v0, vk: the record's row values under W; ag: the greedy action of the acting table, so that the cut falls where it would):
    lambda_returns_device      ScgContext.lambda_returns, the baseline
    trace_returns_uncut        ScgContext.trace_returns(cut=False), no horizon: the same targets
    trace_returns_cut          cut=True, no horizon
    trace_returns_cut_h        cut=True with the horizon h
  each round times --reps calls of an arm behind one synchronise (a single call is well under a millisecond).

  --cross: SPEC §29's cross row values instead, on the record's first --rows rows, the row's table its vf, W_sel = W and W_val an
  independent table of the same scale, every arm on uploaded arrays, --reps calls behind one synchronise:
    row_values               one ScgContext.row_values call under W_sel: the yardstick
    two_row_values_gather    what the cross target needs today at the least: row_values under W_sel for the action, a second call
                             under W_val, and the gather of a [5][n] value array at that action on the device
    row_values_cross         ScgContext.row_values_cross (v, a and vs)
    row_values_cross_given   ScgContext.row_action_values at the recorded actions

One JSON line per comparison: per arm the median, fastest and slowest round in ms, the ratio of the medians, and same_bits (the two
paths' values agree bit for bit; for the scan: y0 is returns_to_go's g where every episode ended done).

    python tools/lambda_targets_bench.py [--rows 1048576] [--episodes 2048] [--envs 65536] [--rounds 15] [--out file.jsonl]
"""
import argparse
import json
import statistics

import gram_bench
import rig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20); ap.add_argument("--episodes", type=int, default=2048)
    ap.add_argument("--envs", type=int, default=65536); ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--epsilon", type=float, default=0.1); ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="time scg_trace_returns against scg_lambda_returns instead (SPEC §28.4)")
    ap.add_argument("--cross", action="store_true", help="time scg_row_values_cross against scg_row_values instead (SPEC §29.4)")
    ap.add_argument("--reps", type=int, default=20, help="--trace, --cross: calls per timed window")
    a = ap.parse_args()
    import numpy as np
    import torch
    from skill_chaining_with_graphs_amd.valuefit import greedy_max, returns_to_go
    ag = rig.headline_agent(envs=a.envs, w_std=0.05)
    ctx, dev = ag.ctx, ag.W.device
    traj, _ = ag.record_episodes(n_episodes=a.episodes, epsilon=a.epsilon, seed=1)
    flat = traj.to_numpy()
    total, lines = len(flat["reward"]), []
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    if a.trace or a.cross:
        lines.append(json.dumps(trace_row(a, ag, flat, up) if a.trace else cross_row(a, ag, flat, up)))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return

    # ---- row values
    n = min(a.rows, total)
    states = [up(flat[f][:n]) for f in ("x", "y", "vx", "vy")]
    tab = up(flat["vf"][:n].astype(np.uint8))
    W = ag.W.contiguous().view(ag.n_vf, -1, 1296)
    per_table = []
    for k in range(ag.n_vf):
        at = torch.nonzero(tab == k)[:, 0]
        per_table.append((at.cpu().numpy(), [t[at].contiguous() for t in states]))

    def old_path():
        v, act = np.zeros(n, np.float32), np.zeros(n, np.uint8)
        for k, (at, sk) in enumerate(per_table):
            for i in range(0, len(at), ctx.n_envs):
                q = ctx.q_values([t[i:i + ctx.n_envs].contiguous() for t in sk], W[k].contiguous().view(-1)).cpu().numpy()
                v[at[i:i + ctx.n_envs]], act[at[i:i + ctx.n_envs]] = greedy_max(q)
        return v, act

    def new_path():
        v, act = ctx.row_values(states, tab, W)
        return v.cpu().numpy(), act.cpu().numpy()

    runs = {"row_values": new_path, "row_values_device": lambda: ctx.row_values(states, tab, W), "q_values_host_max": old_path}
    (v1, a1), (v0, a0) = new_path(), old_path()
    same = bool(np.array_equal(v1.view(np.uint32), v0.view(np.uint32)) and np.array_equal(a1, a0))
    times = gram_bench.interleaved(runs, a.rounds)
    med = {name: statistics.median(t) for name, t in times.items()}
    row = {"what": "row values", "rows": n, "tables": ag.n_vf, "rows_per_table": [int(len(at)) for at, _ in per_table],
           "chunk": ctx.n_envs, "rounds": a.rounds, "same_bits": same}
    row.update({name: gram_bench.spread(t) for name, t in times.items()})
    row["row_values_over_q_values_host_max"] = round(med["row_values"] / med["q_values_host_max"], 4)
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)

    # ---- the scan
    gamma, R = float(ctx.cfg.gamma), float(ctx.cfg.r_option_success)
    zeros = torch.zeros(total, dtype=torch.float32, device=dev)

    def upload():
        return [up(flat["offsets"]), up(flat["reward"])] + [up(flat[f].astype(np.uint8)) for f in ("done", "vf", "term")]

    def scan():
        y0, yk = ctx.lambda_returns(*upload(), zeros, zeros, gamma, 1.0, R)
        return y0.cpu().numpy(), yk.cpu().numpy()

    on_device = upload()
    runs = {"lambda_returns": scan, "lambda_returns_device": lambda: ctx.lambda_returns(*on_device, zeros, zeros, gamma, 1.0, R),
            "returns_to_go": lambda: returns_to_go(flat, gamma, R)}
    (y0, yk), tg = scan(), returns_to_go(flat, gamma, R)
    all_done = bool(np.all(flat["done"][flat["offsets"][1:] - 1] != 0))
    same = bool(np.array_equal(y0.view(np.uint64), tg["g"].view(np.uint64)))
    opt = flat["vf"] >= 1
    times = gram_bench.interleaved(runs, a.rounds)
    med = {name: statistics.median(t) for name, t in times.items()}
    L = np.diff(flat["offsets"])
    row = {"what": "lambda returns at lambda = 1", "rows": total, "envs": int(len(L)), "longest_env": int(L.max()), "rounds": a.rounds,
           "every_episode_done": all_done, "same_bits": same,
           "max_abs_yk_minus_y": float(np.max(np.abs(yk - tg["y"])[opt])) if opt.any() else 0.0}
    row.update({name: gram_bench.spread(t) for name, t in times.items()})
    row["lambda_returns_over_returns_to_go"] = round(med["lambda_returns"] / med["returns_to_go"], 4)
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def trace_row(a, ag, flat, up):
    """--trace: the JSON row of scg_trace_returns against scg_lambda_returns on the record `flat`."""
    import numpy as np
    import torch
    from skill_chaining_with_graphs_amd.valuefit import trace_targets
    ctx = ag.ctx
    gamma, R, lam = float(ctx.cfg.gamma), float(ctx.cfg.r_option_success), 0.9
    lt = trace_targets(ctx, flat, ag.W, gamma, lam, R, cut=True)
    rec = [up(flat["offsets"]), up(flat["reward"])] + [up(flat[f].astype(np.uint8)) for f in ("done", "vf", "term")]
    act, agr, v0, vk = up(flat["action"].astype(np.uint8)), up(lt["ag"]), up(lt["v0"]), up(lt["vk"])
    runs = {"lambda_returns_device": lambda: ctx.lambda_returns(*rec, v0, vk, gamma, lam, R),
            "trace_returns_uncut": lambda: ctx.trace_returns(*rec, act, agr, v0, vk, gamma, lam, R, cut=False),
            "trace_returns_cut": lambda: ctx.trace_returns(*rec, act, agr, v0, vk, gamma, lam, R, cut=True),
            "trace_returns_cut_h": lambda: ctx.trace_returns(*rec, act, agr, v0, vk, gamma, lam, R, cut=True, horizon=True)}
    base, uncut = runs["lambda_returns_device"](), runs["trace_returns_uncut"]()
    same = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(base, uncut))
    for fn in runs.values():                                   # every arm once more before the clock
        fn()
    times = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, fn in runs.items():
            times[name].append(rig.timed(fn, a.reps) * 1e3)
    med = {name: statistics.median(t) for name, t in times.items()}
    L = np.diff(flat["offsets"])
    smp = lt["sample"]
    row = {"what": "trace returns at lambda = 0.9", "rows": len(flat["reward"]), "envs": int(len(L)), "longest_env": int(L.max()),
           "rounds": a.rounds, "reps": a.reps, "cut_share": round(float(np.mean(lt["cut"][smp])), 4),
           "mean_horizon": round(float(np.mean(lt["h"][smp])), 3), "uncut_same_bits_as_lambda_returns": bool(same)}
    row.update({name: gram_bench.spread(t) for name, t in times.items()})
    for name in list(runs)[1:]:
        row[f"{name}_over_lambda_returns_device"] = round(med[name] / med["lambda_returns_device"], 4)
    return row


def cross_row(a, ag, flat, up):
    """--cross: the JSON row of scg_row_values_cross against scg_row_values on the first a.rows rows of the record `flat`."""
    import numpy as np
    import torch
    ctx = ag.ctx
    n = min(a.rows, len(flat["reward"]))
    states = [up(flat[f][:n]) for f in ("x", "y", "vx", "vy")]
    tab, act = up(flat["vf"][:n].astype(np.uint8)), up(np.minimum(flat["action"][:n], 4).astype(np.uint8))
    W_sel = ag.W.contiguous().view(ag.n_vf, -1, 1296)
    gen = torch.Generator(device="cpu").manual_seed(7)
    W_val = (torch.randn(W_sel.shape, generator=gen) * float(W_sel.std())).to(W_sel.device)
    q5 = torch.zeros((5, n), dtype=torch.float32, device=W_sel.device)         # the [5][n] array the gather reads
    cols = torch.arange(n, device=W_sel.device)

    def two_calls():
        _, sel = ctx.row_values(states, tab, W_sel)
        ctx.row_values(states, tab, W_val, actions=False)
        return q5[sel.clamp(max=4).long(), cols]

    runs = {"row_values": lambda: ctx.row_values(states, tab, W_sel),
            "two_row_values_gather": two_calls,
            "row_values_cross": lambda: ctx.row_values_cross(states, tab, W_sel, W_val, sel_values=True),
            "row_values_cross_given": lambda: ctx.row_action_values(states, tab, W_val, act)}
    (v1, a1), (v, sel, vs) = runs["row_values"](), runs["row_values_cross"]()
    same = bool(torch.equal(vs.view(torch.int32), v1.view(torch.int32)) and torch.equal(sel, a1))
    for fn in runs.values():                                   # every arm once more before the clock
        fn()
    times = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, fn in runs.items():
            times[name].append(rig.timed(fn, a.reps) * 1e3)
    med = {name: statistics.median(t) for name, t in times.items()}
    row = {"what": "cross row values", "rows": n, "tables": ag.n_vf, "rounds": a.rounds, "reps": a.reps,
           "rows_per_table": [int((tab == k).sum()) for k in range(ag.n_vf)],
           "argmax_differs_share": round(float((ctx.row_values(states, tab, W_val)[1] != sel).float().mean()), 4),
           "vs_and_a_same_bits_as_row_values": same}
    row.update({name: gram_bench.spread(t) for name, t in times.items()})
    for name in list(runs)[1:]:
        row[f"{name}_over_row_values"] = round(med[name] / med["row_values"], 4)
    row["row_values_cross_over_two_row_values_gather"] = round(med["row_values_cross"] / med["two_row_values_gather"], 4)
    return row


if __name__ == "__main__":
    main()
