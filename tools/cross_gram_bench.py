"""What scg_feature_cross_gram costs (SPEC §17.1): the cross Gram of recorded (state, successor) pairs at --sizes samples
in three layouts of segments — one segment, 25 equal ones, and 25 with the uneven sizes an actual fit's (a, a') pairs had
(--fit-sizes: the root's CONT samples of tests/test_gpu_lstdq.py's record, scaled to the sample count) — against two yardsticks on
the same states in the same process: the materialising path (ScgContext.features of s and of s2 in chunks of --chunk samples,
then phi.T @ phi2 per chunk and segment) and scg_feature_gram on s with the same offsets (equal samples per segment; it does
half the products). All are timed interleaved, round by round, as tools/ab_bench.py does; one JSON line per case with the median
times, the TFLOP/s counted on the full square (2 n 1296^2 flops) and its share of the 157.3 TF f32 matrix peak.
The states are snapshots of the headline workload's env states, one per step-batch; s2 is the next snapshot's.
--lib NAME=PATH times further builds of the library (another tiling or chunk: make's DEFS) in the same rounds.

    python tools/cross_gram_bench.py [--sizes 65536 1048576] [--rounds 3] [--lib c16=path/to/libscg_hip_c16.so] [--out file.jsonl]
"""
import argparse
import json
import statistics

import rig

PEAK_TF = 157.3
NF = 1296
FIT_SIZES = [297, 382, 248, 97, 230, 206, 1120, 520, 179, 175, 351, 468, 335, 116, 150, 268, 462, 134, 183, 236, 138, 483, 133, 84, 941]


def recorded_pairs(n, envs):
    """n pairs (s, s2) on the device: the env states of the headline workload after each of ceil(n / envs) step-batches and after
    the step-batch that follows."""
    import torch
    ag = rig.headline_agent(envs=envs)
    snaps = []
    for _ in range(-(-n // envs) + 1):
        ag.step_batch()
        snaps.append([t.clone() for t in ag.state.state()])
    s = [torch.cat([p[d] for p in snaps[:-1]])[:n].contiguous() for d in range(4)]
    s2 = [torch.cat([p[d] for p in snaps[1:]])[:n].contiguous() for d in range(4)]
    torch.cuda.synchronize()
    return ag, s, s2


def layouts(n, fit_sizes):
    """{name: offsets} of the three layouts over n samples."""
    total = sum(fit_sizes)
    cuts, acc = [0], 0
    for v in fit_sizes:
        acc += v
        cuts.append(n * acc // total)
    return {"1 segment": [0, n], "25 equal": [n * i // 25 for i in range(26)], "25 as fitted": cuts}


def materialised(ctx, s, s2, offsets, chunk):
    import torch
    out = torch.zeros((len(offsets) - 1, NF, NF), dtype=torch.float32, device=s[0].device)
    for g in range(len(offsets) - 1):
        for lo in range(offsets[g], offsets[g + 1], chunk):
            hi = min(lo + chunk, offsets[g + 1])
            out[g].addmm_(ctx.features([t[lo:hi] for t in s]).T, ctx.features([t[lo:hi] for t in s2]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 1048576]); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=65536); ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--fit-sizes", type=int, nargs=25, default=FIT_SIZES); ap.add_argument("--lib", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd.core import ScgContext
    ag, s, s2 = recorded_pairs(max(a.sizes), a.envs)
    ctxs = {"shipped": ag.ctx}
    for spec in a.lib:
        name, path = spec.split("=", 1)
        ctxs[name] = ScgContext(64, 0, ag.map, device=0, library=path)
    lines = []
    for n in a.sizes:
        sub, sub2 = [t[:n] for t in s], [t[:n] for t in s2]
        for layout, off in layouts(n, a.fit_sizes).items():
            runs = {name: (lambda c=c: c.feature_cross_gram(sub, sub2, off)) for name, c in ctxs.items()}
            runs["feature_gram"] = lambda: ag.ctx.feature_gram(sub, off)
            runs["materialised"] = lambda: materialised(ag.ctx, sub, sub2, off, a.chunk)
            ref = runs["shipped"]()
            err = float((runs["materialised"]() - ref).abs().max() / ref.abs().max())
            times = {name: [] for name in runs}
            for _ in range(a.rounds):
                for name, fn in runs.items():
                    times[name].append(rig.timed(fn, 1) * 1e3)
            flops = 2 * n * NF * NF
            sizes = [off[i + 1] - off[i] for i in range(len(off) - 1)]
            row = {"samples": n, "layout": layout, "largest_segment": max(sizes), "smallest_segment": min(sizes), "rounds": a.rounds,
                   "materialised_max_rel_diff": err}
            for name, t in times.items():
                ms = statistics.median(t)
                row[name] = {"ms": round(ms, 3), "min_ms": round(min(t), 3), "tflops_square": round(flops / ms / 1e9, 2),
                             "peak_fraction": round(flops / ms / 1e9 / PEAK_TF, 4)}
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
