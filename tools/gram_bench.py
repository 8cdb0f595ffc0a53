"""What scg_feature_gram costs (SPEC §16.1): the Gram of recorded states at --sizes samples per segment and --segs
segments, against the materialising path (ScgContext.features in chunks of --chunk samples, then phi.T @ phi per chunk and
segment). The two are timed interleaved, round by round, as tools/ab_bench.py does; one JSON line per case with the median
times, the TFLOP/s counted on the triangle (n 1296 1297 flops) and its share of the 157.3 TF f32 matrix peak.
The states are snapshots of the headline workload's env states, one per step-batch.
--lib NAME=PATH times further builds of the library (another tiling: make's DEFS) in the same rounds.
--order P (3, 5 or 7; SPEC §18) times scg_basis_gram at that order against ScgContext.basis_features + phi.T @ phi,
flops counted on the triangle of F = (P + 1)^4 features; without it the tool is scg_feature_gram's, as it was.
--targets C (1 .. 16; SPEC §20.1) times, at each of --sizes samples, three ways to the C right-hand sides of one set of
states, interleaved round by round: "targets" = scg_feature_gram_targets, one segment, C targets; "one_rhs" = scg_feature_gram, one
segment with yv (it issues the same number of MFMAs: the floor); "repeated" = scg_feature_gram on C segments of the same states
repeated, target c as segment c's yv (what a fit of C actions would otherwise call). One JSON line per size: per arm the median,
the fastest and the slowest round in ms (the tool's own round-to-round spread), and the ratios of the medians. --segs is not used.
With --lib NAME=PATH a fourth arm "targets@NAME" is that build's scg_feature_gram_targets on the same operands in the same rounds.
--weighted C (0 .. 16; SPEC §22.1) times, at each of --sizes samples and interleaved round by round, "weighted" =
scg_feature_gram_weighted with C targets under seeded root weights in [0.25, 4] against "targets" = the unweighted call on the same
operands (scg_feature_gram_targets; C = 0: scg_feature_gram without yv): per arm the median, the fastest and the slowest round, the
ratio of the medians, and same_bits = does the weighted call under unit weights give the unweighted call's A and B by bits.

    python tools/gram_bench.py [--sizes 65536 1048576] [--segs 1 5] [--rounds 5] [--lib r3=path/to/libscg_hip_r3.so] [--order 7] [--out file.jsonl]
    python tools/gram_bench.py --targets 5 [--sizes 8192 65536 1048576] [--rounds 9] [--lib parent=path/to/libscg_hip.so] [--out file.jsonl]
    python tools/gram_bench.py --weighted 5 [--sizes 8192 65536 1048576] [--rounds 9] [--out file.jsonl]
"""
import argparse
import json
import statistics

import rig

PEAK_TF = 157.3
NF = 1296


def recorded_states(n, envs):
    """n states (x, y, vx, vy) on the device: the env states of the headline workload after each of ceil(n / envs) step-batches."""
    import torch
    ag = rig.headline_agent(envs=envs)
    parts = []
    for _ in range(-(-n // envs)):
        ag.step_batch()
        parts.append([t.clone() for t in ag.state.state()])
    s = [torch.cat([p[d] for p in parts])[:n].contiguous() for d in range(4)]
    torch.cuda.synchronize()
    return ag, s


def materialised(ctx, s, offsets, chunk, order=None):
    import torch
    F = NF if order is None else (order + 1) ** 4
    out = torch.zeros((len(offsets) - 1, F, F), dtype=torch.float32, device=s[0].device)
    for g in range(len(offsets) - 1):
        for lo in range(offsets[g], offsets[g + 1], chunk):
            hi = min(lo + chunk, offsets[g + 1])
            phi = ctx.features([t[lo:hi] for t in s]) if order is None else ctx.basis_features(order, [t[lo:hi] for t in s])
            out[g].addmm_(phi.T, phi)
    return out


def other_builds(a, ag):
    """{NAME: a context on the library at PATH} for every --lib NAME=PATH."""
    from skill_chaining_with_graphs_amd.core import ScgContext
    return {name: ScgContext(64, 0, ag.map, device=0, library=path) for name, path in (spec.split("=", 1) for spec in a.lib)}


def interleaved(runs, rounds):
    """Every arm once per round, round by round: {arm: [ms per round]}."""
    times = {name: [] for name in runs}
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(rig.timed(fn, 1) * 1e3)
    return times


def spread(t):
    return {"ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}


def weighted_bench(a):
    """--weighted C: the two arms at each size; returns the JSON lines."""
    import torch
    C = a.weighted
    ag, s = recorded_states(max(a.sizes), a.envs)
    ctx, lines = ag.ctx, []
    for n in a.sizes:
        sub = [t[:n].contiguous() for t in s]
        gen = torch.Generator(sub[0].device).manual_seed(n)
        Y = torch.randn((C, n), dtype=torch.float32, device=sub[0].device, generator=gen) if C else None
        rw = torch.rand(n, dtype=torch.float32, device=sub[0].device, generator=gen) * 3.75 + 0.25
        plain = (lambda: ctx.feature_gram_targets(sub, [0, n], Y)) if C else (lambda: (ctx.feature_gram(sub, [0, n]), None))
        runs = {"weighted": lambda: ctx.feature_gram_weighted(sub, [0, n], rw, Y), "targets": plain}
        (A1, B1), (A0, B0) = ctx.feature_gram_weighted(sub, [0, n], torch.ones_like(rw), Y), plain()
        same = bool(torch.equal(A1.view(torch.int32), A0.view(torch.int32)) and (C == 0 or torch.equal(B1.view(torch.int32), B0.view(torch.int32))))
        times = interleaved(runs, a.rounds)
        row = {"samples": n, "n_targets": C, "rounds": a.rounds, "same_bits": same}
        row.update({name: spread(t) for name, t in times.items()})
        row["weighted_over_targets"] = round(statistics.median(times["weighted"]) / statistics.median(times["targets"]), 4)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    return lines


def targets_bench(a):
    """--targets C: the three arms at each size (and one per --lib build); returns the JSON lines."""
    import torch
    C = a.targets
    ag, s = recorded_states(max(a.sizes), a.envs)
    ctx, lines = ag.ctx, []
    others = other_builds(a, ag)
    for n in a.sizes:
        sub = [t[:n].contiguous() for t in s]
        Y = torch.randn((C, n), dtype=torch.float32, device=sub[0].device, generator=torch.Generator(sub[0].device).manual_seed(n))
        tiled, yv = [t.repeat(C) for t in sub], Y.reshape(-1)
        runs = {"targets": lambda: ctx.feature_gram_targets(sub, [0, n], Y),
                "one_rhs": lambda: ctx.feature_gram(sub, [0, n], Y[0]),
                "repeated": lambda: ctx.feature_gram(tiled, [i * n for i in range(C + 1)], yv)}
        runs.update({f"targets@{name}": (lambda c=c: c.feature_gram_targets(sub, [0, n], Y)) for name, c in others.items()})
        (A, B), (A1, _), (_, bC) = runs["targets"](), runs["one_rhs"](), runs["repeated"]()
        same = bool(torch.equal(A, A1) and torch.equal(B[0], bC))      # (the bits the three ways must share)
        for name in others:
            Ao, Bo = runs[f"targets@{name}"]()
            same = same and bool(torch.equal(A, Ao) and torch.equal(B, Bo))
        times = interleaved(runs, a.rounds)
        med = {name: statistics.median(t) for name, t in times.items()}
        row = {"samples": n, "n_targets": C, "rounds": a.rounds, "same_bits": same}
        row.update({name: spread(t) for name, t in times.items()})
        row["targets_over_one_rhs"] = round(med["targets"] / med["one_rhs"], 4)
        row["repeated_over_one_rhs"] = round(med["repeated"] / med["one_rhs"], 4)
        row["repeated_over_targets"] = round(med["repeated"] / med["targets"], 4)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 1048576]); ap.add_argument("--segs", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--envs", type=int, default=65536); ap.add_argument("--lib", nargs="*", default=[])
    ap.add_argument("--order", type=int, default=None, choices=(3, 5, 7)); ap.add_argument("--out", default=None)
    ap.add_argument("--targets", type=int, default=None, choices=range(1, 17), metavar="C")
    ap.add_argument("--weighted", type=int, default=None, choices=range(0, 17), metavar="C")
    a = ap.parse_args()
    if a.targets is not None or a.weighted is not None:
        lines = targets_bench(a) if a.weighted is None else weighted_bench(a)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        return
    F = NF if a.order is None else (a.order + 1) ** 4
    import torch
    ag, s = recorded_states(max(a.sizes) * max(a.segs), a.envs)
    ctxs = dict({"shipped": ag.ctx}, **other_builds(a, ag))
    lines = []
    for n in a.sizes:
        for k in a.segs:
            off = [i * n for i in range(k + 1)]
            sub = [t[: n * k] for t in s]
            if a.order is None:
                runs = {name: (lambda c=c: c.feature_gram(sub, off)) for name, c in ctxs.items()}
            else:
                runs = {name: (lambda c=c: c.basis_gram(a.order, sub, off)) for name, c in ctxs.items()}
            runs["materialised"] = lambda: materialised(ag.ctx, sub, off, a.chunk, a.order)
            ref = runs["shipped"]()
            err = float((runs["materialised"]() - ref).abs().max() / ref.abs().max())
            times = interleaved(runs, a.rounds)
            flops = n * k * F * (F + 1)
            row = {"samples_per_segment": n, "segments": k, "rounds": a.rounds, "materialised_max_rel_diff": err}
            if a.order is not None:
                row["order"] = a.order
            for name, t in times.items():
                ms = statistics.median(t)
                row[name] = {"ms": round(ms, 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "tflops_triangle": round(flops / ms / 1e9, 2),
                             "peak_fraction": round(flops / ms / 1e9 / PEAK_TF, 4)}
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
