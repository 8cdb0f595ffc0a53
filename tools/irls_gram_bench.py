"""What scg_basis_gram_irls costs (SPEC §23.2): at the orders 3 / 5 / 7 and --sizes samples (one segment), interleaved
round by round as tools/gram_bench.py times its arms, "irls" = scg_basis_gram_irls under the logistic terms of seeded logits against
"gram" = scg_basis_gram with yv = e at the same order — the same MFMAs without the weight — and, at order 5, against "weighted" =
scg_feature_gram_weighted (n_tgt = 0: the same weighted A without the right-hand side). With --lib NAME=PATH (the parent commit's
library) "gram@NAME" is that build's scg_basis_gram in the same rounds: what the existing instantiations cost before and after. One
JSON line per order and size: per arm the median, the fastest and the slowest round in ms, the ratios of the medians, and same_bits
= grad is scg_basis_gram's b and, under unit weights, H its A. A last line is one initfit.irls_fit's wall time (order 3, "state",
vx > 0 labels on the first size's states), its iterations and its reason.

    python tools/irls_gram_bench.py [--sizes 8192 65536] [--orders 3 5 7] [--rounds 9] [--lib parent=path/to/libscg_hip.so] [--out file.jsonl]
"""
import argparse
import json
import statistics
import time

import gram_bench
import rig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 65536]); ap.add_argument("--orders", type=int, nargs="+", default=[3, 5, 7])
    ap.add_argument("--rounds", type=int, default=9); ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--lib", nargs="*", default=[]); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from skill_chaining_with_graphs_amd import initfit
    ag, s = gram_bench.recorded_states(max(a.sizes), a.envs)
    ctx, lines = ag.ctx, []
    others = gram_bench.other_builds(a, ag)
    for order in a.orders:
        for n in a.sizes:
            sub = [t[:n].contiguous() for t in s]
            gen = torch.Generator(sub[0].device).manual_seed(n)
            z = torch.randn(n, dtype=torch.float32, device=sub[0].device, generator=gen) * 4
            label = (torch.rand(n, device=sub[0].device, generator=gen) < 0.5).to(torch.uint8)
            _, rw, e = ctx.logistic_terms(z, label)
            runs = {"irls": lambda: ctx.basis_gram_irls(order, sub, [0, n], rw, e),
                    "gram": lambda: ctx.basis_gram(order, sub, [0, n], e)}
            if order == 5:
                runs["weighted"] = lambda: ctx.feature_gram_weighted(sub, [0, n], rw)
            runs.update({f"gram@{name}": (lambda c=c: c.basis_gram(order, sub, [0, n], e)) for name, c in others.items()})
            (H, g), (A, b) = runs["irls"](), runs["gram"]()
            H1, _ = ctx.basis_gram_irls(order, sub, [0, n], torch.ones_like(rw), e)
            same = bool(torch.equal(g.view(torch.int32), b.view(torch.int32)) and torch.equal(H1.view(torch.int32), A.view(torch.int32)))
            for name in others:
                Ao, bo = runs[f"gram@{name}"]()
                same = same and bool(torch.equal(A.view(torch.int32), Ao.view(torch.int32)) and torch.equal(b.view(torch.int32), bo.view(torch.int32)))
            del H, g, A, b, H1
            times = gram_bench.interleaved(runs, a.rounds)
            med = {name: statistics.median(t) for name, t in times.items()}
            row = {"order": order, "samples": n, "rounds": a.rounds, "same_bits": same}
            row.update({name: gram_bench.spread(t) for name, t in times.items()})
            row["irls_over_gram"] = round(med["irls"] / med["gram"], 4)
            if order == 5:
                row["irls_over_weighted"] = round(med["irls"] / med["weighted"], 4)
            for name in others:
                row[f"gram_over_gram@{name}"] = round(med["gram"] / med[f"gram@{name}"], 4)
            lines.append(json.dumps(row))
            print(lines[-1], flush=True)
    n = a.sizes[0]
    sub = [t[:n].contiguous() for t in s]
    label = (sub[2] > 0).to(torch.uint8)
    if 0 < int(label.sum()) < n:
        initfit.irls_fit(ctx, 3, sub, label)                               # (warm: the first launches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w, hist, reason = initfit.irls_fit(ctx, 3, sub, label)
        torch.cuda.synchronize()
        lines.append(json.dumps({"fit": "order 3, state, vx > 0", "samples": n, "wall_ms": round((time.perf_counter() - t0) * 1e3, 2),
                                 "iterations": len(hist) - 1, "reason": reason, "tol": initfit.DEFAULT_TOL}))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
