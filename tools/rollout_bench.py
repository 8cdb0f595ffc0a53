"""µs per acting step-batch: scg_rollout (K steps in one launch, SPEC §8) against K calls of scg_step(flags = 0).

Root + 5 options (chain classifiers, all enabled), bench-like weights (std 1e-3), 4096 and 65 536 envs, K = 64. Each side is
warmed up and synchronised, and the two are timed alternately (rounds of rollout, step loop, rollout, ...); the line per size
gives the median over the rounds. --record adds rollouts that record every step (SPEC §10) of all envs (`all`) or of the
first N envs (`N`), timed in the same alternation (`none` is the plain rollout, always timed). --interrupt adds interrupting
rollouts (SPEC §11, scg_rollout_interrupt) on a state of their own, timed in the same alternation. --choose times something
else: value-ranked choice (SPEC §14, scg_rollout_select) against scg_rollout_record's kernel, on the default chain and on the
sibling tree of tools/choice_report.py (bench_choose). --audit times the audited rollout (SPEC §15, scg_rollout_audit, keeping the
discounted return) against scg_rollout_select with the same rules, record and launches (bench_audit). --population C times a
population rollout (SPEC §21, scg_rollout_population) of C policies x 4096 envs against C sequential audited rollouts of 4096 envs
and against one audited rollout of C x 4096 envs under a single weight table (bench_population). --population-clf C times the same
population launch with a classifier table per policy (SPEC §24.1, scg_rollout_population_clf) against the launch without one
(bench_population_clf), --population-gate C the same launch with a gate table per policy as well (SPEC §25.1,
scg_rollout_population_gate; bench_population_gate), and --logits scg_classifier_logits against scg_classifier_predict at 65 536 points (bench_logits); both
print each arm's min - max over the rounds beside the ratio.

    python tools/rollout_bench.py [--sizes 4096 65536] [--k 64] [--rounds 7] [--epw 2 4 8 16 32] [--record none 1024 all]
                                  [--interrupt] [--choose] [--audit] [--population 1 4 8 16] [--population-clf 1 4 8 16] [--logits]
                                  [--population-gate 1 4 8 16]
"""
import argparse
import json
import os

import rig


def bench(n, k, rounds, n_opt=5, epw=None, record=(), interrupt=False):
    import numpy as np
    import torch
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd.core import ScgContext
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    m = scg.load_map("pinball_simple")
    ctx = ScgContext(n, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000)
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    clf = torch.as_tensor(rig.chain_classifiers(m, n_opt), device=ctx.device).view(-1)
    g = torch.Generator().manual_seed(3)
    W = (torch.randn((n_opt + 1) * 5 * 1296, generator=g) * 1e-3).to(ctx.device)
    st_r, st_s = rig.state_on(ctx, m, n), rig.state_on(ctx, m, n)
    t = {"r": 0, "s": 0}

    def roll():
        if epw:                                           # pinned launch geometry (envs per wave) instead of scg_rollout's pick
            os.environ["SCG_ROLLOUT_EPW"] = str(epw)
        try:
            ctx.rollout(st_r, W, clf, mask, t["r"], k)
        finally:
            os.environ.pop("SCG_ROLLOUT_EPW", None)
        t["r"] += k

    def loop():
        for _ in range(k):
            ctx.step(st_s, W, clf, mask, t["s"], learn=False)
            t["s"] += 1

    recs = []                                             # (label, its own state and step counter, the record)
    for spec in record:
        nr = n if spec == "all" else min(int(spec), n)
        recs.append((spec, {"st": rig.state_on(ctx, m, n), "t": 0}, Trajectory(nr, k, 0, ctx.device)))

    def roll_rec(r):
        ctx.rollout(r[1]["st"], W, clf, mask, r[1]["t"], k, record=r[2])
        r[1]["t"] += k

    ist = {"st": rig.state_on(ctx, m, n), "t": 0, "intr": torch.zeros((n_opt + 1) * n, dtype=torch.int32, device=ctx.device)}

    def roll_int():
        ctx.rollout(ist["st"], W, clf, mask, ist["t"], k, interrupt=True, interrupts=ist["intr"])
        ist["t"] += k

    roll(); loop(); roll(); loop()                        # warm-up (first launches, allocator, code objects)
    for r in recs:
        roll_rec(r); roll_rec(r)
    if interrupt:
        roll_int(); roll_int()
    r_us, s_us, rec_us, int_us = [], [], {r[0]: [] for r in recs}, []
    for _ in range(rounds):
        r_us.append(rig.timed(roll, 3) * 1e6 / k)
        s_us.append(rig.timed(loop, 3) * 1e6 / k)
        for r in recs:
            rec_us[r[0]].append(rig.timed(lambda: roll_rec(r), 3) * 1e6 / k)
        if interrupt:
            int_us.append(rig.timed(roll_int, 3) * 1e6 / k)
    r, s = float(np.median(r_us)), float(np.median(s_us))
    out = {"n_envs": n, "k": k, "epw": epw or "auto", "options": n_opt, "rollout_us_per_step": round(r, 2), "step_loop_us_per_step": round(s, 2),
           "speedup": round(s / r, 2), "rollout_rounds_us": [round(v, 2) for v in r_us],
           "step_loop_rounds_us": [round(v, 2) for v in s_us]}
    for label, v in rec_us.items():
        med = float(np.median(v))
        out[f"record_{label}_us_per_step"] = round(med, 2)
        out[f"record_{label}_cost_pct"] = round(100.0 * (med / r - 1.0), 1)
        out[f"record_{label}_rounds_us"] = [round(x, 2) for x in v]
    if interrupt:
        med = float(np.median(int_us))
        out["interrupt_us_per_step"] = round(med, 2)
        out["interrupt_cost_pct"] = round(100.0 * (med / r - 1.0), 1)
        out["interrupt_rounds_us"] = [round(x, 2) for x in int_us]
        out["interrupts_per_env_step"] = round(float(ist["intr"].sum()) / (ist["t"] * n), 4)
    return out


SIBLING_PARENTS = [0, 0, 0, 1, 1, 2]


def bench_choose(n, k, rounds, layout, n_opt=5):
    """µs per step of scg_rollout_select(BEST) against scg_rollout_record's kernel (a record of one env: the same recording
    instantiation, next to nothing recorded), each on a state of its own, timed alternately. layout "chain": the default chain
    (at most one candidate: the kernel's overhead alone); "sibling": tools/choice_report.py's hand-set tree (several candidates:
    the extra evaluations too)."""
    import numpy as np
    import torch
    import skill_chaining_with_graphs_amd as scg
    from choice_report import disc_weights, sibling_discs
    from skill_chaining_with_graphs_amd.core import ScgContext
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    m = scg.load_map("pinball_simple")
    ctx = ScgContext(n, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000)
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    if layout == "sibling":
        ctx.set_option_parents(SIBLING_PARENTS)
        c = np.zeros((n_opt + 1, 8), np.float32)
        c[1:] = [disc_weights(*d) for d in sibling_discs(m)]
    else:
        c = rig.chain_classifiers(m, n_opt)
    clf = torch.as_tensor(c, device=ctx.device).view(-1)
    g = torch.Generator().manual_seed(3)
    W = (torch.randn((n_opt + 1) * 5 * 1296, generator=g) * 1e-3).to(ctx.device)
    side = {}
    for name in ("record", "choose"):
        side[name] = {"st": rig.state_on(ctx, m, n), "t": 0, "stats": EpisodeStats(n_opt + 1, n, ctx.device), "us": []}
    rec = Trajectory(1, k, 0, ctx.device)

    def roll(name):
        s = side[name]
        kw = {"record": rec} if name == "record" else {"choose": "value"}
        ctx.rollout(s["st"], W, clf, mask, s["t"], k, s["stats"], **kw)
        s["t"] += k

    for name in side:
        roll(name); roll(name)
    for _ in range(rounds):
        for name in side:
            side[name]["us"].append(rig.timed(lambda: roll(name), 3) * 1e6 / k)
    r, c_us = (float(np.median(side[x]["us"])) for x in ("record", "choose"))
    out = {"n_envs": n, "k": k, "options": n_opt, "layout": layout, "record_kernel_us_per_step": round(r, 2),
           "choose_us_per_step": round(c_us, 2), "choose_over_record": round(c_us / r, 4),
           "record_rounds_us": [round(v, 2) for v in side["record"]["us"]], "choose_rounds_us": [round(v, 2) for v in side["choose"]["us"]]}
    for name in side:
        s = side[name]
        out[f"{name}_offers_per_env_step"] = round(float(s["stats"].entries.sum() + s["stats"].declines.sum()) / (s["t"] * n), 4)
    st = side["choose"]
    out["choose_overrides_per_env_step"] = round(float(st["stats"].overrides.sum()) / (st["t"] * n), 4)
    return out


def bench_audit(n, k, rounds, rules, n_opt=5):
    """µs per step of scg_rollout_audit (disc_ret, disc_g and disc_final kept; no begin, so no force) against scg_rollout_select
    with the same `rules` ("" / "interrupt" / "best" / "best+interrupt"), both with a record of one env, each on a state of its own, on
    tools/choice_report.py's sibling tree, timed alternately."""
    import numpy as np
    import torch
    import skill_chaining_with_graphs_amd as scg
    from choice_report import disc_weights, sibling_discs
    from skill_chaining_with_graphs_amd.core import ScgContext
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats, GateAudit
    from skill_chaining_with_graphs_amd.trajectory import Trajectory
    m = scg.load_map("pinball_simple")
    ctx = ScgContext(n, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000)
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    ctx.set_option_parents(SIBLING_PARENTS)
    c = np.zeros((n_opt + 1, 8), np.float32)
    c[1:] = [disc_weights(*d) for d in sibling_discs(m)]
    clf = torch.as_tensor(c, device=ctx.device).view(-1)
    g = torch.Generator().manual_seed(3)
    W = (torch.randn((n_opt + 1) * 5 * 1296, generator=g) * 1e-3).to(ctx.device)
    kw = {"interrupt": "interrupt" in rules, "choose": "value" if "best" in rules else None}
    if kw["choose"] is None:                                   # rules without BEST: scg_rollout_select's kernels, reached by their own names
        del kw["choose"]
    side = {}
    for name in ("select", "audit"):
        side[name] = {"st": rig.state_on(ctx, m, n), "t": 0, "stats": EpisodeStats(n_opt + 1, n, ctx.device), "us": []}
    rec, ga = Trajectory(1, k, 0, ctx.device), GateAudit(n, ctx.device)

    def roll(name):
        s = side[name]
        ctx.rollout(s["st"], W, clf, mask, s["t"], k, s["stats"], record=rec, **kw, **({"audit": ga} if name == "audit" else {}))
        s["t"] += k

    for name in side:
        roll(name); roll(name)
    for _ in range(rounds):
        for name in side:
            side[name]["us"].append(rig.timed(lambda: roll(name), 3) * 1e6 / k)
    sel, aud = (float(np.median(side[x]["us"])) for x in ("select", "audit"))
    return {"n_envs": n, "k": k, "options": n_opt, "rules": rules or "none", "select_us_per_step": round(sel, 2),
            "audit_us_per_step": round(aud, 2), "audit_over_select": round(aud / sel, 4),
            "select_rounds_us": [round(v, 2) for v in side["select"]["us"]], "audit_rounds_us": [round(v, 2) for v in side["audit"]["us"]]}


def bench_population(n_pol, k, rounds, n_per=4096, n_opt=5):
    """µs per step of ONE population rollout of n_pol policies x n_per envs (distinct weight tables, the bench's epsilon and mask
    for all) against (a) n_pol audited rollouts of n_per envs one after the other, one per table, and (b) one audited rollout of
    n_pol * n_per envs under a single table: what per-policy tables cost. bench()'s workload, each side on states of its own,
    the discounted return kept on all three, timed alternately."""
    import numpy as np
    import torch
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd.core import ScgContext
    from skill_chaining_with_graphs_amd.evaluation import GateAudit
    m = scg.load_map("pinball_simple")
    n = n_pol * n_per
    small, big = (ScgContext(v, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000) for v in (n_per, n))
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    clf = torch.as_tensor(rig.chain_classifiers(m, n_opt), device=big.device).view(-1)
    g = torch.Generator().manual_seed(3)
    W = (torch.randn((n_pol, n_opt + 1, 5, 1296), generator=g) * 1e-3).to(big.device)
    eps = torch.full((n_pol,), 0.05, dtype=torch.float32, device=big.device)
    enabled = torch.full((n_pol,), mask, dtype=torch.int32, device=big.device)
    side = {"pop": {"st": rig.state_on(big, m, n), "au": GateAudit(n, big.device)},
            "one": {"st": rig.state_on(big, m, n), "au": GateAudit(n, big.device)},
            "seq": {"st": [rig.state_on(small, m, n_per, seed=1 + c) for c in range(n_pol)], "au": [GateAudit(n_per, small.device) for _ in range(n_pol)]}}
    for s in side.values():
        s["t"], s["us"] = 0, []

    def roll(name):
        s = side[name]
        if name == "pop":
            big.rollout(s["st"], W, clf, mask, s["t"], k, audit=s["au"], population=(eps, enabled))
        elif name == "one":
            big.rollout(s["st"], W[0].view(-1), clf, mask, s["t"], k, audit=s["au"])
        else:
            for c in range(n_pol):
                small.rollout(s["st"][c], W[c].view(-1), clf, mask, s["t"], k, audit=s["au"][c])
        s["t"] += k

    for name in side:
        roll(name); roll(name)
    for _ in range(rounds):
        for name in side:
            side[name]["us"].append(rig.timed(lambda: roll(name), 3) * 1e6 / k)
    pop, one, seq = (float(np.median(side[x]["us"])) for x in ("pop", "one", "seq"))
    return {"policies": n_pol, "n_per": n_per, "k": k, "options": n_opt, "population_us_per_step": round(pop, 2),
            "sequential_us_per_step": round(seq, 2), "single_table_us_per_step": round(one, 2),
            "population_over_sequential": round(pop / seq, 4), "population_over_single_table": round(pop / one, 4),
            "population_rounds_us": [round(v, 2) for v in side["pop"]["us"]], "sequential_rounds_us": [round(v, 2) for v in side["seq"]["us"]],
            "single_table_rounds_us": [round(v, 2) for v in side["one"]["us"]]}


def _arm(us):
    """median and [min, max] of an arm's rounds."""
    import numpy as np
    return round(float(np.median(us)), 2), [round(float(min(us)), 2), round(float(max(us)), 2)]


def bench_population_clf(n_pol, k, rounds, n_per=4096, n_opt=5):
    """µs per step of the population rollout of bench_population with a classifier table per policy (the chain's discs, their radii
    scaled by 1 - 0.02 c for policy c) against the same launch without one (every policy reads `clf`, the chain's discs), each on a
    state of its own, timed alternately. What the per-workgroup staging of pop_clf[c] costs."""
    import torch
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd.core import ScgContext
    from skill_chaining_with_graphs_amd.evaluation import GateAudit
    m = scg.load_map("pinball_simple")
    n = n_pol * n_per
    ctx = ScgContext(n, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000)
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    clf = torch.as_tensor(rig.chain_classifiers(m, n_opt), device=ctx.device)
    tabs = clf.reshape(1, n_opt + 1, 8).repeat(n_pol, 1, 1)
    shrink = (1.0 - 0.02 * torch.arange(n_pol, dtype=torch.float32, device=ctx.device)) ** 2
    # a disc's row is [r^2 - |c|^2, 2 cu, 2 cv, -1, 0, -1] in (u, v) = 2 (x, y) - 1: scaling r changes its constant alone
    r2 = tabs[:, 1:, 0] + (tabs[:, 1:, 1] ** 2 + tabs[:, 1:, 2] ** 2) / 4
    tabs[:, 1:, 0] += r2 * (shrink[:, None] - 1.0)
    tabs = tabs.contiguous()
    g = torch.Generator().manual_seed(3)
    W = (torch.randn((n_pol, n_opt + 1, 5, 1296), generator=g) * 1e-3).to(ctx.device)
    eps = torch.full((n_pol,), 0.05, dtype=torch.float32, device=ctx.device)
    enabled = torch.full((n_pol,), mask, dtype=torch.int32, device=ctx.device)
    side = {name: {"st": rig.state_on(ctx, m, n), "au": GateAudit(n, ctx.device), "t": 0, "us": []} for name in ("pop", "clf")}

    def roll(name):
        s = side[name]
        ctx.rollout(s["st"], W, clf.view(-1), mask, s["t"], k, audit=s["au"], population=(eps, enabled) + ((tabs,) if name == "clf" else ()))
        s["t"] += k

    for name in side:
        roll(name); roll(name)
    for _ in range(rounds):
        for name in side:
            side[name]["us"].append(rig.timed(lambda: roll(name), 3) * 1e6 / k)
    (pop, pop_mm), (pc, pc_mm) = _arm(side["pop"]["us"]), _arm(side["clf"]["us"])
    return {"policies": n_pol, "n_per": n_per, "k": k, "options": n_opt, "population_us_per_step": pop, "population_min_max_us": pop_mm,
            "population_clf_us_per_step": pc, "population_clf_min_max_us": pc_mm, "clf_over_population": round(pc / pop, 4),
            "population_rounds_us": [round(v, 2) for v in side["pop"]["us"]], "population_clf_rounds_us": [round(v, 2) for v in side["clf"]["us"]]}


def bench_population_gate(n_pol, k, rounds, n_per=4096, n_opt=5):
    """µs per step of bench_population_clf's population rollout with a gate table per policy too (SPEC §25.1,
    scg_rollout_population_gate; the table is gatefit.shipped_gate(W[c]), so the three arms act alike) against the same launch with
    the classifier tables alone (--population-clf's arm) and with neither, each on a state of its own, timed alternately. What the
    fifth POP kernel's gate units cost. `offers_per_env_step`: one more, untimed launch of the gated arm with the episode counters."""
    import torch
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd import gatefit
    from skill_chaining_with_graphs_amd.core import ScgContext
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats, GateAudit
    m = scg.load_map("pinball_simple")
    n = n_pol * n_per
    ctx = ScgContext(n, n_opt, m, device=0, seed=7, epsilon=0.05, max_episode_steps=2000)
    mask = ((1 << (n_opt + 1)) - 1) & ~1
    clf = torch.as_tensor(rig.chain_classifiers(m, n_opt), device=ctx.device)
    tabs = clf.reshape(1, n_opt + 1, 8).repeat(n_pol, 1, 1).contiguous()
    g = torch.Generator().manual_seed(3)
    W = (torch.randn((n_pol, n_opt + 1, 5, 1296), generator=g) * 1e-3).to(ctx.device)
    gates = torch.stack([gatefit.shipped_gate(W[c]) for c in range(n_pol)]).contiguous()
    eps = torch.full((n_pol,), 0.05, dtype=torch.float32, device=ctx.device)
    enabled = torch.full((n_pol,), mask, dtype=torch.int32, device=ctx.device)
    tail = {"pop": (), "clf": (tabs,), "gate": (tabs, gates)}
    side = {name: {"st": rig.state_on(ctx, m, n), "au": GateAudit(n, ctx.device), "t": 0, "us": []} for name in tail}

    def roll(name, **kw):
        s = side[name]
        ctx.rollout(s["st"], W, clf.view(-1), mask, s["t"], k, audit=s["au"], population=(eps, enabled) + tail[name], **kw)
        s["t"] += k

    for name in side:
        roll(name); roll(name)
    for _ in range(rounds):
        for name in side:
            side[name]["us"].append(rig.timed(lambda: roll(name), 3) * 1e6 / k)
    stats = EpisodeStats(n_opt + 1, n, ctx.device)
    roll("gate", stats=stats)
    torch.cuda.synchronize()
    offers = float(stats.entries.sum() + stats.declines.sum()) / (n * k)
    (pop, pop_mm), (pc, pc_mm), (pg, pg_mm) = (_arm(side[x]["us"]) for x in ("pop", "clf", "gate"))
    return {"policies": n_pol, "n_per": n_per, "k": k, "options": n_opt, "population_us_per_step": pop, "population_min_max_us": pop_mm,
            "population_clf_us_per_step": pc, "population_clf_min_max_us": pc_mm, "population_gate_us_per_step": pg,
            "population_gate_min_max_us": pg_mm, "gate_over_clf": round(pg / pc, 4), "gate_over_population": round(pg / pop, 4),
            "offers_per_env_step": round(offers, 5),
            "population_clf_rounds_us": [round(v, 2) for v in side["clf"]["us"]], "population_gate_rounds_us": [round(v, 2) for v in side["gate"]["us"]]}


def bench_logits(rounds, n=65536):
    """µs per call of scg_classifier_logits against scg_classifier_predict on n points and one row, timed alternately (100 calls a round)."""
    import torch
    import skill_chaining_with_graphs_amd as scg
    from skill_chaining_with_graphs_amd.core import ScgContext
    m = scg.load_map("pinball_simple")
    ctx = ScgContext(n, 1, m, device=0, seed=7)
    g = torch.Generator().manual_seed(3)
    x, y = (torch.rand(n, generator=g).to(ctx.device) for _ in range(2))
    w8 = torch.as_tensor(rig.chain_classifiers(m, 1)[1], device=ctx.device).contiguous()
    arms = {"predict": lambda: ctx.classifier_predict(x, y, w8), "logits": lambda: ctx.classifier_logits(x, y, w8)}
    us = {name: [] for name in arms}
    for fn in arms.values():
        rig.timed(fn, 20)
    for _ in range(rounds):
        for name, fn in arms.items():
            us[name].append(rig.timed(fn, 100) * 1e6)
    (p, p_mm), (l, l_mm) = _arm(us["predict"]), _arm(us["logits"])
    return {"points": n, "predict_us_per_call": p, "predict_min_max_us": p_mm, "logits_us_per_call": l, "logits_min_max_us": l_mm,
            "logits_over_predict": round(l / p, 4), "predict_rounds_us": [round(v, 2) for v in us["predict"]],
            "logits_rounds_us": [round(v, 2) for v in us["logits"]]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--epw", type=int, nargs="*", default=None,
                    help="also time the rollout at these pinned launch geometries (envs per wave: 2, 4, 8, 16, 32)")
    ap.add_argument("--record", nargs="+", default=["none"],
                    help="also time recorded rollouts: `all` envs or the first N envs (`none`: the plain rollout only)")
    ap.add_argument("--interrupt", action="store_true", help="also time interrupting rollouts (SPEC §11)")
    ap.add_argument("--choose", action="store_true",
                    help="instead: value-ranked choice (SPEC §14) against the recording kernel, on the chain and on the sibling tree")
    ap.add_argument("--audit", action="store_true",
                    help="instead: the audited rollout (SPEC §15) against scg_rollout_select, for the four rules, on the sibling tree")
    ap.add_argument("--population", type=int, nargs="+", default=None,
                    help="instead: a population rollout (SPEC §21) of C policies x 4096 envs against C sequential audited rollouts and one of C x 4096 envs")
    ap.add_argument("--population-clf", type=int, nargs="+", default=None,
                    help="instead: the population rollout with a classifier table per policy (SPEC §24.1) against the same launch without one")
    ap.add_argument("--population-gate", type=int, nargs="+", default=None,
                    help="instead: the population rollout with a gate table per policy (SPEC §25.1) against --population-clf's launch and the plain one")
    ap.add_argument("--logits", action="store_true", help="instead (or after --population-clf): scg_classifier_logits against scg_classifier_predict at 65 536 points")
    a = ap.parse_args()
    if a.population_gate:
        for c in a.population_gate:
            print(json.dumps(bench_population_gate(c, a.k, a.rounds)), flush=True)
        return
    if a.population_clf or a.logits:
        for c in a.population_clf or []:
            print(json.dumps(bench_population_clf(c, a.k, a.rounds)), flush=True)
        if a.logits:
            print(json.dumps(bench_logits(a.rounds)), flush=True)
        return
    if a.population:
        for c in a.population:
            print(json.dumps(bench_population(c, a.k, a.rounds)), flush=True)
        return
    if a.audit:
        for n in a.sizes:
            for rules in ("", "interrupt", "best", "best+interrupt"):
                print(json.dumps(bench_audit(n, a.k, a.rounds, rules)), flush=True)
        return
    if a.choose:
        for n in a.sizes:
            for layout in ("chain", "sibling"):
                print(json.dumps(bench_choose(n, a.k, a.rounds, layout)), flush=True)
        return
    rec = [r for r in a.record if r != "none"]
    for r in rec:
        if r != "all" and not r.isdigit():
            ap.error(f"--record takes none, all or an env count, not {r}")
    for n in a.sizes:
        print(json.dumps(bench(n, a.k, a.rounds, record=rec, interrupt=a.interrupt)), flush=True)
        for epw in a.epw or []:
            print(json.dumps(bench(n, a.k, a.rounds, epw=epw)), flush=True)


if __name__ == "__main__":
    main()
