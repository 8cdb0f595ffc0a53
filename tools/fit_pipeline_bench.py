"""What SPEC §30's device record and device fit pipeline cost against the host paths they stand beside, in one run on one recorded
set of episodes of the headline workload (tools/lambda_targets_bench.py's: chain classifiers, all options on, random weights). Arms
interleaved round by round as tools/gram_bench.py times its arms, every arm ending in a device synchronise; the host arms are the
default paths. Both fit arms run fit_values_to_returns' one loop: they differ in where the flat view comes from (an upload of the
Trajectory per call / DeviceRecord.flat()) and in how Q of a sample list is formed (q_values in chunks / one row_action_values).

  the record, --episodes episodes at --epsilon:
    record_host      agent.record_episodes(): every launch's buffers downloaded and cut per env on the host
    record_device    agent.record_episodes(device=True), then DeviceRecord.flat(): appended and packed on the device
  the fit, a Watkins fit at --lam with --sweeps sweeps on that record:
    fit_host         fit_values_to_returns(trajectory=the Trajectory)
    fit_device       fit_values_to_returns(trajectory=the DeviceRecord, pipeline="device")

Per comparison the medians with the fastest and slowest round, the ratio of the medians, whether the two results agree by bits, and
`separated`: the device arm's median lies below the host arm's by more than the rounds' own min-max spread (the wider of the two).
Text lines; the first names the settings.

    python tools/fit_pipeline_bench.py [--episodes 2048] [--envs 65536] [--rounds 9] [--out profiles/r36_fit_pipeline_bench.txt]

--solver (SPEC §31.4) times instead who solves the refit's normal equations, on the same record and the same fit (host pipeline):
    host      fit_values_to_returns(): the Gram downloaded, valuefit.ridge_solve on the host
    torch     the same loop with valuefit.ridge_solve(device=): a vendor Cholesky per action on the device, Delta downloaded
    device    fit_values_to_returns(solver="device"): scg_ridge_solve, A and b left where the Gram call wrote them
arms interleaved; then one instrumented fit per arm (a device synchronise after every part, so its total is not a timing) split
per sweep into the targets, the Gram call to its sync, the solve, the refit's rest (the read-back of A or of Delta, the new rows),
the Q^old / Q^new calls and the rest (sample lists, statistics); then the kernel call alone on 30 matrices of 1296^2 and 5 of
4096^2 against torch.linalg.cholesky_ex + cholesky_solve on the same systems.

    python tools/fit_pipeline_bench.py --solver [--rounds 9] [--out profiles/r37_ridge_solve_bench.txt]
"""
import argparse
import statistics
import time

import gram_bench
import rig


def compare(what, times, host, device, same):
    sp = {name: gram_bench.spread(t) for name, t in times.items()}
    width = max(sp[name]["max_ms"] - sp[name]["min_ms"] for name in (host, device))
    gap = sp[host]["ms"] - sp[device]["ms"]
    out = [f"{what}: same_bits {same}"]
    for name in (host, device):
        out.append(f"  {name:<14} median {sp[name]['ms']:11.3f} ms  min {sp[name]['min_ms']:11.3f}  max {sp[name]['max_ms']:11.3f}  rounds {len(times[name])}")
    out.append(f"  {device} / {host} = {sp[device]['ms'] / sp[host]['ms']:.4f}; the medians differ by {gap:.3f} ms, the wider min-max spread is "
               f"{width:.3f} ms: separated {gap > width}")
    return out


def fmt(name, t):
    sp = gram_bench.spread(t)
    return f"  {name:<14} median {sp['ms']:11.3f} ms  min {sp['min_ms']:11.3f}  max {sp['max_ms']:11.3f}  rounds {len(t)}"


def solver_bench(a, ag, say):
    """--solver: the three arms, the per-sweep breakdown and the kernel call alone."""
    import numpy as np
    import torch
    from skill_chaining_with_graphs_amd import valuefit
    from skill_chaining_with_graphs_amd._lib import NUM_ACTIONS
    traj = ag.record_episodes(n_episodes=a.episodes, epsilon=a.epsilon, seed=1)[0]
    ectx = ag._eval_ctx[int(a.episodes)][0]
    say(f"# fit_pipeline_bench --solver envs {a.envs} options {ag.n_options} episodes {a.episodes} epsilon {a.epsilon} rows "
        f"{len(traj.to_numpy()['reward'])} lam {a.lam} sweeps {a.sweeps} trace watkins pipeline host rounds {a.rounds}"
        f"{' (toy)' if a.toy else ''} device {torch.cuda.get_device_name(0)}")
    fit_kw = dict(trajectory=traj, epsilon=a.epsilon, seed=1, lam=a.lam, sweeps=a.sweeps, trace="watkins")
    refit = ag._refit_rows

    def refit_torch(gram, states, d, act_fit, ridge, scale, W_k, solver="host", ectx=None):
        """_refit_rows with the vendor Cholesky on the device: A and b are not downloaded, Delta is."""
        n_a = np.bincount(act_fit, minlength=NUM_ACTIONS).astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(n_a)]).astype(np.int64)
        A, b = gram(states, offsets, torch.from_numpy(d).to(ag.W.device))
        delta = valuefit.ridge_solve(A, b, n_a, ridge, scale, device=ag.W.device)
        w_old = W_k.cpu().numpy()
        w_new = (w_old.astype(np.float64) + delta).astype(np.float32)
        w_new[n_a == 0] = w_old[n_a == 0]
        return n_a, offsets, A, b, delta, w_new

    def arm(name):
        def run():
            ag._refit_rows = refit_torch if name == "torch" else refit
            try:
                return ag.fit_values_to_returns(solver="device" if name == "device" else "host", **fit_kw)
            finally:
                ag._refit_rows = refit
        return run

    arms = {name: arm(name) for name in ("host", "torch", "device")}
    res = {name: fn() for name, fn in arms.items()}
    i32 = lambda t: t.contiguous().view(torch.int32)
    same = lambda x, y: bool(torch.equal(i32(x[1]), i32(y[1]))) and all(
        torch.equal(i32(p["W"]), i32(q["W"])) for p, q in zip(x[0]["sweeps"], y[0]["sweeps"]))
    say(f"equal by bits: host arm twice {same(res['host'], arms['host']())}, device arm twice {same(res['device'], arms['device']())}, "
        f"device arm under pipeline='device' {same(res['device'], ag.fit_values_to_returns(solver='device', pipeline='device', **fit_kw))}")
    for name in ("torch", "device"):
        gap = [float((p["W"].double() - q["W"].double()).abs().max()) for p, q in zip(res[name][0]["sweeps"], res["host"][0]["sweeps"])]
        say(f"max |W - W_host| per sweep, {name}: {' '.join(f'{g:.3g}' for g in gap)}  (another summation order: not equal by bits)")
    times = gram_bench.interleaved(arms, a.rounds)
    say(f"fit_values_to_returns(lam={a.lam}, sweeps={a.sweeps}, trace='watkins'), the whole call:")
    for name in arms:
        say(fmt(name, times[name]))
    sp = {name: gram_bench.spread(t) for name, t in times.items()}
    for name in ("torch", "device"):
        width = max(sp[n]["max_ms"] - sp[n]["min_ms"] for n in ("host", name))
        gap = sp["host"]["ms"] - sp[name]["ms"]
        say(f"  {name} / host = {sp[name]['ms'] / sp['host']['ms']:.4f}; the medians differ by {gap:.3f} ms ({gap / a.sweeps:.1f} ms a sweep), the "
            f"wider min-max spread is {width:.3f} ms: separated {gap > width}")

    # ---- the breakdown: one instrumented fit per arm
    parts = {}

    def clocked(part, fn):
        def run(*args, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*args, **kw)
            torch.cuda.synchronize()
            parts[part] = parts.get(part, 0.0) + (time.perf_counter() - t0) * 1e3
            return out
        return run

    say("per sweep, one instrumented fit per arm (ms; a synchronise after every part):")
    say(f"  {'arm':<8}{'targets':>10}{'gram':>10}{'solve':>10}{'refit rest':>12}{'q calls':>10}{'rest':>10}{'total':>10}")
    orig = {"sweep_targets": valuefit.sweep_targets, "ridge_solve": valuefit.ridge_solve, "pinned": valuefit.ridge_solve_pinned,
            "gram": ectx.feature_gram, "q": ag._q_chunks}
    for name in arms:
        parts.clear()
        valuefit.sweep_targets = clocked("targets", orig["sweep_targets"])
        valuefit.ridge_solve = clocked("solve", orig["ridge_solve"])
        valuefit.ridge_solve_pinned = clocked("solve", orig["pinned"])
        ectx.feature_gram = clocked("gram", orig["gram"])
        ag._q_chunks = clocked("q", orig["q"])
        inner = refit_torch if name == "torch" else refit
        ag._refit_rows = clocked("refit", inner)
        try:
            clocked("total", lambda: ag.fit_values_to_returns(solver="device" if name == "device" else "host", **fit_kw))()
        finally:
            valuefit.sweep_targets, valuefit.ridge_solve, valuefit.ridge_solve_pinned = orig["sweep_targets"], orig["ridge_solve"], orig["pinned"]
            del ectx.feature_gram, ag._q_chunks, ag._refit_rows
        p = {k: v / a.sweeps for k, v in parts.items()}
        rest_refit = p["refit"] - p["gram"] - p["solve"]
        rest = p["total"] - p["targets"] - p["refit"] - p["q"]
        say(f"  {name:<8}{p['targets']:10.1f}{p['gram']:10.1f}{p['solve']:10.1f}{rest_refit:12.1f}{p['q']:10.1f}{rest:10.1f}{p['total']:10.1f}")

    # ---- the kernel call alone
    for n_mat, F in ((30, 1296), (5, 4096)):
        gen = torch.Generator(ag.W.device).manual_seed(F)
        X = torch.randn((n_mat, 2 * F, F), dtype=torch.float32, device=ag.W.device, generator=gen)
        A = torch.bmm(X.transpose(1, 2), X).contiguous()
        del X
        B = torch.randn((n_mat, F), dtype=torch.float32, device=ag.W.device, generator=gen)
        lam = torch.ones(F, dtype=torch.float64, device=ag.W.device)
        M = torch.tril(A.double())
        M = M + torch.tril(M, -1).transpose(1, 2)
        M.diagonal(dim1=1, dim2=2).add_(1.0)
        B64 = B.double()[:, :, None]

        def vendor():                                          # (a matrix at a time, as valuefit.ridge_solve(device=) calls them)
            return torch.stack([torch.cholesky_solve(B64[g], torch.linalg.cholesky_ex(M[g])[0])[:, 0] for g in range(n_mat)])

        mine = lambda: ectx.ridge_solve(A, B, lam, [1.0] * n_mat)
        x_v, (x_m, _, info) = vendor(), mine()
        rel = float((x_m - x_v).abs().max() / x_v.abs().max())
        t = gram_bench.interleaved({"scg_ridge_solve": mine, "torch": vendor}, a.rounds)
        say(f"the call alone, {n_mat} matrices of {F}^2, one right-hand side each (info all 0: {not bool(info.any())}; max |x - x_torch| / max |x_torch| "
            f"{rel:.3g}; torch: cholesky_ex + cholesky_solve on the float64 matrices, one at a time):")
        for name in t:
            say(fmt(name, t[name]))
        say(f"  scg_ridge_solve / torch = {statistics.median(t['scg_ridge_solve']) / statistics.median(t['torch']):.3f}")
        del A, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=2048); ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=9); ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--lam", type=float, default=0.9); ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--options", type=int, default=None, help="options of the workload (default: the headline's)")
    ap.add_argument("--toy", action="store_true", help="lift the floor of 9 rounds (the suite's end-to-end run: its figures measure nothing)")
    ap.add_argument("--solver", action="store_true", help="SPEC §31.4: the refit's solver arms instead of the record and pipeline arms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 9 and not a.toy:
        raise SystemExit("--rounds must be at least 9")
    import numpy as np
    import torch
    ag = rig.headline_agent(envs=a.envs, w_std=0.05, **({} if a.options is None else {"options": a.options}))
    rec_kw = dict(n_episodes=a.episodes, epsilon=a.epsilon, seed=1)
    lines = []

    def say(ln):
        lines.append(ln)
        print(ln, flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    if a.solver:
        return solver_bench(a, ag, say)

    def record_device():
        rec, _ = ag.record_episodes(device=True, **rec_kw)
        rec.flat()
        return rec

    traj, rec = ag.record_episodes(**rec_kw)[0], record_device()
    want, got = traj.to_numpy(), rec.to_numpy()
    same = all(np.array_equal(got[f].view(np.uint8), want[f].view(np.uint8)) for f in want if f != "first")
    say(f"# fit_pipeline_bench envs {a.envs} options {ag.n_options} episodes {a.episodes} epsilon {a.epsilon} rows {len(want['reward'])} "
        f"max_episode_steps {int(ag.ctx.cfg.max_episode_steps)} lam {a.lam} sweeps {a.sweeps} trace watkins rounds {a.rounds}{' (toy)' if a.toy else ''} "
        f"device {torch.cuda.get_device_name(0)}")
    times = gram_bench.interleaved({"record_host": lambda: ag.record_episodes(**rec_kw), "record_device": record_device}, a.rounds)
    for ln in compare("record_episodes", times, "record_host", "record_device", same):
        say(ln)

    fit_kw = dict(epsilon=a.epsilon, seed=1, lam=a.lam, sweeps=a.sweeps, trace="watkins")
    fit_host = lambda: ag.fit_values_to_returns(trajectory=traj, **fit_kw)
    fit_device = lambda: ag.fit_values_to_returns(trajectory=rec, pipeline="device", **fit_kw)
    (rep_h, W_h), (rep_d, W_d) = fit_host(), fit_device()
    same = bool(torch.equal(W_h.view(torch.int32), W_d.view(torch.int32))) and all(
        torch.equal(x["W"].view(torch.int32), y["W"].view(torch.int32)) for x, y in zip(rep_h["sweeps"], rep_d["sweeps"]))
    times = gram_bench.interleaved({"fit_host": fit_host, "fit_device": fit_device}, a.rounds)
    for ln in compare(f"fit_values_to_returns(lam={a.lam}, sweeps={a.sweeps}, trace='watkins')", times, "fit_host", "fit_device", same):
        say(ln)
    med = {name: statistics.median(t) for name, t in times.items()}
    say(f"per sweep: host {med['fit_host'] / a.sweeps:.1f} ms, device {med['fit_device'] / a.sweeps:.1f} ms")


if __name__ == "__main__":
    main()
