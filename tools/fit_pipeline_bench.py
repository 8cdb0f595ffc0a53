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
"""
import argparse
import statistics

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=2048); ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=9); ap.add_argument("--epsilon", type=float, default=0.1)
    ap.add_argument("--lam", type=float, default=0.9); ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--options", type=int, default=None, help="options of the workload (default: the headline's)")
    ap.add_argument("--toy", action="store_true", help="lift the floor of 9 rounds (the suite's end-to-end run: its figures measure nothing)")
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
