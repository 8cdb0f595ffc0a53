"""Is the automatic block geometry (auto_block_envs) the fastest of the three builds at every env count? One MI355X;
per env count: bench.py (root + 5 options, pinball_simple) with --block-envs 64 / 128 / 256, and which one the context picks by itself.
A bench run that fails ends the sweep there.    python tools/geometry_sweep.py [--steps 300] [N ...]"""
import argparse
import rig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300); ap.add_argument("--options", type=int, default=5)
    ap.add_argument("envs", type=int, nargs="*", default=[2048, 4096, 8192, 16384, 20480, 24576, 32768, 40960, 49152, 65536, 98304, 131072])
    a = ap.parse_args()
    from skill_chaining_with_graphs_amd import auto_block_envs
    print(f"# python tools/geometry_sweep.py: M env-steps/s (us per step-batch), root + {a.options} options, pinball_simple, {a.steps} steps; * = what the context picks", flush=True)
    worst = 1.0
    for n in a.envs:
        row = {b: rig.bench_row(rig.bench_line(rig.ROOT, "--envs-per-gpu", n, "--options", a.options, "--block-envs", b, "--steps", a.steps, "--warmup", 50,
                                               "--ramp", 100, "--no-cpu-baseline", "--no-extras")) for b in (64, 128, 256)}
        pick = auto_block_envs(n)
        best = max(row, key=lambda b: row[b][0])
        ratio = row[pick][0] / max(row[best][0], 1e-9)
        worst = min(worst, ratio)
        print(f"envs {n:7d}: " + "  ".join(f"B={b:3d}{'*' if b == pick else ' '} {row[b][0]:7.1f} ({row[b][1]:6.1f})" for b in (64, 128, 256))
              + f"   pick / best = {ratio:.3f}", flush=True)
    print(f"# worst pick / best over the sweep: {worst:.3f}")


if __name__ == "__main__":
    main()
