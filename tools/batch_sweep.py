"""env-steps/s of the shipped build against the number of envs on ONE MI355X (5 options, pinball_simple): python bench.py --envs-per-gpu N
(the three builds against each other: tools/geometry_sweep.py). A bench run that fails ends the sweep there.   python tools/batch_sweep.py"""
import rig

COMMON = ("--steps", 400, "--warmup", 50, "--no-cpu-baseline", "--no-extras")


def main():
    print("# python bench.py --envs-per-gpu N --steps 400 --warmup 50 --no-cpu-baseline --no-extras, one MI355X, shipped build (5 options, pinball_simple)", flush=True)
    for n in (4096, 16384, 32768, 49152, 65536, 98304, 131072, 262144):
        v, us, td = rig.bench_row(rig.bench_line(rig.ROOT, "--envs-per-gpu", n, *COMMON))
        print(f"envs {n:7d}  blocks {n // 256:5d}  {v:7.1f} M env-steps/s  step {us:7.2f} us  td {td:7.2f} us", flush=True)
    v, us, td = rig.bench_row(rig.bench_line(rig.ROOT, "--no-learn", *COMMON))
    print(f"# acting-only (--no-learn, 65536 envs): {v:.1f} M env-steps/s, {us:.1f} us/step", flush=True)
    v, us, td = rig.bench_row(rig.bench_line(rig.ROOT, "--options", 1, "--envs-per-gpu", 4096, *COMMON))
    print(f"# BASELINE configs[1] (4096 envs, root + 1 option): {v:.1f} M env-steps/s, {us:.2f} us/step (td {td:.2f})")


if __name__ == "__main__":
    main()
