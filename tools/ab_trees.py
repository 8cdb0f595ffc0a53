"""A/B timing across source TREES and library builds on one box (round 5: the ABI moved, so a round-4 library no longer loads into
this tree's binding): python tools/ab_trees.py [--rounds R] [--steps K] name=tree_root[:lib.so] ...
Runs `python <tree_root>/bench.py` once per arm per round, interleaved (clock drift hits every arm alike), with SCG_LIB pointing at
the arm's library when one is given; prints M env-steps/s, us per step and the fused kernel's event time per run, then the medians.
A run that fails ends the tool there (rig.bench_line raises): nothing more is started on the GPU."""
import argparse, os, statistics
import rig


def main(argv=None, width=24, us_in_median=True):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--extra", default="", help="extra bench.py flags for every arm")
    ap.add_argument("arms", nargs="+")
    a = ap.parse_args(argv)
    arms = []
    for spec in a.arms:
        name, rest = spec.split("=", 1)
        root, _, lib = rest.partition(":")
        arms.append((name, os.path.abspath(root), os.path.abspath(lib) if lib else None))
    res = {n: [] for n, _, _ in arms}
    for r in range(a.rounds):
        for name, root, lib in arms:
            row = rig.bench_row(rig.bench_line(root, "--steps", a.steps, "--warmup", 50, "--no-cpu-baseline", "--no-extras", *a.extra.split(), lib=lib))
            res[name].append(row)
            print(f"{name:{width}s} {row[0]:7.1f} M/s  {row[1]:7.2f} us/step  td {row[2]:6.2f} us", flush=True)
    for name, _, _ in arms:
        med = [statistics.median(x[i] for x in res[name]) for i in range(3)]
        print(f"median {name:{width}s} {med[0]:7.1f} M/s  " + (f"{med[1]:7.2f} us/step  " if us_in_median else "") + f"td {med[2]:6.2f} us")


if __name__ == "__main__":
    main()
