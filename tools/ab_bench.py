"""A/B timing of library builds on one box: python tools/ab_bench.py [--rounds R] [--steps K] lib1.so lib2.so ...
Runs bench.py once per library per round (interleaved, so clock drift hits every arm alike) with SCG_LIB pointing at
the build, and prints M env-steps/s, us per step and the td_kernel's event time per run, then the per-arm medians.
It is tools/ab_trees.py with every arm in this tree: the fields it reads (value, ms_per_step, roofline.kernel_ms) are rig.bench_row's."""
import argparse, os
import ab_trees, rig


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args(argv)
    ab_trees.main([f"--rounds={a.rounds}", f"--steps={a.steps}"] + [f"{os.path.basename(l)}={rig.ROOT}:{l}" for l in a.libs],
                  width=28, us_in_median=False)


if __name__ == "__main__":
    main()
