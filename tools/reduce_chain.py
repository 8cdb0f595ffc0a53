"""Who ends the reduce launch: per-workgroup clock stamps of reduce_kernel from the reduce timing build (`make -C .../csrc rstamps`;
SCG_RSTAMPS_LIB: another such library). Every workgroup leaves the 100 MHz clock at entry and at exit (stores drained), a slab
workgroup's wave 0 also where its own segment sums are parked, where it has passed the barrier and where G is summed. Printed per
kind of workgroup — commit rows, slab workgroups of the root, of the options — over --launches launches of the bench workload: when
they start and end after the launch's first entry, which kind holds the last workgroup to end, the slab chain's pieces, how far
apart the waves of a root slab workgroup park their sums, and a commit row's wave 0 from entry to the record, the barrier and the end.
   python tools/reduce_chain.py [--launches 40] [--ncol 26 --waves 16: a library whose slab workgroups own 64 columns]"""
import argparse, os
import rig


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("--options", type=int, default=5); ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--ncol", type=int, default=rig.RED_NCOL); ap.add_argument("--waves", type=int, default=rig.RED_WAVES)
    args = ap.parse_args()
    import numpy as np, torch
    path = rig.timing_library("rstamps")
    agent = rig.headline_agent(options=args.options, warm=250, library=path)
    NCOL, n_vf, nrow = args.ncol, agent.n_vf, (agent.n_envs + 255) // 256
    nwg = len(rig.read_reduce_stamps(agent.ctx, True, NCOL))
    rows_y = nwg // NCOL - n_vf
    kind = np.full(nwg, -1)                                  # -1: a row slot past the last row (leaves at once)
    wg = np.arange(nwg)
    kind[(wg // NCOL < rows_y) & (wg < nrow)] = 0            # commit rows (grid order: y major, the rows first)
    kind[wg // NCOL >= rows_y] = 1 + (wg[wg // NCOL >= rows_y] // NCOL - rows_y)       # 1 + value function
    names = {0: "commit rows", 1: "slab, root"}
    names.update({1 + k: f"slab, option {k}" for k in range(1, n_vf)})
    ends = {k: [] for k in names}; starts = {k: [] for k in names}; last_kind = []; spans = []; pieces = []; parks = []; rows = []
    for _ in range(args.launches):
        agent.step_batch(); torch.cuda.synchronize()
        t = rig.read_reduce_stamps(agent.ctx, True, NCOL).astype(np.int64)
        t0 = t[kind >= 0, 0].min()
        end = np.where(kind == 0, t[:, 1:5].max(1), t[:, 1])
        live = kind >= 0
        spans.append((end[live].max() - t0) / 100.0)
        last_kind.append(int(kind[live][np.argmax(end[live])]))
        for k in names:
            ends[k].append((end[kind == k] - t0) / 100.0); starts[k].append((t[kind == k, 0] - t0) / 100.0)
        s = kind == 1                                        # the root's slab workgroups: every block holds a slab of theirs
        pieces.append(np.stack([t[s, 5] - t[s, 0], t[s, 6] - t[s, 5], t[s, 7] - t[s, 6], t[s, 1] - t[s, 7]], 1) / 100.0)
        park = t[s, 8:8 + args.waves] - t[s, 0:1]            # every wave's sums parked, after the workgroup's entry
        parks.append(np.stack([park.min(1), park.max(1)], 1) / 100.0)
        r = kind == 0                                        # a commit row's wave 0
        rows.append(np.stack([t[r, 5] - t[r, 0], t[r, 6] - t[r, 5], t[r, 1] - t[r, 6]], 1) / 100.0)
    pc = lambda a, q: float(np.percentile(np.concatenate(a), q))
    print(f"{os.path.basename(path)}: {args.launches} launches, {nwg} workgroups ({nrow} commit rows, {NCOL} x {n_vf} slab); us after the launch's first entry")
    print(f"first entry -> last exit: median {np.median(spans):.2f}  min {np.min(spans):.2f}  max {np.max(spans):.2f}")
    print(f"{'kind':16s} {'start p50':>9s} {'start max':>9s} | {'end p10':>8s} {'end p50':>8s} {'end p90':>8s} {'end max':>8s} {'mean of launch max':>19s} | ends the launch")
    for k, nm in names.items():
        print(f"{nm:16s} {pc(starts[k], 50):9.2f} {pc(starts[k], 100):9.2f} | {pc(ends[k], 10):8.2f} {pc(ends[k], 50):8.2f} {pc(ends[k], 90):8.2f} {pc(ends[k], 100):8.2f} "
              f"{np.mean([e.max() for e in ends[k]]):19.2f} | {last_kind.count(k):3d} of {args.launches}")
    p = np.concatenate(pieces)
    print("root slab workgroups, wave 0, us (median / p90): entry -> own sums parked %.2f / %.2f; -> barrier passed %.2f / %.2f; "
          "-> G summed %.2f / %.2f; -> stores drained %.2f / %.2f" % tuple(v for j in range(4) for v in (np.median(p[:, j]), np.percentile(p[:, j], 90))))
    k = np.concatenate(parks)
    if (k >= 0).all():                                       # (a library without the per-wave slots leaves zeros there)
        print("root slab workgroups, sums parked after entry, us: first wave median %.2f, last wave median %.2f, last - first median %.2f / p90 %.2f"
              % (np.median(k[:, 0]), np.median(k[:, 1]), np.median(k[:, 1] - k[:, 0]), np.percentile(k[:, 1] - k[:, 0], 90)))
    w = np.concatenate(rows)
    if (w >= 0).all():
        print("commit rows, wave 0, us (median / p90): entry -> record arrived %.2f / %.2f; -> barrier passed %.2f / %.2f; -> stores drained %.2f / %.2f"
              % tuple(v for j in range(3) for v in (np.median(w[:, j]), np.percentile(w[:, j], 90))))


if __name__ == "__main__":
    main()
