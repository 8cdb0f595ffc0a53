"""Who ends the reduce launch: per-workgroup clock stamps of reduce_kernel from the reduce timing build (`make -C .../csrc rstamps`;
SCG_RSTAMPS_LIB: another such library). Every workgroup leaves the 100 MHz clock at entry and at exit (stores drained), a slab
workgroup's wave 0 also where its own segment sums are parked, where it has passed the barrier and where G is summed. Printed per
kind of workgroup — commit rows, slab workgroups of the root, of the options — over --launches launches of the bench workload: when
they start and end after the launch's first entry, which kind holds the last workgroup to end, and the slab chain's pieces.
   python tools/reduce_chain.py [--launches 40]"""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
ap = argparse.ArgumentParser(); ap.add_argument("--options", type=int, default=5); ap.add_argument("--launches", type=int, default=40)
args = ap.parse_args()
from skill_chaining_with_graphs_amd import _lib
_lib.LIB_PATH = os.environ.get("SCG_RSTAMPS_LIB") or os.path.join(os.path.dirname(_lib.LIB_PATH), "libscg_hip_rstamps.so")
import numpy as np, torch
import bench
from skill_chaining_with_graphs_amd import SkillChainingAgent
n = bench.ENVS_PER_GPU
agent = SkillChainingAgent(bench.MAP, n, args.options, seed=0, **bench.HP)
agent.clf.copy_(torch.as_tensor(bench.chain_discs(agent.map, args.options)))
for k in range(1, args.options + 1): agent.enable_option(k)
agent.init_weights(std=1e-3); agent.domain.reset_random(seed=1000)
for _ in range(250): agent.step_batch()
torch.cuda.synchronize()
lib, ctx = agent.ctx.lib, agent.ctx._ctx
lib.scg_diag_reduce_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
lib.scg_diag_reduce_stamps.restype = C.c_int
nwg = lib.scg_diag_reduce_stamps(ctx, None, 1)
assert nwg > 0, "not a reduce timing build"
NCOL, n_vf, nrow = 26, args.options + 1, (n + 255) // 256
rows_y = nwg // NCOL - n_vf
kind = np.full(nwg, -1)                                  # -1: a row slot past the last row (leaves at once)
wg = np.arange(nwg)
kind[(wg // NCOL < rows_y) & (wg < nrow)] = 0            # commit rows (grid order: y major, the rows first)
kind[wg // NCOL >= rows_y] = 1 + (wg[wg // NCOL >= rows_y] // NCOL - rows_y)       # 1 + value function
names = {0: "commit rows", 1: "slab, root"}
names.update({1 + k: f"slab, option {k}" for k in range(1, n_vf)})
ends = {k: [] for k in names}; starts = {k: [] for k in names}; last_kind = []; spans = []; pieces = []
out = np.zeros((nwg, 8), np.uint64)
for _ in range(args.launches):
    agent.step_batch(); torch.cuda.synchronize()
    lib.scg_diag_reduce_stamps(ctx, out.ctypes.data_as(C.c_void_p), 1)
    t = out.astype(np.int64)
    t0 = t[kind >= 0, 0].min()
    end = np.where(kind == 0, t[:, 1:5].max(1), t[:, 1])
    live = kind >= 0
    spans.append((end[live].max() - t0) / 100.0)
    last_kind.append(int(kind[live][np.argmax(end[live])]))
    for k in names:
        ends[k].append((end[kind == k] - t0) / 100.0); starts[k].append((t[kind == k, 0] - t0) / 100.0)
    s = kind == 1                                        # the root's slab workgroups: every block holds a slab of theirs
    pieces.append(np.stack([t[s, 5] - t[s, 0], t[s, 6] - t[s, 5], t[s, 7] - t[s, 6], t[s, 1] - t[s, 7]], 1) / 100.0)
pc = lambda a, q: float(np.percentile(np.concatenate(a), q))
print(f"{os.path.basename(_lib.LIB_PATH)}: {args.launches} launches, {nwg} workgroups ({nrow} commit rows, {NCOL} x {n_vf} slab); us after the launch's first entry")
print(f"first entry -> last exit: median {np.median(spans):.2f}  min {np.min(spans):.2f}  max {np.max(spans):.2f}")
print(f"{'kind':16s} {'start p50':>9s} {'start max':>9s} | {'end p10':>8s} {'end p50':>8s} {'end p90':>8s} {'end max':>8s} {'mean of launch max':>19s} | ends the launch")
for k, nm in names.items():
    print(f"{nm:16s} {pc(starts[k], 50):9.2f} {pc(starts[k], 100):9.2f} | {pc(ends[k], 10):8.2f} {pc(ends[k], 50):8.2f} {pc(ends[k], 90):8.2f} {pc(ends[k], 100):8.2f} "
          f"{np.mean([e.max() for e in ends[k]]):19.2f} | {last_kind.count(k):3d} of {args.launches}")
p = np.concatenate(pieces)
print("root slab workgroups, wave 0, us (median / p90): entry -> own sums parked %.2f / %.2f; -> barrier passed %.2f / %.2f; "
      "-> G summed %.2f / %.2f; -> stores drained %.2f / %.2f" % tuple(v for j in range(4) for v in (np.median(p[:, j]), np.percentile(p[:, j], 90))))
