"""The action mix of the headline workload after 300 / 1000 / 3000 step-batches, and what it means for U2's SIMD loads per block
(DESIGN §10).   python tools/action_skew.py"""
import rig


def main():
    import numpy as np
    n = 65536
    ag = rig.headline_agent(n, 5)
    for t in (300, 1000, 3000):
        while ag.t < t: ag.step_batch()
        a = ag.state.action.cpu().numpy()
        print("t", t, "action shares", np.round(np.bincount(a, minlength=5) / n, 3).tolist())
    # per block (in the env order the kernel uses: approximate by env id blocks of 256)
    a = ag.state.action.cpu().numpy().reshape(-1, 256)
    cnt = np.stack([(a == k).sum(1) for k in range(5)], 1)
    g = (cnt + 3) // 4
    S = np.stack([g[:, 0] + g[:, 1] + g[:, 2] + g[:, 4], g[:, 0] + g[:, 1] + g[:, 3] + g[:, 4], g[:, 0] + g[:, 2] + g[:, 3] + g[:, 4], g[:, 1] + g[:, 2] + g[:, 3]], 1)
    print("groups per action per block: mean", g.mean(0).round(1).tolist(), "max-SIMD load / mean-SIMD load per block: mean %.3f" % (S.max(1) / (g.sum(1) * 15 / 16 / 4 * 1.0)).mean(), " (SIMD loads mean", S.mean(0).round(1).tolist(), ")")


if __name__ == "__main__":
    main()
