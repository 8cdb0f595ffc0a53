"""Where does the dispatcher put wave w of the step kernel's 16-wave workgroup? Every design note since round 3 ASSUMES SIMD = w % 4.
The light timing build (`make -C .../csrc lite`) stores HW_REG_HW_ID of every wave of every block of the last launch (slots 34..41);
this prints the wave -> SIMD table over all blocks.   python tools/wave_placement.py"""
import rig


def main():
    import numpy as np, torch
    agent = rig.headline_agent(65536, 5, library=rig.timing_library("lite"))
    for rep in range(3):
        rig.read_step_stamps(agent.ctx, True)
        for _ in range(20): agent.step_batch()
        torch.cuda.synchronize()
        out = rig.read_step_stamps(agent.ctx, False)
        nblk = len(out)
        hw = out[:, 34:42].copy().view(np.uint32).reshape(nblk, 16)
        simd, wid, cu, se = (hw >> 4) & 3, hw & 15, (hw >> 8) & 15, (hw >> 13) & 7
        print(f"launch set {rep}: wave -> SIMD_ID, blocks with that placement")
        pats, cnt = np.unique(simd, axis=0, return_counts=True)
        for p, c in sorted(zip(pats.tolist(), cnt.tolist()), key=lambda t: -t[1])[:8]:
            print("   ", "".join(str(v) for v in p), f" x {c}   per-SIMD wave counts {np.bincount(p, minlength=4).tolist()}")
        print("    is w % 4 everywhere:", bool((simd == (np.arange(16) % 4)[None, :]).all()), " is w // 4 everywhere:", bool((simd == (np.arange(16) // 4)[None, :]).all()))
        print("    SIMDs of waves 12, 13, 14 (the no-op's U2 waves), first 8 blocks:", simd[:8, 12:15].tolist())
        print("    WAVE_ID of waves 0..15, block 0:", wid[0].tolist(), " CU", cu[0, 0], "SE", se[0, 0])


if __name__ == "__main__":
    main()
