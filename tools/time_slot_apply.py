"""What the order-pinned multi-rank apply launch costs on the critical path of a shared-weights step (the price
of NOT folding the slot sum into the next step's weight staging). One GPU; the all-gather itself is not here (no second GPU): the
slots are this rank's own packed operand copied n_ranks times, which exercises the launch exactly as a node would after its gather.
    python tools/time_slot_apply.py [--ranks 8] [--steps 400]
Prints us per step-batch of (a) step with its own fused apply (independent shards: the headline), (b) step without apply + copy
into the slots + scg_apply_update_slots, (c) step without apply alone; (b) - (c) is what a fold into stage_w could remove at most."""
import argparse
import rig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=8); ap.add_argument("--steps", type=int, default=400); ap.add_argument("--envs", type=int, default=65536)
    a = ap.parse_args()
    import torch

    def run(mode):
        ag = rig.headline_agent(a.envs, 5)     # the headline workload (synthetic nested-disc initiation sets)
        ctx = ag.ctx
        gp = ctx.grad_packed()
        slots = torch.zeros((a.ranks, gp.numel()), dtype=torch.float32, device=gp.device)
        def one():
            if mode == "fused":
                ctx.step(ag.state, ag.W, ag.clf, ag.enabled_mask, ag.t, learn=True, apply=True)
            else:
                ctx.step(ag.state, ag.W, ag.clf, ag.enabled_mask, ag.t, learn=True, apply=False)
                if mode == "slots":
                    slots[0].copy_(gp)                       # (stands in for the all-gather's landing: the other slots stay zero operands)
                    ctx.apply_update_slots(ag.W, slots)
            ag.t += 1
        for _ in range(200): one()
        return rig.timed(one, a.steps) * 1e6

    res = {m: run(m) for m in ("fused", "slots", "noapply")}
    print(f"envs {a.envs} ranks {a.ranks} steps {a.steps}: step with fused apply {res['fused']:.2f} us; step + slot copy + scg_apply_update_slots "
          f"{res['slots']:.2f} us; step without any apply {res['noapply']:.2f} us; the slot apply on the critical path = {res['slots'] - res['noapply']:.2f} us "
          f"(of which a fold into the weight staging could remove at most that)")


if __name__ == "__main__":
    main()
