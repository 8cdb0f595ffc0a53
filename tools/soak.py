"""Soak: 30 000 learning step-batches of the bench workload on one GPU; prints the asynchronous status word, whether W stayed finite,
|W|max and how many envs sit in an option at the end (rounds 2 and 3 print the same numbers: the arithmetic did not change)."""
import time
import rig


def main():
    import torch
    ag = rig.headline_agent(65536, 5)
    t0=time.time()
    for i in range(30000): ag.step_batch()
    torch.cuda.synchronize()
    print("30000 learning steps in %.1f s; status word %d; W finite %s |W|max %.1f; envs in an option %d; goals this step %d" % (
        time.time()-t0, ag.ctx.async_status(True), bool(torch.isfinite(ag.W).all()), float(ag.W.abs().max()), int((ag.state.option_id>0).sum()), int((ag.state.done==1).sum())))


if __name__ == "__main__":
    main()
