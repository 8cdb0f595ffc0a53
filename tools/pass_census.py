"""Which passes a step-batch of the headline workload runs: update and evaluation-only passes per block under SPEC §5's chunked
env order, re-made on the host from the option ids before and after one step.   python tools/pass_census.py"""
import rig


def main():
    import numpy as np
    from option_rules import env_order     # tests/: SPEC §5's env order on the host, perm[position] = env
    n=65536; nopt=5
    ag=rig.headline_agent(n,nopt,warm=200)
    key=lambda ids: np.where(ids>0,ids,0)               # SPEC §5: an env staying out of an option (a negative id) is keyed as the root's
    ids=ag.state.option_id.cpu().numpy().copy(); o=key(ids)
    ag.step_batch()
    on=key(ag.state.option_id.cpu().numpy())
    B=ag.ctx.block_envs
    tot=np.bincount(o,minlength=7); S=tot[1:].sum(); R=(tot[1:]>0).sum(); Bf=n//B
    c=min(B,-(-S//(Bf-R)))
    perm=env_order(ids,nopt+1,B)
    nb=n//B; upd_passes=0; eval_only=0; hist=np.zeros(8,int); items=[]
    for b in range(nb):
        e=perm[b*B:(b+1)*B]
        up=set(o[e].tolist())|{0}
        ev=set(on[e].tolist())
        eo=len(ev-up); eval_only+=eo; upd_passes+=len(up); hist[eo]+=1
        for v in ev-up: items.append(int((on[e]==v).sum()))
    print("blocks",nb,"chunk c",c,"update passes/block",upd_passes/nb,"eval-only passes/block",eval_only/nb,"hist of eval-only per block",hist.tolist())
    print("option counts",tot.tolist())

    items=np.array(items); print("items per evaluation-only pass: mean %.1f, median %d, p90 %d, max %d; quads mean %.2f" % (items.mean(), np.median(items), np.percentile(items,90), items.max(), np.ceil(items/4).mean()))


if __name__ == "__main__":
    main()
