"""The HIP example collectors — scg_harvest, scg_collect_examples (two launches, and one after scg_arm_collect),
scg_collect_frontier — against the numpy models of SPEC §7 (tests/collect_model.py) and §13 (tests/frontier_model.py, with
the test's own cover decision), bit for bit, at the edges where prefix sums, wave scans, ballots and lane-parallel gathers go
wrong. The collectors read only the trace arrays, the classifier rows and the caller's buffers, so every trace here but the
armed path's is written by tests/collect_cases.py into the context's own trace tensors and no step runs. Every buffer lies
between 64 rows of sentinels in front of it and behind it; compare_buffers() also demands the sentinel in every row at or beyond
the fill level.

What runs (ids name n, ring_len H, hit density, ev_len family, l_pos+l_neg, capacity mode, prev_in, event bits, masks):

§7 scg_collect_examples, un-armed (collect_cases.collect_cases)
  A  hit density {none, all, env0, envlast, lane63, lane0, fullrow, altwaves, rand1, rand50, rand99} x EVERY size
     {1, 63, 64, 65, 255, 256, 257, 4097, 65536, 65537, 70000, 262144} (the last three take the second trip of the cross-row
     loop), ev_len mixed; (l_pos, l_neg), ring_len {1, 2, 64, 256} (<= 64 from 65536 envs, <= 2 at 262144: memory), event bits
     {1, 2, 0b100100, 0b111111} and prev_in {None, random, zeros} rotate over the cases. At n > 65537 the dense families use
     L <= 5 so that count_0 + sum v stays near a million rows.
  B  (l_pos, l_neg) {(1,0), (0,1), (0,5), (5,0), (32,32), (33,32), (100,100), (1,255)} x ring_len {1, 2, 64, 256} x ev_len
     {0, 1, ring_len-1, ring_len, ring_len+1, 10^6, mixed} at n = 257, and (l_pos, l_neg) x ring_len with ev_len mixed at
     n = 4097: v, the wrap and the gather loop's second trip (v > 64) depend on the env alone, not on n.
  C  capacity {roomy, cap = 1, exactly count_0 + sum v, one less, cut in the middle of an env, count_0 = cap, append
     (count_0 > 0), cap = 0 (through the C ABI, one-element buffer), count_0 = -3} at n = 65, 257, 4097, 65537.
  D  prev_in with all four (in, prev) combinations at random at n = 63, 257, 4097, 70000, 262144; every case with prev_in
     checks prev_in for every env and calls a second time on the unchanged trace, which must append nothing.
§13 scg_collect_frontier, n_options = 5 (collect_cases.frontier_cases)
  FA every density x every size up to 4097, a third of the densities at each larger size; masks {goal only / cover 0; goal + set
     3 / cover set 3; all six nodes / every set; two nodes / every set; target_mask 0; set 5 alone} and nodes per hit env
     {1, 2, all 6, mixed} rotate; each node its own count_0, one shared cap; untargeted nodes keep count and sentinels.
  FB (l_pos, l_neg) x ring_len at n = 257, and every ev_len family (0 on hit envs: skipped) at ring_len 2 and 64.
  FC the capacity modes (cap = 0 aside: refused) at n = 257 and 4097.
  Every s_t clears 4 x tol_z of ref64.clf_model for every set (asserted by the generator): no env is left out.
scg_harvest (collect_cases.HARVEST_CASES): unsorted and duplicate sel_env, n_sel = 1 and 0, n_sel * L = 255 / 256 / 257,
  L > ring_len, n up to 262144; the output lies between sentinels too.
The armed path on real step-batches: block_envs {64, 128, 256} x n {257, 3000, 70000} x {LEARN|APPLY, LEARN + scg_apply_update,
  acting only, LEARN|INTERRUPT, a gestating option}; after every step-batch the trace is read back, the model run on it, and
  buffers, count and prev_in compared. At n = 3000 / 256 also, between step and collect: a rollout, a recorded rollout, option
  trials, a collect_frontier, scg_invalidate_order, and a skipped collect.
Refusals of l_pos + l_neg beyond INT32_MAX in all four entry points (no launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import collect_cases as cc
import collect_model as cm
import skill_chaining_with_graphs_amd as scg
from gpu_util import dev
from skill_chaining_with_graphs_amd.core import EnvState, ScgContext
from util import HP, chain_classifiers, random_states, random_weights

pytestmark = pytest.mark.gpu

CASES, FCASES = cc.collect_cases(), cc.frontier_cases()
G = cc.GUARD
_CTX = {}


def context(n, ring_len, block_envs=256, **kw):
    """One context at a time (the large ones hold a lot of memory), its trace tensors re-made when ring_len changes."""
    key = (n, block_envs, tuple(sorted(kw.items())))
    if _CTX.get("key") != key:
        if "ctx" in _CTX:
            _CTX["ctx"].close()
        _CTX.clear()
        hp = dict(HP)
        hp.update(kw)
        _CTX.update(key=key, ctx=ScgContext(n, cc.N_OPTIONS, scg.load_map("pinball_simple"), device=0, seed=3,
                                            block_envs=block_envs, **hp), ring_len=None)
    ctx = _CTX["ctx"]
    if _CTX["ring_len"] != ring_len:
        ctx.set_trace_buffers(ring_len)
        _CTX["ring_len"] = ring_len
    return ctx


def put_trace(ctx, tr):
    for t, a in zip(ctx._trace, (tr["ring_x"], tr["ring_y"], tr["events"], tr["ev_len"])):
        t.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def framed(a):
    """A device tensor holding `a` between G rows of its sentinel; returns (whole, the part in between)."""
    fill = cm.XY_SENTINEL if a.dtype == np.float32 else cm.LABEL_SENTINEL
    whole = np.concatenate([np.full((G,) + a.shape[1:], fill, a.dtype), a])
    t = dev(whole)
    return t, t[G:]


def front_ok(whole, what):
    head = whole[:G].cpu().numpy()
    bad = (cm._bits(head) != cm.XY_SENTINEL_BITS) if head.dtype == np.float32 else (head != cm.LABEL_SENTINEL)
    assert not bad.any(), f"{what}: written in front of the buffer, first at row {int(np.nonzero(bad.reshape(G, -1).any(1))[0][0]) - G}"


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_collect_examples_equals_the_model(case):
    tr, cap, (xy0, lab0, cnt0, prev0), want = cc.setup_collect(case, np.random.default_rng(len(case["id"]) * 7919 + case["n"]))
    ctx = context(case["n"], case["ring_len"])
    put_trace(ctx, tr)
    xy_w, xy = framed(xy0)                                 # xy0 / lab0 carry G guard rows behind cap already
    lab_w, lab = framed(lab0)
    cnt, prev = dev(cnt0), None if prev0 is None else dev(prev0)

    def call():
        if cap == 0:                                       # the wrapper sizes cap from the buffer: cap = 0 goes through the C ABI
            ctx._call("scg_collect_examples", C.c_uint32(case["bits"]), C.c_void_p(prev.data_ptr() if prev is not None else 0),
                      case["l_pos"], case["l_neg"], C.c_void_p(xy.data_ptr()), C.c_void_p(lab.data_ptr()),
                      C.c_void_p(cnt.data_ptr()), 0, ctx._stream())
        else:
            ctx.collect_examples(case["bits"], prev, case["l_pos"], case["l_neg"], xy[:cap].view(-1), lab[:cap], cnt, rearm=False)

    def check(what):
        torch.cuda.synchronize()
        cm.compare_buffers(xy.cpu().numpy(), lab.cpu().numpy(), cnt.cpu().numpy(), want[0], want[1], want[2], cap, G,
                           got_prev=None if prev is None else prev.cpu().numpy(), want_prev=want[3], what=what)
        front_ok(xy_w, what); front_ok(lab_w, what)

    call()
    check(case["id"])
    if prev is not None:                                   # unchanged trace: nobody enters, nothing is appended
        cm.collect(tr["ring_x"], tr["ring_y"], tr["events"], tr["ev_len"], case["bits"], want[3], case["l_pos"], case["l_neg"],
                   want[0], want[1], want[2], cap=cap)
        call()
        check(case["id"] + " (second call)")


@pytest.mark.parametrize("case", FCASES, ids=[c["id"] for c in FCASES])
def test_collect_frontier_equals_the_model(case):
    tr, cap, (xy0, lab0, cnt0), want = cc.setup_frontier(case, np.random.default_rng(len(case["id"]) * 104729 + case["n"]))
    ctx = context(case["n"], case["ring_len"])
    put_trace(ctx, tr)
    n_vf = cc.N_OPTIONS + 1
    tail_xy, tail_lab = np.full((G, 2), cm.XY_SENTINEL, np.float32), np.full(G, cm.LABEL_SENTINEL, np.uint8)
    xy_w, xy = framed(np.concatenate([xy0.reshape(-1, 2), tail_xy]))
    lab_w, lab = framed(np.concatenate([lab0.reshape(-1), tail_lab]))
    cnt, clf = dev(cnt0), dev(tr["clf"])
    target, cover = case["masks"]
    ctx.collect_frontier(target, cover, clf.view(-1), case["l_pos"], case["l_neg"], xy[:n_vf * cap].view(-1), lab[:n_vf * cap], cnt)
    torch.cuda.synchronize()
    gxy, glab = xy.cpu().numpy(), lab.cpu().numpy()
    cm.compare_nodes(gxy[:n_vf * cap].reshape(n_vf, cap, 2), glab[:n_vf * cap].reshape(n_vf, cap), cnt.cpu().numpy(), want[0],
                     want[1], want[2], cap, guard_xy=gxy[n_vf * cap:], guard_label=glab[n_vf * cap:], what=case["id"])
    front_ok(xy_w, case["id"]); front_ok(lab_w, case["id"])
    for t, a in zip(ctx._trace, (tr["ring_x"], tr["ring_y"], tr["events"], tr["ev_len"])):       # the trace is left as it was
        assert np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8))


@pytest.mark.parametrize("hc", cc.HARVEST_CASES, ids=[f"n{h[0]}-H{h[1]}-L{h[2]}+{h[3]}-{h[4]}" for h in cc.HARVEST_CASES])
def test_harvest_equals_the_model(hc):
    n, H, l_pos, l_neg, mode = hc
    rng = np.random.default_rng(n + H)
    tr = cc.build_trace(n, H, ("rand50", "mixed"), rng)
    sel = cc.harvest_selection(n, mode, rng)
    assert len(sel) == 0 or (sel.min() >= 0 and sel.max() < n)
    ctx = context(n, H)
    put_trace(ctx, tr)
    L, total = l_pos + l_neg, len(sel) * (l_pos + l_neg)
    wxy, wlab = cm.harvest(tr["ring_x"], tr["ring_y"], tr["ev_len"], sel, l_pos, l_neg)
    xy0, lab0, _ = cm.fresh_buffers(total, G)
    xy_w, xy = framed(xy0)
    lab_w, lab = framed(lab0)
    sel_d = dev(sel) if len(sel) else torch.zeros(1, dtype=torch.int32, device="cuda:0")
    ring_x, ring_y, _, ev_len = ctx._trace
    P = lambda t: C.c_void_p(t.data_ptr())
    ctx._call("scg_harvest", len(sel), P(sel_d), P(ring_x), P(ring_y), H, P(ev_len), l_pos, l_neg, P(xy), P(lab), ctx._stream())
    torch.cuda.synchronize()
    xy0[:total], lab0[:total] = wxy.reshape(-1, 2), wlab.reshape(-1)
    cm.compare_buffers(xy.cpu().numpy(), lab.cpu().numpy(), [total], xy0, lab0, [total], total, G, what="harvest")
    front_ok(xy_w, "harvest"); front_ok(lab_w, "harvest")
    if len(sel):                                           # the wrapper's own output, the same rows
        gxy, glab = ctx.harvest(sel_d, l_pos, l_neg)
        assert np.array_equal(cm._bits(gxy.cpu().numpy()), cm._bits(wxy)) and np.array_equal(glab.cpu().numpy(), wlab)


def test_sum_overflow_refusals_launch_nothing():
    """l_pos + l_neg is formed in 64 bits by all four entry points: a sum beyond INT32_MAX is SCG_ERR_INVALID."""
    ctx = context(257, 2)
    xy_w, xy = framed(cm.fresh_buffers(8, G)[0])
    lab_w, lab = framed(cm.fresh_buffers(8, G)[1])
    cnt, sel, clf = dev(np.array([2] * 6, np.int32)), dev(np.zeros(1, np.int32)), dev(cc.band_classifiers())
    ring_x, ring_y, _, ev_len = ctx._trace
    P, big = (lambda t: C.c_void_p(t.data_ptr())), 2 ** 31 - 1
    lib = ctx.lib
    for lp, ln in ((big, 1), (1, big), (big, big), (2 ** 30, 2 ** 30)):
        assert lib.scg_collect_examples(ctx._ctx, C.c_uint32(1), None, lp, ln, P(xy), P(lab), P(cnt), 8, None) == -1
        assert lib.scg_arm_collect(ctx._ctx, C.c_uint32(1), None, lp, ln, P(cnt)) == -1
        assert lib.scg_harvest(ctx._ctx, 1, P(sel), P(ring_x), P(ring_y), 2, P(ev_len), lp, ln, P(xy), P(lab), None) == -1
        assert lib.scg_collect_frontier(ctx._ctx, C.c_uint32(1), C.c_uint32(0), P(clf), lp, ln, P(xy), P(lab), P(cnt), 1, None) == -1
    torch.cuda.synchronize()
    assert cnt.tolist() == [2] * 6
    assert (cm._bits(xy_w.cpu().numpy()) == cm.XY_SENTINEL_BITS).all() and bool((lab_w == int(cm.LABEL_SENTINEL)).all())


# ---------------------------------------------------------------------------------------------------- the armed path
FLAVOURS = ("fused", "split_apply", "acting", "interrupt", "gestating")
BETWEEN = ("rollout", "recorded_rollout", "trials", "frontier", "invalidate_order", "skipped_collect")


def _armed_run(block_envs, n, flavour, between=None, steps=5):
    H, l_pos, l_neg, nopt = 16, 6, 5, cc.N_OPTIONS
    ctx = context(n, H, block_envs, max_episode_steps=12)
    m = ctx.map
    mask, bits = (0b000010, 0b000100) if flavour == "gestating" else (0b111110, 0b000010)
    ctx.set_gestation(0b000100 if flavour == "gestating" else 0)
    st = EnvState(n, ctx.device, m)
    x, y, vx, vy = random_states(m, n, 17, vmax=1.5)
    for t_, a in zip(st.state(), (x, y, vx, vy)):
        t_.copy_(dev(a))
    st.ep_steps.copy_(dev(np.random.default_rng(n).integers(0, 11, n).astype(np.int32)))
    W, clf = dev(random_weights(nopt + 1, 5, std=0.05)), dev(chain_classifiers(m, nopt))
    Gb, n_k = ctx.grad_buffers()
    cap = max(3 * n // 2, 40)
    xy0, lab0, cnt0 = cm.fresh_buffers(cap, G)
    want = [xy0.copy(), lab0.copy(), cnt0.copy(), np.zeros(n, np.uint8)]
    xy_w, xy = framed(xy0)
    lab_w, lab = framed(lab0)
    cnt, prev = dev(cnt0), dev(want[3])
    fr = [dev(a) for a in cm.fresh_buffers(64, 0, 0, n_nodes=nopt + 1)]
    st2 = EnvState(n, ctx.device, m)
    appended = 0

    def step(t):
        kw = dict(fused={}, split_apply=dict(apply=False), acting=dict(learn=False), interrupt=dict(interrupt=True), gestating={})
        ctx.step(st, W.view(-1), clf.view(-1), mask, t, **kw[flavour])
        if flavour == "split_apply":
            ctx.apply_update(W.view(-1), Gb, n_k)

    for t in range(steps):
        step(t)
        if between == "skipped_collect" and t % 2 == 0:
            continue                                       # no collect behind this step: its announced totals go stale
        trace0 = [a.clone() for a in ctx._trace]
        if between == "rollout":
            ctx.rollout(st2, W.view(-1), clf.view(-1), mask, 100 + t, 3, begin=True)
        elif between == "recorded_rollout":
            from skill_chaining_with_graphs_amd.trajectory import Trajectory
            ctx.rollout(st2, W.view(-1), clf.view(-1), mask, 100 + t, 3, begin=True, record=Trajectory(n, 4, 0, ctx.device))
        elif between == "trials":
            from skill_chaining_with_graphs_amd.trials import TrialResult
            res = TrialResult(n, np.full(n, 1, np.int32), ctx.device)
            ctx.option_trials(st.x.clone(), st.y.clone(), st.vx.clone(), st.vy.clone(), res.option, W.view(-1), clf.view(-1),
                              mask, 100 + t, res)
        elif between == "frontier":
            ctx.collect_frontier(0b000011, 0b000010, clf.view(-1), 3, 3, fr[0].view(-1), fr[1].view(-1), fr[2])
        elif between == "invalidate_order":
            ctx.invalidate_order()
        ctx.collect_examples(bits, prev, l_pos, l_neg, xy[:cap].view(-1), lab[:cap], cnt)        # rearm: announced for the next step
        torch.cuda.synchronize()
        for a, b in zip(trace0, ctx._trace):
            assert torch.equal(a, b), "the call between step and collect changed the trace"
        rx, ry, ev, el = (a.cpu().numpy() for a in ctx._trace)
        before = int(want[2][0])
        cm.collect(rx, ry, ev, el, bits, want[3], l_pos, l_neg, want[0], want[1], want[2], cap=cap)
        appended += int(want[2][0]) - before
        what = f"armed b{block_envs} n{n} {flavour} {between} t={t}"
        cm.compare_buffers(xy.cpu().numpy(), lab.cpu().numpy(), cnt.cpu().numpy(), want[0], want[1], want[2], cap, G,
                           got_prev=prev.cpu().numpy(), want_prev=want[3], what=what)
        front_ok(xy_w, what); front_ok(lab_w, what)
    ctx.disarm_collect()
    ctx.set_gestation(0)
    return appended


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("n", [257, 3000, 70000])
@pytest.mark.parametrize("block_envs", [64, 128, 256])
def test_armed_collect_equals_the_model_after_every_step(block_envs, n, flavour):
    appended = _armed_run(block_envs, n, flavour)
    assert n < 3000 or appended > 0, "no env entered the region: the case checked nothing"


@pytest.mark.parametrize("between", BETWEEN)
def test_armed_collect_survives_the_calls_that_promise_to_leave_it_alone(between):
    assert _armed_run(256, 3000, "fused", between=between, steps=6) > 0


def teardown_module(module):
    if "ctx" in _CTX:
        _CTX["ctx"].close()
    _CTX.clear()
