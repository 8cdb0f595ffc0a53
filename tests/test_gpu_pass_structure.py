"""The step kernel's pass structure: the merged pass alone, one and several single-VF passes behind it, the
value gate and SPEC §12's rewrite behind a single pass, and the two un-fused entry points that run the same pass body.

Every case seats a batch so that the structure it is about occurs in the first step-batch, runs five step-batches on the build's
block size B (n = B + B/4: a full block and a partial one; n = 2B) and compares the env state, G, n_k and W with the oracle by
bits after each. `_passes` restates SPEC §5's env order and the kernel's choice of passes on the host, from the option ids and
the classifiers alone; `_reference` counts over the five steps what occurred, and a case whose structure did not occur fails
(it cannot pass on the merged pass alone). The seeds were chosen on the CPU oracle so that the counts hold on all three builds.

The plain step's reference is the oracle's own sco_step; the interrupting step's is tests/interrupt_learning_model.py (the
oracle knows no interruption), which also hands out the masks and maxima the structure checks read."""
import numpy as np
import pytest
import torch

import interrupt_learning_model as ilm
import option_rules as rules
import sc_oracle
from bits import assert_bits_equal
from gpu_util import as_bytes, assert_same_bits, block_envs, dev, make_pair, state_to_device      # noqa: F401 (block_envs: a fixture)
from ref64 import env_order_layout
from util import copy_state, crossing_weights, disc_weights, random_states, random_weights

pytestmark = pytest.mark.gpu

BLOCKS = [64, 128, 256]
SHAPES = ["1.25B", "2B"]
STEPS = 5
RADII = (0.3, 0.55, 0.85)         # nested discs round the goal: zone z = inside disc z + 1 and outside disc z; zone 3 = outside all


def _n(B, shape):
    return B + B // 4 if shape == "1.25B" else 2 * B


# Cases: n_options, enabled mask, gestation mask, then the seating as (share of the envs, option id, zone) — an env running
# option k sits inside I_k and outside its target's set (it goes on), a root env in zone z has option z + 1 as its candidate
# if that one is enabled — and the seed.
CASES = {
    # 1. the merged pass only
    "merged": dict(n_opt=1, enabled=0b10, gest=0, seats=[(0.4, 1, 0), (0.3, 0, 0), (0.3, 0, 1)], seed=11),
    "no_option": dict(n_opt=1, enabled=0b10, gest=0, seats=[(0.5, 0, 0), (0.5, 0, 1)], seed=12),
    # 2. one single pass: option 2 gestates, its off-policy items lie in the block whose option is 1
    "one_single": dict(n_opt=2, enabled=0b010, gest=0b100, seats=[(0.4, 1, 0), (0.3, 0, 0), (0.2, 0, 1), (0.1, 0, 3)], seed=13),
    # 3. two single passes: two gestating options beside the block's option; the padded order (three running options, U B > n)
    "two_gestating": dict(n_opt=3, enabled=0b0010, gest=0b1100, seats=[(0.4, 1, 0), (0.2, 0, 0), (0.2, 0, 1), (0.2, 0, 2)], seed=14),
    "padded": dict(n_opt=3, enabled=0b1110, gest=0, seats=[(0.3, 1, 0), (0.3, 2, 1), (0.3, 3, 2), (0.1, 0, 3)], seed=15),
    # 4. the gate behind a single pass: root envs inside I_2 (outside I_1) in the block that holds option 2's run behind option 1's
    "gate_single": dict(n_opt=3, enabled=0b1110, gest=0, seats=[(0.3, 1, 0), (0.3, 2, 1), (0.3, 3, 2), (0.1, 0, 1)], seed=16),
}


def _clf(m, n_opt):
    clf = np.zeros((n_opt + 1, 8), np.float32)
    tx, ty, _ = m.target
    for k in range(1, n_opt + 1):
        clf[k] = disc_weights(tx, ty, RADII[k - 1])
    return clf


def _seat(case, m, orc, n):
    """The entry state: every env takes a collision-free state of its zone from a seeded pool; env ids are shuffled over the
    seats so that the env order is no identity."""
    c = CASES[case]
    rng = np.random.default_rng(c["seed"])
    px, py, pvx, pvy = random_states(m, 8192, 1000 + c["seed"], vmax=1.0)
    tx, ty, _ = m.target
    d = np.hypot(px.astype(np.float64) - tx, py.astype(np.float64) - ty)
    lo, hi = np.array((0.0,) + RADII), np.array(RADII + (9.0,))
    zone = np.full(len(d), -1)
    for z in range(4):                                          # (7 % clear of either rim: s' and s_next stay in the zone as a rule)
        zone[(d > 1.07 * lo[z]) & (d < 0.93 * hi[z])] = z
    st = sc_oracle.new_state(n, m)
    envs = rng.permutation(n)
    lo = 0
    for i, (share, oid, z) in enumerate(c["seats"]):
        hi = n if i == len(c["seats"]) - 1 else lo + int(round(share * n))
        pick = rng.choice(np.nonzero(zone == z)[0], hi - lo, replace=False)
        e = envs[lo:hi]
        st["x"][e], st["y"][e], st["vx"][e], st["vy"][e] = px[pick], py[pick], pvx[pick], pvy[pick]
        st["option_id"][e] = oid
        lo = hi
    st["opt_steps"][:] = rng.integers(0, 5, n)
    st["ep_steps"][:] = rng.integers(0, 20, n)
    st["qcache"][:] = rng.standard_normal((5, n)).astype(np.float32)
    return st


def _passes(pre, clf, orc, n_vf, B, gest, learn):
    """SPEC §5's env order and the passes of every block, restated: the block's option kB is the option of position 0 if it does
    not gestate and its envs are the block's position prefix (it shares the merged pass with the root); every other option with
    an update item in the block — an env running it, or (gestating) an env whose s lies in its set — takes a single pass."""
    oid = pre["option_id"].astype(np.int64)
    o = rules.vf_of(oid, n_vf)
    perm = rules.env_order(oid, n_vf, B)
    in_s = rules.membership(lambda x, y, k: orc.classifier_predict(x, y, clf[k]), pre["x"], pre["y"], n_vf, gest)   # (read where k gestates)
    blocks, block_of = [], np.zeros(len(o), np.int64)
    for b in range(0, len(perm), B):
        pos = perm[b:b + B]
        ob = o[pos]
        k0, cnt = int(ob[0]), int((ob == ob[0]).sum())
        kB = k0 if k0 >= 1 and not (gest >> k0) & 1 and bool((ob[:cnt] == k0).all()) else -1
        singles, off = [], 0
        for k in range(1, n_vf):
            own = ob == k
            gst = ~own & in_s[k][pos] if (gest >> k) & 1 else np.zeros(len(pos), bool)
            if learn and k != kB and (own | gst).any():
                singles.append(k)
            off += int(gst.sum())
        block_of[pos] = len(blocks)
        blocks.append(dict(kB=kB, singles=singles, off_policy=off if learn else 0, running=sorted(set(ob[ob >= 1].tolist()))))
    return blocks, block_of


def _reference(case, orc, m, n, B, interrupt=False, learn=True):
    """Five step-batches on the oracle: [(post state, G, n_k, W after the apply)] and the counts of what occurred."""
    c = CASES[case]
    n_vf = c["n_opt"] + 1
    clf = _clf(m, c["n_opt"])
    st = _seat(case, m, orc, n)
    W = crossing_weights(n_vf, c["seed"])
    orc.set_gestation(c["gest"])
    seen = dict(merged_only=0, kB_blocks=0, no_kB_blocks=0, one_single=0, two_singles=0, two_running=0, off_policy=0, accepted=0,
                declined=0, accepted_single=0, declined_single=0, interrupted=0, interrupted_single=0, first=None)
    out = [(copy_state(st), None, None, W)]
    for t in range(STEPS):
        blocks, block_of = _passes(st, clf, orc, n_vf, B, c["gest"], learn)
        post, G, n_k, info = ilm.step(orc, st, W, clf, 50 + t, c["enabled"], gest=c["gest"], interrupt=interrupt, recompute=interrupt)
        idx = np.arange(n)
        entering = ~info["keep"] & (info["cand"] >= 1)                                   # (reoffer_period 1: every candidate is offered)
        holds = info["m"][info["cand"], idx] >= info["m"][0]
        acc, dec = entering & holds, entering & ~holds
        assert np.array_equal(post["option_id"][acc], info["cand"][acc]) and np.all(post["option_id"][dec] <= 0)
        behind = np.array([info["cand"][e] in blocks[block_of[e]]["singles"] for e in idx])   # the env's candidate has a single pass in its block
        o_run = np.where(st["option_id"] >= 1, st["option_id"], 0)
        cut_single = info["interrupted"] & np.array([o_run[e] in blocks[block_of[e]]["singles"] for e in idx])
        now = dict(merged_only=sum(not b["singles"] for b in blocks), kB_blocks=sum(b["kB"] >= 1 for b in blocks),
                   no_kB_blocks=sum(b["kB"] < 0 for b in blocks), one_single=sum(b["kB"] >= 1 and len(b["singles"]) == 1 for b in blocks),
                   two_singles=sum(len(b["singles"]) >= 2 for b in blocks), two_running=sum(len(b["running"]) >= 2 for b in blocks),
                   off_policy=sum(b["off_policy"] for b in blocks), accepted=int(acc.sum()), declined=int(dec.sum()),
                   accepted_single=int((acc & behind).sum()), declined_single=int((dec & behind).sum()),
                   interrupted=int(info["interrupted"].sum()), interrupted_single=int(cut_single.sum()))
        if t == 0:
            seen["first"] = dict(now, blocks=blocks, layout=env_order_layout(st["option_id"], n_vf, B))
        for k, v in now.items():
            seen[k] += int(v)
        if learn:
            W = ilm.apply(orc, W, G, n_k)
        st = post
        out.append((post, G, n_k, W))
    return out, seen, clf


def _pair(case, n, **hp):
    c = CASES[case]
    return make_pair("pinball_simple", n, n_options=c["n_opt"], seed=c["seed"], enabled_mask=c["enabled"], reoffer_period=1, **hp)


def _run(case, B, shape, interrupt=False, learn=True):
    """The five step-batches on the device, each compared with the reference by bits; returns the counts of what occurred."""
    c = CASES[case]
    n = _n(B, shape)
    ctx, orc, m = _pair(case, n)
    ref, seen, clf = _reference(case, orc, m, n, B, interrupt=interrupt, learn=learn)
    ctx.set_gestation(c["gest"])
    st = state_to_device(ref[0][0], ctx)
    W, clf_d = dev(ref[0][3]).view(-1), dev(clf).view(-1)
    G_d, nk_d = ctx.grad_buffers()
    for t in range(STEPS):
        post, G, n_k, W_h = ref[t + 1]
        ctx.step(st, W, clf_d, c["enabled"], 50 + t, learn=learn, apply=True, interrupt=interrupt)
        torch.cuda.synchronize()
        msg = f"{case} B {B} n {n} step {t}"
        assert_same_bits(st, post, msg=msg)
        if learn:
            assert np.array_equal(nk_d.cpu().numpy(), n_k), (msg, nk_d.cpu().numpy(), n_k)
            assert_bits_equal(G_d.cpu().numpy(), G, msg=msg + " G:")
        assert np.array_equal(as_bytes(W), as_bytes(W_h.reshape(-1))), msg + ": W differs"
    assert ctx.async_status(synchronize=True) == 0
    return seen


def _check_structure(case, seen, shape, interrupt=False, learn=True):
    """What the case is about occurred — in the first step-batch where the seating decides it, over the five otherwise."""
    first = seen["first"]
    assert seen["accepted"] >= 1 and seen["declined"] >= 1, seen
    if case == "merged":
        assert first["kB_blocks"] >= 1 and first["merged_only"] == len(first["blocks"]) and first["layout"] == "chunked", first
        assert seen["two_singles"] == seen["one_single"] == 0, seen          # root + one enabled option: never a single pass
    elif case == "no_option":
        assert first["kB_blocks"] == 0 and first["merged_only"] == len(first["blocks"]), first
    elif case == "one_single":
        assert first["one_single"] >= 1 and first["off_policy"] >= 1 and first["layout"] == "chunked", first
    elif case == "two_gestating":
        assert any(b["kB"] == 1 and b["singles"] == [2, 3] for b in first["blocks"]) and first["off_policy"] >= 2, first
    elif case == "padded":
        assert first["layout"] == "padded" and first["two_running"] >= 1, first
        assert any(b["kB"] >= 1 and b["singles"] for b in first["blocks"]), first
        if shape == "1.25B":
            assert first["two_singles"] >= 1, first                           # all three runs meet in block 0
    elif case == "gate_single":
        assert first["layout"] == "padded" and first["two_running"] >= 1, first
        assert seen["accepted_single"] >= 1 and seen["declined_single"] >= 1, seen
    if interrupt:
        assert seen["interrupted"] >= 1, seen
        if case in ("padded", "gate_single"):
            assert seen["interrupted_single"] >= 1, seen                      # SPEC §12's rewrite behind option k's own single pass


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("block_envs", BLOCKS, indirect=True)
@pytest.mark.parametrize("case", ["merged", "no_option"])
def test_merged_pass_only(case, block_envs, shape):
    _check_structure(case, _run(case, block_envs, shape), shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("block_envs", BLOCKS, indirect=True)
def test_merged_pass_only_acting(block_envs, shape):
    """Acting-only step-batches: no helper waves, the weights staged inside the pass, no U1 / U2, the gate behind E."""
    seen = _run("merged", block_envs, shape, learn=False)
    _check_structure("merged", seen, shape, learn=False)
    assert seen["off_policy"] == 0 and seen["one_single"] == 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("block_envs", BLOCKS, indirect=True)
@pytest.mark.parametrize("interrupt", [False, True], ids=["plain", "interrupt"])
@pytest.mark.parametrize("case", ["one_single", "two_gestating", "padded", "gate_single"])
def test_single_passes_behind_the_merged_pass(case, interrupt, block_envs, shape):
    _check_structure(case, _run(case, block_envs, shape, interrupt=interrupt), shape, interrupt=interrupt)


@pytest.mark.parametrize("block_envs", BLOCKS, indirect=True)
def test_q_update_and_q_values_one_env_past_a_block(block_envs):
    """scg_q_update and scg_q_values run the merged pass's body on one value function: n = B + 1, the second block holds one item."""
    n, k = block_envs + 1, 1
    ctx, orc, m = make_pair("pinball_simple", n, n_options=2)
    s, sn = random_states(m, n, 21), random_states(m, n, 22)
    rng = np.random.default_rng(23)
    act = rng.integers(0, 5, n).astype(np.uint8)
    r = rng.choice([-1.0, -5.0, 100.0], n).astype(np.float32)
    cont = np.where(rng.random(n) < 0.3, 0.0, 0.99).astype(np.float32)
    W = random_weights(3, 24, std=0.5)
    assert_bits_equal(ctx.q_values([dev(a) for a in sn], dev(W[k]).view(-1)).cpu().numpy(), orc.q_values(*sn, W[k]), msg="q_values:")
    G_o, cnt = orc.q_update_grad(s, act, r, cont, sn, W[k])
    n_k = np.zeros(3, np.int32)
    n_k[k] = cnt
    G_all = np.zeros((3, 5, 1296), np.float32)
    G_all[k] = G_o
    W_o = W.copy()
    orc.apply(W_o, G_all, n_k)
    W_d = dev(W.copy())
    G_d, n_d = ctx.grad_buffers()
    ctx.q_update(k, [dev(a) for a in s], dev(act), dev(r), dev(cont), [dev(a) for a in sn], W_d.view(-1))
    assert cnt == n and n_d.cpu().numpy().tolist() == n_k.tolist()
    assert_bits_equal(G_d[k].cpu().numpy(), G_o, msg="G:")
    assert_bits_equal(W_d.cpu().numpy(), W_o, msg="W:")
