"""SPEC §12 (the interrupting learner) emulated from oracle primitives, bit for bit.

The oracle knows no interruption, so one step-batch of scg_step(LEARN | INTERRUPT) is rebuilt around sco_step:
  * sco_step gives the plain step; by §12 only the interrupted envs' outputs and the options' G differ from it;
  * the physics is re-run (sco_pinball_step) for s', the classifiers (sco_classifier_predict) give §4.2's membership bits, and
    sco_q_values gives every value function's max at s_next (SPEC §5's max order), so `keep`, `interrupted` and the candidate c
    follow from §4.2 and §12 directly (tests/option_rules.py's option_end, interrupted and candidates);
  * the env order is rebuilt from the option ids at entry (§5's chunked and padded layouts), and every option VF's block partials
    are recomputed with sco_q_update_grad on exactly that block's update items in position order, with cont = 0 and r = the
    item's target (with cont = 0 the target is r itself), the targets made with libm's fmaf; blocks without items are skipped
    and the partials summed in §5's two levels.
"""
import ctypes as C
import ctypes.util

import numpy as np

import option_rules as rules
import sc_oracle
from util import copy_state

NACT, NF, SEG = 5, 1296, 16

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.fmaf.restype = C.c_float
_libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]


def fmaf(a, b, c):
    """float32 fma, element by element (Python 3.10 has no math.fma)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    return np.array([_libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())],
                    np.float32).reshape(a.shape)


def step(orc, pre, W, clf, t, enabled, gest=0, interrupt=True, recompute=True):
    """One learning step-batch of SPEC §12 from the entry state `pre` (dict of numpy arrays, not modified) and the weights W
    [n_vf][5][1296] (not modified). Returns (post state, G [n_vf][5][1296], n_k, info); info holds the masks `keep` and
    `interrupted`, the candidates `cand` and the maxima `m` [n_vf][n]. interrupt=False is the plain step (G of the options
    still recomputed when `recompute`: that is what shows the recomputation is right)."""
    p = orc.p
    n, n_vf = len(pre["x"]), orc.n_vf
    B = sc_oracle.BLOCK_ENVS
    gamma, r_succ = np.float32(p.gamma), np.float32(p.r_option_success)
    parents = [int(p.parents[k]) for k in range(8)]
    known = enabled | gest
    W = np.ascontiguousarray(W, np.float32).reshape(n_vf, NACT, NF)
    clf = np.ascontiguousarray(clf, np.float32).reshape(n_vf, -1)
    post = copy_state(pre)
    G0, nk0 = orc.step(post, W, clf, t, enabled)                   # the plain step (acting outputs, the root's G)
    a = post["action"]
    xp, yp, vxp, vyp = (np.array(pre[f], np.float32, copy=True) for f in ("x", "y", "vx", "vy"))
    rew, goal = orc.pinball_step(xp, yp, vxp, vyp, a)              # s' (before the reset)
    assert np.array_equal(rew.view(np.uint32), post["reward"].view(np.uint32))
    dn = post["done"].astype(np.int64)
    sn = [post[f] for f in ("x", "y", "vx", "vy")]
    s = [np.ascontiguousarray(pre[f], np.float32) for f in ("x", "y", "vx", "vy")]
    member = lambda x, y: rules.membership(lambda px, py, k: orc.classifier_predict(px, py, clf[k]), x, y, n_vf, known)
    in_p, in_n, in_s = member(xp, yp), member(sn[0], sn[1]), member(s[0], s[1])
    goal = goal != 0
    end = rules.option_end(in_p, goal, dn, pre["option_id"], pre["opt_steps"], parents, known, p.max_option_steps)
    o, succ, term, keep = end["o"], end["succ"], end["term"], end["keep"]
    r_o = (post["reward"] + np.where(succ, r_succ, np.float32(0))).astype(np.float32)
    qn = np.stack([orc.q_values(*sn, W[k]) for k in range(n_vf)])  # [n_vf][5][n]
    m = np.stack([rules.vmax(qn[k]) for k in range(n_vf)])
    interrupted = rules.interrupted(keep, m, o) if interrupt else np.zeros(n, bool)
    cand = rules.candidates(in_n, enabled, parents, n_vf)
    e = np.nonzero(interrupted)[0]
    post["option_id"][e] = (-cand[e]).astype(np.int32)
    post["opt_steps"][e] = 0
    post["qcache"][:, e] = qn[0][:, e]
    G, n_k = G0.copy(), nk0.copy()
    if recompute or interrupted.any():
        perm = rules.env_order(pre["option_id"], n_vf, B)
        nblk = -(-n // B)
        for k in range(1, n_vf):
            own = o == k
            gst = ~own & (((gest >> k) & 1) == 1) & in_s[k]
            end_k = rules.option_end(in_p, goal, dn, np.full(n, k), pre["opt_steps"], parents, known, p.max_option_steps)
            succ_k, fail_k = end_k["succ"], end_k["fail"]          # option k's own end at every env (its gestation items)
            r_k = (post["reward"] + np.where(succ_k, r_succ, np.float32(0))).astype(np.float32)
            cont_k = np.where((dn != 0) | succ_k | fail_k, np.float32(0), gamma).astype(np.float32)
            cont_o = np.where(keep, gamma, np.float32(0)).astype(np.float32)
            parts = []                                             # (block, partial, count) of the blocks with items
            for b in range(nblk):
                pos = perm[b * B:(b + 1) * B]
                items = pos[own[pos] | gst[pos]]
                if len(items) == 0:
                    continue
                io = own[items]
                r = np.where(io, r_o[items], r_k[items]).astype(np.float32)
                cont = np.where(io, cont_o[items], cont_k[items]).astype(np.float32)
                boot = np.where(io, term[items] & (dn[items] == 0), (dn[items] == 0) & (succ_k[items] | fail_k[items]))
                tgt = np.where(boot, fmaf(gamma, m[0][items], r),
                               np.where(cont > 0, fmaf(cont, m[k][items], r), r)).astype(np.float32)
                cut = interrupted[items] & io                      # SPEC §12: the exit rule's bootstrap (own items only: an
                                                                   #  env's gestation items of another option are unchanged)
                tgt[cut] = fmaf(gamma, m[0][items][cut], r[cut])
                Gb, cnt = orc.q_update_grad([v[items] for v in s], a[items], tgt, np.zeros(len(items), np.float32),
                                            [v[items] for v in sn], W[k])
                parts.append((b, Gb, cnt))
            g, tot = None, 0
            for s0 in range(0, nblk, SEG):
                seg = [P for b, P, _ in parts if s0 <= b < s0 + SEG]
                if not seg:
                    continue
                T = seg[0].copy()
                for P in seg[1:]:
                    T = (T + P).astype(np.float32)
                g = T if g is None else (g + T).astype(np.float32)
            tot = sum(c for _, _, c in parts)
            assert tot == nk0[k], (k, tot, nk0[k])                 # §12: the item set does not change
            G[k] = g if g is not None else np.zeros((NACT, NF), np.float32)
    info = dict(keep=keep, interrupted=interrupted, cand=cand, m=m)
    return post, G, n_k, info


def apply(orc, W, G, n_k):
    """SPEC §5's apply on a copy of W."""
    W = np.array(W, np.float32, copy=True)
    orc.apply(W, G, n_k)
    return W
