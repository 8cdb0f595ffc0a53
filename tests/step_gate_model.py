"""SPEC §26 (the step-batch under a gate table, scg_step_gated) emulated from oracle primitives, bit for bit.

The oracle knows no gate table, so one step-batch is rebuilt around sco_step, as tests/interrupt_learning_model.py does for §12:
  * sco_step gives the plain step. By §26.1 the gate's decision enters no update item of the step that takes it, so G, n_k and
    every output but the ids and qcache of the re-decided envs are the plain step's;
  * the physics is re-run (sco_pinball_step) for s', the classifiers (sco_classifier_predict) give §4.2's membership bits, and
    tests/option_rules.py's option_end and candidates give `keep` and `cand` at every env; §4.2's stay (an env that stays out of
    its candidate and is not due for a re-offer) is the two lines below. `entering` = not keep, cand >= 1, not stay;
  * sco_q_values at s_next under W gives §4.2's own decision (held against the plain step's ids: the derivation of `entering`
    and `cand` is checked on every step), and under the table's two sides with §5's max (rules.vmax) the gated decision of the
    options in the mask;
  * a flipped env's option_id is +-cand and its qcache Q(s_next, .) under W[cand] (entered) or W[0] (declined).

`scenario` holds the inputs the CPU and the GPU tests share, so that what the CPU test shows about them (the noisy table flips
offers both ways) holds for the GPU test's run."""
import numpy as np

import option_rules as rules
import sc_oracle
import skill_chaining_with_graphs_amd as scg
from util import HP, SCALE, copy_state, crossing_weights, random_env_state, wide_chain

NACT, NF = 5, 1296
N_OPT = 3
ENABLED = 0b1110
PARENTS = {"chain": [0, 0, 1, 2], "tree": [0, 0, 1, 1]}
STEPS = 12
T0 = 40


def shipped(W):
    """gatefit.shipped_gate on the host: [k][0] = W[k], [k][1] = W[0], row 0 zeros."""
    W = np.asarray(W, np.float32).reshape(-1, NACT, NF)
    g = np.zeros((len(W), 2, NACT, NF), np.float32)
    g[1:, 0] = W[1:]
    g[1:, 1] = W[0]
    return g


def full_mask(n_vf):
    return (1 << n_vf) - 2


def scenario(n, parents="chain", reoffer=4, env_id_base=0, seed=5):
    """(map, parents, clf [4][8], entry state, W [4][5][1296], hyper-parameters) of one test case: three options on nested discs
    round pinball_simple's goal that are entered everywhere, their weights the root's plus noise (V_o and V_0 cross both ways),
    envs running options, staying out of them and under the root."""
    m = scg.load_map("pinball_simple")
    clf = wide_chain(m, N_OPT)
    st = random_env_state(m, n, N_OPT, seed, id_lo=-N_OPT, id_hi=N_OPT, opt_steps_hi=10, max_episode_steps=HP["max_episode_steps"])
    W = crossing_weights(N_OPT + 1, seed + 1)
    hp = dict(HP, reoffer_period=reoffer, update_count_floor=8)
    return dict(map=m, parents=list(PARENTS[parents]), clf=clf, state=st, W=W, hp=hp, n=n, env_id_base=env_id_base, seed=3)


def make_oracle(sc, n_threads=4):
    orc = sc_oracle.Oracle(sc["map"], SCALE, n_envs=sc["n"], n_options=N_OPT, seed=sc["seed"], env_id_base=sc["env_id_base"],
                           enabled_mask=ENABLED, n_threads=n_threads, **sc["hp"])
    orc.set_parents(sc["parents"])
    return orc


def oracle_state(sc):
    st = sc_oracle.new_state(sc["n"], sc["map"])
    for f, v in sc["state"].items():
        st[f][...] = v
    return st


def step(orc, pre, W, clf, t, enabled, gate=None, gate_mask=0):
    """One step-batch of SPEC §26.1 from the entry state `pre` (dict of numpy arrays, not modified) under the weights W
    [n_vf][5][1296] (not modified), the table `gate` [n_vf][2][5][1296] and `gate_mask`. Returns (post state, G, n_k, info); info
    holds the masks `entering`, `plain_declined` (§4.2's decision on W), `declined` (the step's), `to_declined` / `to_entered`
    (where the two differ) and the candidates `cand`."""
    p = orc.p
    n, n_vf = len(pre["x"]), orc.n_vf
    parents = [int(p.parents[k]) for k in range(8)]
    W = np.ascontiguousarray(W, np.float32).reshape(n_vf, NACT, NF)
    clf = np.ascontiguousarray(clf, np.float32).reshape(n_vf, -1)
    post = copy_state(pre)
    G, n_k = orc.step(post, W, clf, t, enabled)
    xp, yp, vxp, vyp = (np.array(pre[f], np.float32, copy=True) for f in ("x", "y", "vx", "vy"))
    rew, goal = orc.pinball_step(xp, yp, vxp, vyp, post["action"])             # s' (before the reset)
    assert np.array_equal(rew.view(np.uint32), post["reward"].view(np.uint32))
    dn = post["done"].astype(np.int64)
    sn = [np.ascontiguousarray(post[f], np.float32) for f in ("x", "y", "vx", "vy")]
    member = lambda x, y: rules.membership(lambda px, py, k: orc.classifier_predict(px, py, clf[k]), x, y, n_vf, enabled)
    in_p, in_n = member(xp, yp), member(sn[0], sn[1])
    keep = rules.option_end(in_p, goal != 0, dn, pre["option_id"], pre["opt_steps"], parents, enabled, p.max_option_steps)["keep"]
    cand = np.where(keep, 0, rules.candidates(in_n, enabled, parents, n_vf))
    period = max(int(p.reoffer_period), 1)
    gid = np.arange(n, dtype=np.int64) + int(p.env_id_base)
    due = ((np.int64(t) + gid) & 0xffffffff) % period == 0
    stay = ~keep & (cand >= 1) & (dn == 0) & (np.asarray(pre["option_id"], np.int64) == -cand) & ~due     # SPEC §4.2's re-offer rule
    entering = ~keep & (cand >= 1) & ~stay
    idx = np.arange(n)
    qn = np.stack([orc.q_values(*sn, W[k]) for k in range(n_vf)])              # [n_vf][5][n]
    m = np.stack([rules.vmax(qn[k]) for k in range(n_vf)])
    with np.errstate(invalid="ignore"):
        plain_declined = entering & ~(m[cand, idx] >= m[0])
    # the derivation against the plain step: the ids it left
    want = np.where(keep, pre["option_id"], np.where(stay | plain_declined, -cand, cand))
    assert np.array_equal(post["option_id"], want.astype(np.int32)), "the model's entering / cand / stay are not the plain step's"
    declined = plain_declined.copy()
    for k in range(1, n_vf):
        if not (gate_mask >> k) & 1:
            continue
        e = np.nonzero(entering & (cand == k))[0]
        if not len(e):
            continue
        s = [np.ascontiguousarray(v[e]) for v in sn]
        v_opt, v_root = (rules.vmax(orc.q_values(*s, np.ascontiguousarray(gate[k][side], np.float32))) for side in (0, 1))
        with np.errstate(invalid="ignore"):
            declined[e] = ~(v_opt >= v_root)
    to_declined, to_entered = declined & ~plain_declined, plain_declined & ~declined
    e = np.nonzero(to_declined)[0]
    post["option_id"][e] = (-cand[e]).astype(np.int32)
    post["qcache"][:, e] = qn[0][:, e]
    e = np.nonzero(to_entered)[0]
    post["option_id"][e] = cand[e].astype(np.int32)
    post["qcache"][:, e] = qn[cand[e], :, e].T
    info = dict(entering=entering, cand=cand, plain_declined=plain_declined, declined=declined, to_declined=to_declined,
                to_entered=to_entered, stay=stay, keep=keep)
    return post, G, n_k, info


def apply(orc, W, G, n_k):
    """SPEC §5's apply on a copy of W."""
    W = np.array(W, np.float32, copy=True)
    orc.apply(W, G, n_k)
    return W


def noisy_gate(W, scale=None):
    """The shipped gate of W plus seeded noise on every option row: tests/test_gpu_population_gate.py's helper and its scale, for
    one policy (imported here, not at the top: that module is a GPU test's)."""
    import test_gpu_population_gate as PG
    return PG._noisy(np.asarray(W, np.float32)[None], PG.NOISE if scale is None else scale)[0]


def run(sc, steps=STEPS, gate_of=None, gate_mask=0, learn=True):
    """`steps` step-batches of the scenario from T0: per step (pre, W before, post, G, n_k, W after, info, gate). gate_of(W) makes
    the step's table (None: no table)."""
    orc = make_oracle(sc)
    st, W = oracle_state(sc), sc["W"].copy()
    out = []
    for j in range(steps):
        gate = None if gate_of is None else gate_of(W)
        pre = copy_state(st)
        post, G, n_k, info = step(orc, pre, W, sc["clf"], T0 + j, ENABLED, gate, gate_mask)
        W2 = apply(orc, W, G, n_k) if learn else W
        out.append(dict(pre=pre, W=W, post=post, G=G, n_k=n_k, W2=W2, info=info, gate=gate))
        st, W = copy_state(post), W2
        for f in ("action", "reward", "done"):                 # (copy_state covers EnvState.FIELDS)
            st[f] = post[f].copy()
    return out
