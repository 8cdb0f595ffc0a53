"""tests/trace_model.py, the host model of SPEC §28.1's scan with a trace coefficient per row, against tests/lambda_model.py: the three
bit identities (no cut and one lambda; a cut that never fires; a cut that always fires is lambda = 0), the horizon against its Horner
form, a lambda per value function on hand-built edge rows with hand-computed values, and the condition on the synthetic action /
greedy-action pattern the device test relies on (cut and uncut coefficients in each of the three places a mix occurs). No GPU."""
import numpy as np
import pytest

import lambda_model as LM
import trace_model as TM

GAMMA = 0.99
LENGTHS = (0, 1, 2, 3, 14, 65, 130)
FIELDS = ("reward", "done", "vf", "term")
LAM_VF = (0.9, 0.3, 1.0)


def record(seed, all_done=False):
    """Envs over LENGTHS, three of each, the edge rows planted in every second env that has room; unless all_done every fifth env is
    a cut record. v0, vk arbitrary binary32 values; action / ag in SPEC §28.3's pattern."""
    rng = np.random.default_rng(seed)
    envs = []
    for e in range(3 * len(LENGTHS)):
        L = LENGTHS[e % len(LENGTHS)]
        env = LM.synthetic_env(rng, L, end_done=all_done or e % 5 != 4)
        envs.append(LM.plant_edges(env) if L >= 12 and e % 2 else env)
    flat = LM.flatten(envs)
    total = int(flat["offsets"][-1])
    flat["v0"], flat["vk"] = (rng.normal(0, 50, total).astype(np.float32) for _ in range(2))
    flat["action"], flat["ag"] = TM.synthetic_actions(rng, flat)
    return flat


def trace(flat, lam_vf, flags, R, coefficients=None, gamma=GAMMA, **over):
    f = dict(flat, **over)
    return TM.trace_returns(f["offsets"], len(f["reward"]), *[f[k] for k in FIELDS], f["action"], f["ag"], f["v0"], f["vk"], gamma, lam_vf,
                            flags, R, coefficients=coefficients)


def peng(flat, lam, R, gamma=GAMMA):
    return LM.lambda_returns(flat["offsets"], len(flat["reward"]), *[flat[k] for k in FIELDS], flat["v0"], flat["vk"], gamma, lam, R)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def step_rows(flat):
    L = np.diff(flat["offsets"])
    env = np.repeat(np.arange(len(L)), L)
    return (np.arange(len(env)) - flat["offsets"][:-1][env]) >= 1


def greedy_everywhere(flat):
    """ag with action[i] == ag[i - 1] on every row (the env borders included: harmless, no coefficient is read across one)."""
    return np.concatenate([flat["action"][1:], [255]]).astype(np.uint8)


def greedy_nowhere(flat):
    return ((np.concatenate([flat["action"][1:], [0]]) + 1) % 5).astype(np.uint8)


@pytest.mark.parametrize("R", [0.0, 100.0])
@pytest.mark.parametrize("lam", [0.0, 0.3, 0.9, 1.0])
def test_one_lambda_without_the_cut_is_the_lambda_return(lam, R):
    flat = record(7)
    want = peng(flat, lam, R)
    for lam_vf in ([lam], [lam] * 3):
        y0, yk, _ = trace(flat, lam_vf, 0, R)
        assert same_bits(y0, want[0]) and same_bits(yk, want[1]), lam_vf
    assert np.any(want[1] != 0) and np.isfinite(want[0]).all()


@pytest.mark.parametrize("lam", [0.3, 0.9, 1.0])
def test_a_cut_that_never_fires_changes_nothing(lam):
    flat = record(8)
    want = peng(flat, lam, 100.0)
    y0, yk, h = trace(flat, [lam] * 3, TM.TRACE_CUT, 100.0, ag=greedy_everywhere(flat))
    assert same_bits(y0, want[0]) and same_bits(yk, want[1])
    assert same_bits(h, trace(flat, [lam] * 3, 0, 100.0)[2])


@pytest.mark.parametrize("lam", [0.3, 0.9, 1.0])
def test_a_cut_that_always_fires_is_lambda_zero(lam):
    flat = record(9)
    want = peng(flat, 0.0, 100.0)
    for ag in (greedy_nowhere(flat), np.full(len(flat["reward"]), 255, np.uint8)):
        y0, yk, h = trace(flat, [lam] * 3, TM.TRACE_CUT, 100.0, ag=ag)
        assert same_bits(y0, want[0]) and same_bits(yk, want[1])
        step = step_rows(flat)
        assert np.all(h[step] == 1.0) and not h[~step].any()
    assert not same_bits(want[0], peng(flat, lam, 100.0)[0])


@pytest.mark.parametrize("lam", [0.0, 0.5, 0.9, 1.0])
def test_the_horizon_is_the_geometric_sum_in_horner_form(lam):
    flat = record(10, all_done=True)
    _, _, h = trace(flat, [lam] * 3, 0, 0.0)
    horner = [1.0]
    for _ in range(max(LENGTHS)):
        horner.append(1.0 + lam * horner[-1])                  # H_0 = 1 on the done row, H_{m+1} = 1 + lambda H_m
    off = flat["offsets"]
    for e in range(len(off) - 1):
        L = int(off[e + 1] - off[e])
        want = [0.0] + [horner[L - 1 - j] for j in range(1, L)]
        assert same_bits(h[off[e]: off[e + 1]], want[:L]), e
    if lam == 1.0:                                             # the plain number of steps to the end
        assert h[off[-2] + 1] == float(off[-1] - off[-2] - 1)


def test_a_lambda_per_value_function_on_hand_built_edge_rows():
    """One env of 12 rows, plant_edges' rows: the coefficient of every mix is the one of the NEXT row's value function, also where
    an option ends and the root carries on."""
    g, R = 0.99, 100.0
    lam = dict(enumerate(LAM_VF))                              # root 0.9, option 1 0.3, option 2 1.0
    env = {"reward": np.array([0, -1.5, -2.25, -1, -3.5, -1.25, -2, -4.75, -1.125, -3, -2.5, 10000.5], np.float32),
           "done": np.array([0] * 11 + [1], np.uint8), "vf": np.zeros(12, np.uint8), "term": np.zeros(12, np.uint8)}
    LM.plant_edges(env)
    assert list(env["vf"]) == [0, 2, 2, 2, 2, 2, 0, 1, 1, 2, 2, 0] and list(env["term"]) == [0, 0, 4, 0, 0, 5, 0, 0, 1, 0, 3, 0]
    flat = LM.flatten([env])
    v0 = [7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47]
    vk = [2, 3, 5, 8, 12, 20, 33, 54, 88, 143, 232, 376]
    flat["v0"], flat["vk"] = np.array(v0, np.float32), np.array(vk, np.float32)
    flat["action"] = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1], np.uint8)
    flat["ag"] = greedy_everywhere(flat)
    r = [float(v) for v in env["reward"]]
    c = [None] + [lam[int(k)] for k in env["vf"][1:]]          # c[i]: the coefficient row i carries
    assert c[1:] == [1.0, 1.0, 1.0, 1.0, 1.0, 0.9, 0.3, 0.3, 1.0, 1.0, 0.9]
    mix = lambda ci, b, y: (1.0 - ci) * b + ci * y

    def by_hand(c):
        w0, wk = [0.0] * 12, [0.0] * 12
        w0[11] = r[11]
        for j in range(10, 0, -1):
            w0[j] = r[j] + g * mix(c[j + 1], float(v0[j]), w0[j + 1])
        wk[10] = (r[10] + 0.0) + g * mix(c[11], float(v0[10]), w0[11])       # LEFT_INITIATION: over to the root, the ROOT's coefficient
        wk[9] = (r[9] + 0.0) + g * mix(c[10], float(vk[9]), wk[10])
        wk[8] = (r[8] + R) + g * mix(c[9], float(v0[8]), w0[9])              # SUCCESS: the bonus; the next row is option 2's
        wk[7] = (r[7] + 0.0) + g * mix(c[8], float(vk[7]), wk[8])
        wk[5] = (r[5] + 0.0) + g * mix(c[6], float(v0[5]), w0[6])            # INTERRUPTED: over to the root
        wk[4] = (r[4] + 0.0) + g * mix(c[5], float(vk[4]), wk[5])
        wk[3] = (r[3] + 0.0) + g * mix(c[4], float(vk[3]), wk[4])
        wk[2] = (r[2] + 0.0) + g * mix(c[3], float(v0[2]), w0[3])            # TIMEOUT: over to the root although row 3 has the same vf
        wk[1] = (r[1] + 0.0) + g * mix(c[2], float(vk[1]), wk[2])
        hh = [0.0] * 12
        hh[11] = 1.0
        for j in range(10, 0, -1):
            hh[j] = 1.0 + c[j + 1] * hh[j + 1]
        return w0, wk, hh

    w0, wk, hh = by_hand(c)
    for flags in (0, TM.TRACE_CUT):
        y0, yk, h = trace(flat, LAM_VF, flags, R, gamma=g)
        assert same_bits(y0, w0) and same_bits(yk, wk) and same_bits(h, hh), flags
    # the choice matters: the ending option's own coefficient at rows 10 (1.0 for 0.9) and 8 (0.3 for 1.0) gives other values
    assert wk[10] != (r[10] + 0.0) + g * mix(lam[2], float(v0[10]), w0[11])
    assert wk[8] != (r[8] + R) + g * mix(lam[1], float(v0[8]), w0[9])
    # a vf beyond n_lam reads lam_vf[0]
    y0, yk, _ = trace(flat, LAM_VF[:2], 0, R, gamma=g)
    w0b, wkb, _ = by_hand([None] + [lam[int(k)] if k < 2 else lam[0] for k in env["vf"][1:]])
    assert same_bits(y0, w0b) and same_bits(yk, wkb) and not same_bits(yk, wk)
    # cuts at rows 3 (behind the TIMEOUT: "boot"), 6 (root stream and "boot" of the INTERRUPTED row) and 8 (option 1 going on: "own")
    ag = flat["ag"].copy()
    ag[[2, 5, 7]] = [255, 4, 0]
    assert all(ag[i - 1] != flat["action"][i] for i in (3, 6, 8))
    cc = list(c)
    cc[3] = cc[6] = cc[8] = 0.0
    w0c, wkc, hc = by_hand(cc)
    y0, yk, h = trace(flat, LAM_VF, TM.TRACE_CUT, R, gamma=g, ag=ag)
    assert same_bits(y0, w0c) and same_bits(yk, wkc) and same_bits(h, hc)
    assert yk[2] == (r[2] + 0.0) + g * float(v0[2]) and yk[7] == (r[7] + 0.0) + g * float(vk[7]) and y0[5] == r[5] + g * float(v0[5])
    assert hc[5] == 1.0 and hc[4] == 2.0 and hc[7] == 1.0
    assert same_bits(trace(flat, LAM_VF, 0, R, gamma=g, ag=ag)[1], wk)           # without the flag ag is not looked at


def test_the_synthetic_pattern_cuts_and_keeps_in_every_place_of_a_mix():
    flat = record(11)
    R = 100.0
    seen = []
    cut = trace(flat, LAM_VF, TM.TRACE_CUT, R, coefficients=seen)
    unc = trace(flat, LAM_VF, 0, R)
    vf = flat["vf"]
    for place, stream in (("root", 0), ("own", 1), ("boot", 1)):
        rows_cut = [i for i, p, c in seen if p == place and c == 0.0]
        rows_kept = [i for i, p, c in seen if p == place and c != 0.0]
        assert len(rows_cut) >= 1 and len(rows_kept) >= 1, place
        assert {LAM_VF[vf[i + 1]] for i in rows_kept} == {c for i, p, c in seen if p == place and c != 0.0}
        for i in rows_cut:                                     # the cut target is the one-step target, and not the uncut one
            assert cut[stream][i] != unc[stream][i], (place, i)
    # every cut coefficient sits where the recorded action is not the greedy one, and only there
    for i, _, c in seen:
        assert (c == 0.0) == (flat["action"][i + 1] != flat["ag"][i]), i
    # a record's env borders: the last row of an env reads no coefficient
    last = flat["offsets"][1:][np.diff(flat["offsets"]) > 0] - 1
    assert not ({i for i, _, _ in seen} & set(int(v) for v in last))
