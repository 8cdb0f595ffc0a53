"""The numpy models of the example collectors (SPEC §7: tests/collect_model.py, written from the SPEC's text; §13:
tests/frontier_model.py) on the CPU: against the oracle's sco_harvest / sco_collect_examples and, for §13, the model with the
test's own cover decision against the model with the oracle's predict, on every hand-built family of tests/collect_cases.py up to
70 000 envs; and nine wrong answers that compare_buffers() must refuse. This is what validates the models before
tests/test_gpu_collect_edges.py holds the HIP collectors to them."""
import numpy as np
import pytest

import collect_cases as cc
import collect_model as cm
import frontier_model as fm
import sc_oracle
from sc_oracle import _p

CASES = cc.collect_cases(cc.CPU_SIZES)
FCASES = cc.frontier_cases(cc.CPU_SIZES)
ids = lambda cases: [c["id"] for c in cases]


def oracle_collect(tr, case, cap, xy, lab, cnt, prev):
    """sco_collect_examples on the buffer's first cap rows (it knows no negative fill level and no cap = 0 buffer: the model's
    reading of those two is the SPEC's formula, checked on the GPU)."""
    n, H = tr["ring_x"].shape[1], tr["ring_x"].shape[0]
    import ctypes as C
    sc_oracle.lib().sco_collect_examples(n, _p(tr["events"]), _p(prev), C.c_uint32(case["bits"]), _p(tr["ring_x"]), _p(tr["ring_y"]),
                                         H, _p(tr["ev_len"]), case["l_pos"], case["l_neg"], _p(xy), _p(lab), _p(cnt), cap)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_collect_model_equals_the_oracle(case, oracle_mod):
    tr, cap, (xy, lab, cnt, prev), want = cc.setup_collect(case, np.random.default_rng(len(case["id"]) * 7919 + case["n"]))
    if case["capmode"] == "neg":
        # the oracle would write in front of the buffer; without the dropped rows the model must equal a run from level 0
        xy2, lab2, cnt2 = xy.copy(), lab.copy(), np.zeros(1, np.int32)
        prev2 = None if prev is None else prev.copy()
        cm.collect(tr["ring_x"], tr["ring_y"], tr["events"], tr["ev_len"], case["bits"], prev2, case["l_pos"], case["l_neg"],
                   xy2, lab2, cnt2, cap=cap)
        k = int(want[2][0])
        assert k == max(int(cnt2[0]) - 3, -3) and np.array_equal(cm._bits(want[0][:k]), cm._bits(xy2[3:3 + k]))
        assert np.array_equal(want[1][:k], lab2[3:3 + k])
        return
    oracle_collect(tr, case, cap, xy, lab, cnt, prev)
    cm.compare_buffers(xy, lab, cnt, want[0], want[1], want[2], cap, cc.GUARD, got_prev=prev, want_prev=want[3], what=case["id"])
    if prev is not None:                      # a second call on the unchanged trace appends nothing
        before = (xy.copy(), lab.copy(), cnt.copy())
        cm.collect(tr["ring_x"], tr["ring_y"], tr["events"], tr["ev_len"], case["bits"], want[3], case["l_pos"], case["l_neg"],
                   want[0], want[1], want[2], cap=cap)
        cm.compare_buffers(before[0], before[1], before[2], want[0], want[1], want[2], cap, cc.GUARD, what=case["id"] + " again")


@pytest.mark.parametrize("case", FCASES, ids=ids(FCASES))
def test_frontier_model_with_its_own_cover_equals_the_model_with_the_oracles_predict(case, oracle_mod):
    tr, cap, (xy, lab, cnt), want = cc.setup_frontier(case, np.random.default_rng(len(case["id"]) * 104729 + case["n"]))
    target, cover = case["masks"]
    fm.collect_frontier(tr["ring_x"], tr["ring_y"], tr["events"], tr["ev_len"], target, cover, tr["clf"], case["l_pos"],
                        case["l_neg"], xy, lab, cnt)
    cm.compare_nodes(xy, lab, cnt, want[0], want[1], want[2], cap, what=case["id"])
    untouched = [p for p in range(6) if not (target >> p) & 1]
    assert all(want[2][p] == cnt[p] for p in untouched)


@pytest.mark.parametrize("hc", cc.HARVEST_CASES, ids=[f"n{h[0]}-H{h[1]}-L{h[2]}+{h[3]}-{h[4]}" for h in cc.HARVEST_CASES])
def test_harvest_model_equals_the_oracle(hc, oracle_mod):
    n, H, l_pos, l_neg, mode = hc
    rng = np.random.default_rng(n + H)
    tr = cc.build_trace(n, H, ("rand50", "mixed"), rng)
    sel = cc.harvest_selection(n, mode, rng)
    L = l_pos + l_neg
    xy, lab = np.zeros((len(sel), L, 2), np.float32), np.zeros((len(sel), L), np.uint8)
    if len(sel):
        sc_oracle.lib().sco_harvest(len(sel), _p(sel), _p(tr["ring_x"]), _p(tr["ring_y"]), H, n, _p(tr["ev_len"]), l_pos, l_neg,
                                    _p(xy), _p(lab))
    wxy, wlab = cm.harvest(tr["ring_x"], tr["ring_y"], tr["ev_len"], sel, l_pos, l_neg)
    assert np.array_equal(cm._bits(xy), cm._bits(wxy)) and np.array_equal(lab, wlab)
    if L > H or mode != "none" and tr["ev_len"][sel].min() < L:
        assert (wlab == 255).any()


# ---------------------------------------------------------------------------------------------------- wrong answers
def _good(prev="random", capmode="roomy", n=300, ring_len=4, lpn=(3, 2), density="rand50", evf="million"):
    case = cc._case("M", n, ring_len, density, evf, lpn, capmode=capmode, prev=prev)
    tr, cap, init, want = cc.setup_collect(case, np.random.default_rng(5))
    got = [a.copy() if a is not None else None for a in want]
    return case, tr, cap, init, want, got


def _refused(got, want, cap, match):
    with pytest.raises(AssertionError, match=match):
        cm.compare_buffers(got[0], got[1], got[2], want[0], want[1], want[2], cap, cc.GUARD, got_prev=got[3], want_prev=want[3])


def test_compare_accepts_the_right_answer():
    _, _, cap, _, want, got = _good()
    cm.compare_buffers(got[0], got[1], got[2], want[0], want[1], want[2], cap, cc.GUARD, got_prev=got[3], want_prev=want[3])


def test_compare_refuses_two_envs_row_groups_swapped():
    _, _, cap, _, want, got = _good()                     # every hit env holds 4 rows (ring_len 4 < L = 5)
    got[0][0:4], got[0][4:8] = want[0][4:8], want[0][0:4]
    _refused(got, want, cap, r"ex_xy differs first at position 0 ")


def test_compare_refuses_ages_descending_inside_one_env():
    _, _, cap, _, want, got = _good()
    got[0][8:12] = want[0][8:12][::-1]
    _refused(got, want, cap, r"ex_xy differs first at position 8 ")


@pytest.mark.parametrize("age", [3, 2])                   # l_pos = 3: the first negative row, and the last positive one
def test_compare_refuses_the_label_flipped_at_the_l_pos_boundary(age):
    _, _, cap, _, want, got = _good(ring_len=8)           # 5 rows per env
    assert want[1][5:10].tolist() == [1, 1, 1, 0, 0]
    got[1][5 + age] ^= 1
    _refused(got, want, cap, rf"ex_label differs first at position {5 + age} ")


def test_compare_refuses_a_ring_index_off_by_one_after_a_wrap():
    case, tr, cap, _, want, got = _good()                 # ev_len = 10^6: the slots wrap
    v = cm.rows_per_env(tr["events"], tr["ev_len"], 1, _[3], 5, 4)[1]
    e = int(np.nonzero(v)[0][0])
    slot = (int(tr["ev_len"][e]) - 1 - 1 + 1) & 3         # age 1 read one slot too far on
    got[0][1] = (tr["ring_x"][slot, e], tr["ring_y"][slot, e])
    _refused(got, want, cap, r"ex_xy differs first at position 1 ")


def test_compare_refuses_a_count_not_clamped_to_cap():
    _, _, cap, _, want, got = _good(capmode="oneless")
    assert want[2][0] == cap
    got[2][0] = cap + 1
    _refused(got, want, cap, r"count = \d+ is not clamped to cap")


def test_compare_refuses_a_row_written_at_count_when_the_buffer_was_full():
    _, _, cap, _, want, got = _good(capmode="full")
    got[0][cap], got[1][cap] = (1.0, 2.0), 1
    _refused(got, want, cap, rf"ex_xy written at position {cap} .*guard region")


def test_compare_refuses_one_element_written_in_the_guard_region():
    _, _, cap, _, want, got = _good()
    got[1][cap + cc.GUARD - 1] = 0
    _refused(got, want, cap, rf"ex_label written at position {cap + cc.GUARD - 1} .*guard region")
    _, _, cap, _, want, got = _good()
    got[0][int(want[2][0]) + 2, 1] = 0.5                  # ... and past the fill level inside the buffer
    _refused(got, want, cap, rf"ex_xy written at position {int(want[2][0]) + 2} .*free part")


def test_compare_refuses_prev_in_left_stale_for_an_env_that_is_no_hit():
    _, tr, cap, init, want, got = _good()
    stale = np.nonzero((init[3] != 0) & (want[3] == 0))[0]            # was in, is out now: no hit, yet prev_in must fall
    assert len(stale)
    got[3][stale[0]] = init[3][stale[0]]
    _refused(got, want, cap, rf"prev_in differs first at env {stale[0]}:")


def test_compare_refuses_a_frontier_row_that_reached_one_of_its_two_nodes_only():
    case = cc._case("M", 300, 8, "rand50", "ring", (2, 2), masks=cc.MASKS[2], nodes="two")
    tr, cap, _, want = cc.setup_frontier(case, np.random.default_rng(9))
    got = [a.copy() for a in want]
    cm.compare_nodes(got[0], got[1], got[2], want[0], want[1], want[2], cap)
    ok = ~cc.covered_by(tr, case["masks"][1])
    e = int(np.nonzero(ok & (tr["events"] & 63 != 0))[0][0])          # the first env that hits: two nodes p < q
    p, q = [b for b in range(6) if (tr["events"][e] >> b) & 1]
    k = int(want[2][q])
    c0 = k - cc.frontier_rows(tr, 1 << q, case["masks"][1], 4)[q]
    got[0][q, c0:k - 4], got[1][q, c0:k - 4] = want[0][q, c0 + 4:k], want[1][q, c0 + 4:k]      # node q lacks the env's 4 rows
    got[0][q, k - 4:k], got[1][q, k - 4:k] = cm.XY_SENTINEL, cm.LABEL_SENTINEL
    got[2][q] = k - 4
    with pytest.raises(AssertionError, match=rf"node {q}: count = {k - 4}, the model has {k}"):
        cm.compare_nodes(got[0], got[1], got[2], want[0], want[1], want[2], cap)
