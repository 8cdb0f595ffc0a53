"""SPEC §14 value-ranked option choice, host side (no GPU): tests/option_rules.py's `choose` on hand-made cases (ties, NaN
values, stay, the fresh offer, the re-offer period, |C| <= 1 against §4.2), the sibling layout, the header and the binding of
scg_rollout_select, ScgContext.rollout's own refusals and EpisodeStats' optional `overrides`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import option_rules as rules
from util import SIBLING_PARENTS, sibling_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scg_abi.h")
NAN = np.float32("nan")


def _one(cset, values, v0, keep=False, done=0, oid=0, t=1, gid=0, period=4, n_vf=6):
    """choose() for one env: cset the members of C, values {k: V_k}."""
    Cm = np.zeros((n_vf, 1), bool)
    V = np.full((n_vf, 1), 1e30, np.float32)              # a value outside C must never be read: it would win
    for k in cset:
        Cm[k] = True
    for k, v in values.items():
        V[k] = v
    V[0] = v0
    ch = rules.choose(Cm, V, np.array([keep]), np.array([done]), np.array([oid]), t, np.array([gid], np.uint64), period)
    return {k: (v[0].item()) for k, v in ch.items()}


def test_highest_value_wins_and_ties_go_to_the_lowest():
    r = _one([1, 3, 4], {1: 1.0, 3: 2.0, 4: 1.5}, v0=0.0)
    assert r["offer"] and r["cstar"] == 3 and r["minc"] == 1 and not r["declined"] and r["override"] and r["option_id"] == 3 and r["vf"] == 3
    r = _one([2, 3, 5], {2: 2.0, 3: 2.0, 5: 2.0}, v0=2.0)      # all tie, and tie with the root: the lowest, and the gate holds
    assert r["cstar"] == 2 and not r["declined"] and not r["override"] and r["option_id"] == 2
    r = _one([2, 4], {2: 1.0, 4: 3.0}, v0=3.5)                 # the best still loses to the root: declined, staying out of c*
    assert r["cstar"] == 4 and r["declined"] and not r["override"] and r["option_id"] == -4 and r["vf"] == 0


def test_nan_values():
    r = _one([1, 2, 3], {1: NAN, 2: -5.0, 3: -7.0}, v0=-6.0)   # one NaN candidate is passed over
    assert r["cstar"] == 2 and not r["declined"] and r["override"]
    r = _one([2, 3], {2: NAN, 3: NAN}, v0=-1e9)                # all NaN: min C, and the gate declines it
    assert r["cstar"] == 2 and r["declined"] and r["option_id"] == -2 and r["vf"] == 0 and not r["override"]
    r = _one([2, 3], {2: 1.0, 3: 2.0}, v0=NAN)                 # a NaN root fails the gate, as in §4.2
    assert r["cstar"] == 3 and r["declined"] and r["option_id"] == -3


def test_stay_and_fresh_offer():
    vals = {1: 1.0, 3: 2.0, 4: 0.5}
    r = _one([1, 3, 4], vals, v0=0.0, oid=-4, t=1)             # stayed out of 4, still a candidate, not due: stays, id kept
    assert r["stay"] and not r["offer"] and r["option_id"] == -4 and r["vf"] == 0 and r["cstar"] == 0 and r["minc"] == 1
    r = _one([1, 3], vals, v0=0.0, oid=-4, t=1)                # 4 left C: a fresh offer at once
    assert not r["stay"] and r["offer"] and r["cstar"] == 3 and r["option_id"] == 3
    r = _one([1, 3, 4], vals, v0=0.0, oid=-4, t=1, done=2)     # a new episode is a new offer
    assert r["offer"] and r["option_id"] == 3
    r = _one([1, 3, 4], vals, v0=0.0, oid=-7, t=1)             # an id outside the options stays out of nothing
    assert r["offer"] and r["option_id"] == 3
    r = _one([1, 3, 4], vals, v0=0.0, oid=4, keep=True)        # a keeping env makes no choice
    assert not r["stay"] and not r["offer"] and r["option_id"] == 4 and r["vf"] == 4
    r = _one([], {}, v0=0.0, oid=-2)                           # no candidate: the root, id 0
    assert not r["stay"] and not r["offer"] and r["option_id"] == 0 and r["vf"] == 0


@pytest.mark.parametrize("period", [1, 4])
def test_reoffer_period(period):
    vals = {2: 1.0, 3: 2.0}
    for t in range(8):
        for gid in (0, 1, 6):
            r = _one([2, 3], vals, v0=5.0, oid=-3, t=t, gid=gid, period=period)
            due = (t + gid) % period == 0
            assert r["stay"] == (not due) and r["offer"] == due
            assert r["option_id"] == -3 and r["declined"] == due


def _spec42(cand, V, keep, done, oid, t, gid, period):
    """SPEC §4.2 for one step, from rules.candidates' cand: (option_id after the step, vf, declined, stay)."""
    idx = np.arange(len(cand))
    stay = ~keep & (cand >= 1) & (done == 0) & (oid == -cand) & (((t + gid) % period) != 0)
    offer = ~keep & (cand >= 1) & ~stay
    with np.errstate(invalid="ignore"):
        declined = offer & ~(V[cand, idx] >= V[0])
    o_keep = rules.vf_of(oid, V.shape[0])
    new = np.where(keep, oid, np.where(declined | stay, -cand, np.where(offer, cand, 0)))
    return new, np.where(keep, o_keep, np.where(offer & ~declined, cand, 0)), declined, stay


def test_at_most_one_candidate_is_spec_4_2():
    """Nested sets and chain parents: C never holds two options, and §14 is §4.2 (what the GPU tests' "chains unchanged" leans on)."""
    rng = np.random.default_rng(11)
    n, n_vf, parents, enabled = 4000, 6, [0, 0, 1, 2, 3, 4], 0b101110          # option 4 disabled
    depth = rng.integers(0, n_vf, n)                                           # in I_k for k >= depth (nested), none for 0
    in_n = np.zeros((n_vf, n), bool)
    for k in range(1, n_vf):
        in_n[k] = (depth >= 1) & (k >= depth)
    Cm = rules.candidate_mask(in_n, enabled, parents, n_vf)
    assert Cm.sum(axis=0).max() == 1
    cand = rules.min_c(Cm)
    assert np.array_equal(cand, np.where((depth >= 1) & (((enabled >> depth) & 1) == 1), depth, 0))   # in I_depth, not in I_(depth-1)
    V = rng.standard_normal((n_vf, n)).astype(np.float32)
    V[:, rng.random(n) < 0.05] = NAN
    V[1:, rng.random(n) < 0.2] = V[0, 0]
    keep = rng.random(n) < 0.3
    oid = np.where(keep, rng.integers(1, n_vf, n), -rng.integers(0, n_vf + 2, n)).astype(np.int64)
    done = rng.choice([0, 0, 0, 1, 2], n)
    gid = np.arange(n, dtype=np.uint64)
    for t in (0, 1, 2, 3):
        ch = rules.choose(Cm, V, keep, done, oid, t, gid, 4)
        new, vf, declined, stay = _spec42(cand, V, keep, done, oid, t, np.arange(n), 4)
        assert np.array_equal(ch["option_id"], new) and np.array_equal(ch["vf"], vf)
        assert np.array_equal(ch["declined"], declined) and np.array_equal(ch["stay"], stay)
        assert not ch["override"].any()
        assert stay.any() and declined.any() and (ch["offer"] & ~declined).any()


def test_candidate_mask_generalises_ilm_candidates():
    """candidate_mask / min_c against §4.2 written out per env: ascending k; enabled, in the set, not in the parent's region."""
    rng = np.random.default_rng(3)
    n, n_vf = 5000, 6
    in_n = rng.random((n_vf, n)) < 0.5
    in_n[0] = False
    for enabled in (0b111110, 0b101010, 0b000100):
        Cm = rules.candidate_mask(in_n, enabled, SIBLING_PARENTS, n_vf)
        assert not Cm[0].any()
        want_c, want_C = np.zeros(n, np.int64), np.zeros((n_vf, n), bool)
        for i in range(n):
            for k in range(1, n_vf):
                p = SIBLING_PARENTS[k]
                if (enabled >> k) & 1 and in_n[k, i] and not (p != 0 and in_n[p, i]):
                    want_C[k, i] = True
                    if want_c[i] == 0:
                        want_c[i] = k
        assert np.array_equal(Cm, want_C)
        assert np.array_equal(rules.min_c(Cm), want_c) and np.array_equal(rules.candidates(in_n, enabled, SIBLING_PARENTS, n_vf), want_c)
    assert (rules.candidate_mask(in_n, 0b111110, SIBLING_PARENTS, n_vf).sum(axis=0) >= 2).mean() > 0.3


@pytest.mark.parametrize("name", ["pinball_simple", "pinball_empty"])
def test_sibling_tree_gives_most_states_several_candidates(name):
    """The layout's point: on the oracle's classifier most random states have two or more candidates."""
    import skill_chaining_with_graphs_amd as scg
    from util import make_oracle, random_states
    orc, m = make_oracle(name, n_envs=1, n_options=5)
    parents, clf = sibling_tree(m)
    assert parents == [0, 0, 0, 1, 1, 2] and clf.shape == (6, 8) and not clf[0].any()
    x, y, _, _ = random_states(m, 2048, 7, vmax=1.5)
    in_n = rules.membership(lambda px, py, k: orc.classifier_predict(px, py, clf[k]), x, y, 6, 0b111110)
    Cm = rules.candidate_mask(in_n, 0b111110, parents, 6)
    assert (Cm.sum(axis=0) >= 2).mean() >= 0.5


def test_header_declares_and_binding_binds_the_entry_point():
    """Fails without the feature: the header, the binding and every build carry scg_rollout_select and its two rules."""
    from skill_chaining_with_graphs_amd import _lib
    src = open(HEADER).read()
    assert "#define SCG_ABI_VERSION 5" in src
    assert re.search(r"#define\s+SCG_SELECT_INTERRUPT\s+1u", src) and re.search(r"#define\s+SCG_SELECT_BEST\s+2u", src)
    decl = re.search(r"int\s+scg_rollout_select\s*\(([^;]*)\);", src).group(1)
    args = [a.strip() for a in decl.replace("\n", " ").split(",")]
    intr = re.search(r"int\s+scg_rollout_interrupt\s*\(([^;]*)\);", src).group(1)
    args_i = [a.strip() for a in intr.replace("\n", " ").split(",")]
    # scg_rollout_interrupt's arguments plus `overrides` (after interrupts) and `rules` (before the stream)
    assert [a for a in args if a not in ("int32_t *overrides", "uint32_t rules")] == args_i
    assert args.index("int32_t *overrides") == args.index("int32_t *interrupts") + 1 and args[-2:] == ["uint32_t rules", "void *stream"]
    assert (_lib.SELECT_INTERRUPT, _lib.SELECT_BEST) == (1, 2)
    assert "scg_rollout_select" in _lib.EXPORTED_SYMBOLS
    res, sig = _lib._SIGS["scg_rollout_select"]
    assert res is C.c_int and len(sig) == len(args) and sig[-2] is C.c_uint32
    assert sig[:-5] == _lib._SIGS["scg_rollout_interrupt"][1][:-3]
    for blk in _lib.BLOCK_ENVS_BUILDS:
        path = _lib.lib_path(blk)
        assert os.path.exists(path), f"{path} not built"
        assert hasattr(C.CDLL(path), "scg_rollout_select"), path


def test_null_ctx_and_unknown_rules_are_refused_without_a_device():
    from skill_chaining_with_graphs_amd import _lib
    lib = _lib.load(256)
    p = C.c_void_p(torch.zeros(64).data_ptr())
    for rules in (0, _lib.SELECT_BEST, _lib.SELECT_BEST | _lib.SELECT_INTERRUPT, 4, 0x80000000):
        args = [p] * 13 + [C.c_uint32(0b10), C.c_uint64(0), C.c_int32(2), C.c_uint32(0), None, None, None, None,
                           C.c_uint32(rules), None]
        assert lib.scg_rollout_select(None, *args) == -1
        assert lib.scg_last_error(None).decode() == "scg_rollout_select: null ctx"


def test_rollout_checks_choose_before_the_library():
    from skill_chaining_with_graphs_amd import ScgError
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
    from test_interrupt_host import _StubCtx, _operands
    n, n_vf = 8, 3
    ctx = _StubCtx(n, n_vf)
    st, W, clf = _operands(n, n_vf)
    stats = EpisodeStats(n_vf, n)
    for bad in ("best", "", 1, True):
        with pytest.raises(ValueError):
            ctx.rollout(st, W, clf, 0b110, 0, 2, stats, choose=bad)
    with pytest.raises(ScgError):                                               # overrides belong to a value-ranking rollout
        ctx.rollout(st, W, clf, 0b110, 0, 2, stats, overrides=torch.zeros(n_vf * n, dtype=torch.int32))
    with pytest.raises(ScgError):
        ctx.rollout(st, W, clf, 0b110, 0, 2, stats, choose="value", overrides=torch.zeros(n_vf * n, dtype=torch.int64))
    assert stats.overrides is None
    for kw, name in ((dict(), "scg_rollout"), (dict(interrupt=True), "scg_rollout_interrupt"),
                     (dict(begin_at=True), "scg_rollout_record"), (dict(choose="value"), "scg_rollout_select"),
                     (dict(choose="value", interrupt=True), "scg_rollout_select")):
        with pytest.raises(AssertionError, match=f"library was called: {name}$"):   # existing paths keep their entry points
            ctx.rollout(st, W, clf, 0b110, 0, 2, stats, **kw)
    assert stats.overrides is not None and stats.overrides.shape == (n_vf, n)


def test_episode_stats_overrides_only_when_asked_for():
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats
    s = EpisodeStats(3, 4)
    plain = s.summary()
    assert "overrides" not in plain and "overrides" not in s.per_env() and s.overrides is None
    ov = s.want_overrides()
    assert ov is s.want_overrides() and ov.dtype == torch.int32 and ov.shape == (3, 4) and int(ov.sum()) == 0
    ov.copy_(torch.tensor([[0, 0, 0, 0], [1, 0, 2, 0], [0, 4, 0, 0]], dtype=torch.int32))
    r = s.summary()
    assert list(r) == list(plain) + ["overrides"] and r["overrides"] == [0, 3, 4]
    assert list(s.per_env()) == list(EpisodeStats.FIELDS) + ["overrides"]
    s.zero_()
    assert s.overrides is None and "overrides" not in s.summary()
