"""SPEC §21 population rollouts, host side (no GPU): the header and the binding of scg_rollout_population; paired_differences against
a plain float64 restatement; damped_tables at lambda = 0, 1 and between; improve_policy's decision rule (valuefit.choose_candidate)
on hand-made candidate tables; EpisodeStats over an env range; and the shape refusals of rollout(population=) and
evaluate_policies that are reached before any device call."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scg_abi.h")


# ---------------------------------------------------------------------------------------------------- header, binding, exports

def _declaration(name):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in include/scg_abi.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_entry_point_and_the_binding_matches(pkg):
    from skill_chaining_with_graphs_amd import _lib
    pop, branch = _declaration("scg_rollout_population"), _declaration("scg_rollout_branch")
    assert pop[:-1] == branch and pop[-1] == "const scg_population *pop"       # scg_rollout_branch's arguments in its order, then pop
    res, args = _lib._SIGS["scg_rollout_population"]
    _, b_args = _lib._SIGS["scg_rollout_branch"]
    assert res is C.c_int and args[:-1] == b_args and args[-1] is C.POINTER(_lib.Population)
    text = open(HEADER).read()
    assert re.search(r"#define\s+SCG_POP_MAX\s+64\b", text) and _lib.POP_MAX == 64
    m = re.search(r"typedef struct \{([^}]*)\} scg_population;", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    members = [" ".join(v.split()) for v in m.group(1).split(";") if v.strip()]
    assert members == ["int32_t n_policies", "int32_t n_per", "const float *epsilon", "const uint32_t *enabled"]
    assert [f for f, _ in _lib.Population._fields_] == ["n_policies", "n_per", "epsilon", "enabled"]
    assert C.sizeof(_lib.Population) == 24
    assert "scg_rollout_population" in pkg.EXPORTED_SYMBOLS and _lib.ABI_VERSION == 5


def test_every_build_exports_it_and_refuses_a_null_ctx(pkg):
    from skill_chaining_with_graphs_amd import _lib
    for b in _lib.BLOCK_ENVS_BUILDS:
        lib = _lib.load(b)
        _, args = _lib._SIGS["scg_rollout_population"]
        zeros = [None if (a is C.c_void_p or hasattr(a, "contents")) else a(0) for a in args]
        assert lib.scg_rollout_population(*zeros) == -1
        assert lib.scg_last_error(None) == b"scg_rollout_population: null ctx"


# ---------------------------------------------------------------------------------------------------- paired_differences

def _per_env(rng, n):
    return {"ret_sum": rng.normal(-50, 30, n), "disc_final": rng.normal(-20, 10, n).astype(np.float32),
            "goals": rng.integers(0, 2, n).astype(np.int32), "len_sum": rng.integers(1, 200, n).astype(np.int32),
            "episodes": np.ones(n, np.int32)}


def test_paired_differences_against_a_plain_restatement(pkg):
    from skill_chaining_with_graphs_amd.evaluation import paired_differences
    rng = np.random.default_rng(0)
    for n in (2, 3, 257):
        a, b = _per_env(rng, n), _per_env(rng, n)
        got = paired_differences({f: torch.from_numpy(v) for f, v in a.items()}, b)       # tensors and arrays alike
        assert set(got) == {"ret", "disc_final", "goal", "steps"}
        for name, f in (("ret", "ret_sum"), ("disc_final", "disc_final"), ("goal", "goals"), ("steps", "len_sum")):
            d = [float(x) - float(y) for x, y in zip(a[f], b[f])]
            mean = math.fsum(d) / n
            se = math.sqrt(math.fsum((v - mean) ** 2 for v in d) / (n - 1)) / math.sqrt(n)
            assert got[name]["n"] == n
            assert abs(got[name]["mean_diff"] - mean) <= 1e-12 * max(1.0, abs(mean)) * n
            assert abs(got[name]["se"] - se) <= 1e-12 * max(1.0, se) * n
    same = paired_differences(a, {f: v.copy() for f, v in a.items()})
    assert all(r == {"mean_diff": 0.0, "se": 0.0, "n": 257} for r in same.values())     # equal inputs: exact zeros
    one = paired_differences(_per_env(rng, 1), _per_env(rng, 1))
    assert all(r["se"] == 0.0 and r["n"] == 1 and r["mean_diff"] != 0.0 for n_, r in one.items() if n_ != "goal")
    with pytest.raises(ValueError):
        paired_differences(a, _per_env(rng, 5))
    with pytest.raises(ValueError, match="disc_final"):
        paired_differences({f: v for f, v in a.items() if f != "disc_final"}, a)


def test_episode_stats_over_an_env_range(pkg):
    from skill_chaining_with_graphs_amd.evaluation import EpisodeStats, GateAudit
    rng = np.random.default_rng(1)
    n, n_vf, lo, hi = 10, 3, 4, 9
    whole, part = EpisodeStats(n_vf, n), EpisodeStats(n_vf, hi - lo)
    whole.audit, part.audit = GateAudit(n), GateAudit(hi - lo)
    whole.interrupting = part.interrupting = True
    whole.want_overrides(); part.want_overrides()
    for f in EpisodeStats.FIELDS + ("interrupts", "overrides"):
        t = getattr(whole, f)
        t.copy_(torch.from_numpy(rng.integers(0, 9, tuple(t.shape))).to(t.dtype))
        getattr(part, f).copy_(t[..., lo:hi])
    whole.audit.disc_final.copy_(torch.from_numpy(rng.normal(size=n).astype(np.float32)))
    part.audit.disc_final.copy_(whole.audit.disc_final[lo:hi])
    assert whole.summary(lo, hi) == part.summary()
    got, want = whole.per_env(lo, hi), part.per_env()
    assert list(got) == list(want) and all(torch.equal(got[f], want[f]) for f in want)
    assert whole.summary() == whole.summary(0, n) and all(v is getattr(whole, f) for f, v in whole.per_env().items() if f in EpisodeStats.FIELDS)
    with pytest.raises(ValueError):
        whole.summary(3, n + 1)


# ---------------------------------------------------------------------------------------------------- damped_tables

def test_damped_tables(pkg):
    from skill_chaining_with_graphs_amd.valuefit import damped_tables
    rng = np.random.default_rng(2)
    W = rng.normal(size=(2, 5, 7)).astype(np.float32)
    Wn = (W + rng.normal(size=W.shape) * 0.1).astype(np.float32)
    # pairs more than 2^30 apart in magnitude: the float64 difference is inexact, W + 1 * (W_new - W) is not W_new
    W[0, 0, :4] = [1.0e10, -3.0e12, 1.2345678e-7, 7.0e-12]
    Wn[0, 0, :4] = [1.2345678e-5, 9.87654e-3, -4.0e9, 2.5e8]
    wide = W.astype(np.float64) + (Wn.astype(np.float64) - W.astype(np.float64))
    assert not np.array_equal(wide.astype(np.float32).view(np.uint32), Wn.view(np.uint32)), "the wide pairs do not exercise lambda = 1"
    lam = (0.0, 0.25, 0.5, 1.0)
    out = damped_tables(W, Wn, lam)
    assert out.shape == (4,) + W.shape and out.dtype == np.float32
    assert np.array_equal(out[0].view(np.uint32), W.view(np.uint32)) and np.array_equal(out[3].view(np.uint32), Wn.view(np.uint32))
    for i in (1, 2):
        want = (W.astype(np.float64) + lam[i] * (Wn.astype(np.float64) - W.astype(np.float64))).astype(np.float32)
        assert np.array_equal(out[i].view(np.uint32), want.view(np.uint32))
    t = damped_tables(torch.from_numpy(W), torch.from_numpy(Wn), lam)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy().view(np.uint32), out.view(np.uint32))
    assert damped_tables(W, Wn, ()).shape == (0,) + W.shape
    with pytest.raises(ValueError):
        damped_tables(W, Wn[:1], lam)


# ---------------------------------------------------------------------------------------------------- the decision rule

def _cand(lam, disc, ret, succ, diff, se):
    """A candidate whose three means are given and whose paired rows all hold (diff, se)."""
    return {"lambda": lam, "summary": {"mean_discounted_return": disc, "mean_return": ret, "success_rate": succ},
            "paired": {k: {"mean_diff": diff, "se": se, "n": 100} for k in ("disc_final", "ret", "goal", "steps")}}


def test_the_decision_rule(pkg):
    from skill_chaining_with_graphs_amd.valuefit import choose_candidate
    base = _cand(0.0, -10.0, -100.0, 0.5, 0.0, 0.0)
    # accept: the best mean, and its paired difference beyond z standard errors
    c = [base, _cand(0.25, -9.0, -90.0, 0.6, 1.0, 0.4), _cand(0.5, -8.0, -95.0, 0.55, 2.0, 0.9), _cand(1.0, -12.0, -80.0, 0.7, -2.0, 0.5)]
    assert choose_candidate(c, "discounted", 2.0) == {"index": 2, "chosen_lambda": 0.5, "accepted": True}
    # keep: the same candidate below z * se (2.0 <= 2.5 * 0.9), and exactly at it (strictly beyond is asked)
    assert choose_candidate(c, "discounted", 2.5) == {"index": 2, "chosen_lambda": 0.0, "accepted": False}
    c[2]["paired"]["disc_final"]["se"] = 1.0
    assert choose_candidate(c, "discounted", 2.0) == {"index": 2, "chosen_lambda": 0.0, "accepted": False}
    # each criterion reads its own mean and its own paired row
    c[3]["paired"]["ret"] = {"mean_diff": 20.0, "se": 1.0, "n": 100}
    assert choose_candidate(c, "return", 2.0) == {"index": 3, "chosen_lambda": 1.0, "accepted": True}
    c[3]["paired"]["goal"] = {"mean_diff": 0.2, "se": 0.15, "n": 100}
    assert choose_candidate(c, "success", 2.0) == {"index": 3, "chosen_lambda": 0.0, "accepted": False}
    assert choose_candidate(c, "success", 1.0) == {"index": 3, "chosen_lambda": 1.0, "accepted": True}
    # ties go to the smallest lambda, whatever the order of the rows; the current policy wins a tie against every candidate
    tie = [_cand(1.0, -8.0, 0.0, 0.0, 2.0, 0.1), _cand(0.25, -8.0, 0.0, 0.0, 2.0, 0.1), _cand(0.5, -8.0, 0.0, 0.0, 2.0, 0.1)]
    assert choose_candidate(tie, "discounted", 2.0) == {"index": 1, "chosen_lambda": 0.25, "accepted": True}
    assert choose_candidate([_cand(0.5, -10.0, 0.0, 0.0, 0.0, 0.0), base], "discounted", 0.0) == {"index": 1, "chosen_lambda": 0.0, "accepted": False}
    # the current policy the best: kept whatever z; a NaN mean never wins; z = -inf accepts any candidate that is picked
    assert choose_candidate([base, _cand(0.5, -11.0, 0.0, 0.0, -1.0, 0.1)], "discounted", -math.inf)["accepted"] is False
    nan = [base, _cand(0.5, float("nan"), 0.0, 0.0, 5.0, 0.1), _cand(1.0, -9.5, 0.0, 0.0, -0.5, 0.3)]
    assert choose_candidate(nan, "discounted", 2.0) == {"index": 2, "chosen_lambda": 0.0, "accepted": False}
    assert choose_candidate(nan, "discounted", -math.inf) == {"index": 2, "chosen_lambda": 1.0, "accepted": True}
    assert choose_candidate(nan, "discounted", math.inf)["accepted"] is False
    with pytest.raises(ValueError, match="criterion"):
        choose_candidate(c, "length", 2.0)


# ---------------------------------------------------------------------------------------------------- refusals before any device call

def test_rollout_population_shape_refusals(pkg):
    from skill_chaining_with_graphs_amd._lib import ScgError
    from skill_chaining_with_graphs_amd.core import ScgContext
    ctx = object.__new__(ScgContext)                              # a stand-in: the checks read these three only
    ctx.n_envs, ctx.n_vf, ctx.device = 120, 3, torch.device("cpu")
    W = torch.zeros((3, 3, 5, 1296))
    eps, en = torch.zeros(3), torch.zeros(3, dtype=torch.int32)
    pop = ctx._chk_population(W, (eps, en))
    assert (pop.n_policies, pop.n_per, pop.epsilon, pop.enabled) == (3, 40, eps.data_ptr(), en.data_ptr())
    none = ctx._chk_population(W, (None, None))
    assert (none.n_policies, none.n_per, none.epsilon, none.enabled) == (3, 40, None, None)
    for Wbad, p in ((W.view(-1), (eps, en)), (W[:, :2], (eps, en)), (torch.zeros((7, 3, 5, 1296)), (None, None)),       # 120 % 7
                    (torch.zeros((65, 3, 5, 1296)), (None, None)), (torch.zeros((0, 3, 5, 1296)), (None, None)),
                    (W, (eps[:2], en)), (W, (eps, en[:2])), (W, (eps.double(), en)), (W, (eps, en.to(torch.int64))), (W, (eps, en.float())),
                    (W, eps), (W, None), (W, (eps,)), (W.numpy(), (eps, en))):
        with pytest.raises(ScgError):
            ctx._chk_population(Wbad, p)


def test_evaluate_policies_refusals(pkg):
    from skill_chaining_with_graphs_amd.agent import SkillChainingAgent
    ag = object.__new__(SkillChainingAgent)                       # a stand-in: no context is made before the refusals
    ag.n_vf, ag.enabled_mask, ag.W = 3, 0b110, torch.zeros((3, 5, 1296))
    ag.ctx = types.SimpleNamespace(cfg=types.SimpleNamespace(max_episode_steps=100, seed=0))
    ag._start_states = None
    W = torch.zeros((3, 3, 5, 1296))
    for kw in (dict(W=torch.zeros((65, 3, 5, 1296))), dict(W=torch.zeros((0, 3, 5, 1296))), dict(W=W[:, :2]), dict(W=W.view(3, -1)),
               dict(W=[W[0], W[1][:2]]), dict(W=W, epsilons=[0.0, 0.1]), dict(W=W, enabled=[6, 6, 6, 6]), dict(W=W, baseline=3),
               dict(W=W, baseline=-1), dict(W=W, n_episodes=0), dict(W=W, steps_per_launch=0), dict(W=W, choose="best"),
               dict(W=torch.zeros((64, 3, 5, 1296)), n_episodes=2 ** 25)):              # 2^31 envs: one more than a context holds
        with pytest.raises(ValueError):
            ag.evaluate_policies(**kw)
