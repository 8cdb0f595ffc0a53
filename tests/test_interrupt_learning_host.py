"""SPEC §12 interrupting learner, host side (no GPU): the header and every build carry SCG_STEP_INTERRUPT, the emulator of
tests/interrupt_learning_model.py rebuilds sco_step's G and n_k bit for bit when nothing is interrupted (both env order layouts,
every block size: the order and the per-block recomputation are right), its acting outputs agree with a step-by-step oracle
emulation of §11's rule, and the Python flag plumbing."""
import os

import numpy as np
import pytest

import sc_oracle
import interrupt_learning_model as ilm
from acting_emulator import oracle_emulator
from ref64 import env_order_layout
from skill_chaining_with_graphs_amd.core import EnvState
from util import HP, SCALE, copy_state, crossing_weights, entry_state, oracle_block, wide_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_python_carry_the_flag():
    src = open(os.path.join(ROOT, "include", "scg_abi.h")).read()
    assert "#define SCG_STEP_INTERRUPT 4u" in src
    assert "#define SCG_ABI_VERSION 5" in src
    from skill_chaining_with_graphs_amd import _lib
    from skill_chaining_with_graphs_amd.core import ScgContext
    assert _lib.STEP_INTERRUPT == 4 and _lib.STEP_LEARN == 1 and _lib.STEP_APPLY == 2
    flags = ScgContext._step_flags
    assert flags(None, True, True) == 3 and flags(None, False, True) == 0            # unchanged without interrupt
    assert flags(None, True, True, True) == 7 and flags(None, True, False, True) == 5
    assert flags(None, False, False, True) == 4                                      # passed on: the library refuses it


def test_every_build_holds_the_interrupting_step_kernel():
    from skill_chaining_with_graphs_amd import _lib
    for blk in _lib.BLOCK_ENVS_BUILDS:
        path = _lib.lib_path(blk)
        assert os.path.exists(path), f"{path} not built"
        assert b"_Z9td_kernelILi3EEv8StepArgs" in open(path, "rb").read(), path      # td_kernel<MODE_FUSED_INT>


def _case(name, n, n_opt, block, seed, run_share, gest=0, layout=None):
    """(The caller holds the oracle on the build for `block` while it uses what this returns: oracle_block(block); 256 is the default.)"""
    import skill_chaining_with_graphs_amd as scg
    m = scg.load_map(name)
    n_vf = n_opt + 1
    mask = ((1 << n_vf) - 1) & ~1 & ~gest
    orc = sc_oracle.Oracle(m, SCALE, n_envs=n, n_options=n_opt, seed=seed, enabled_mask=mask, n_threads=4, reoffer_period=4, **HP)
    if gest:
        orc.set_gestation(gest)
    st = entry_state(m, n, n_opt, seed, run_share, HP["max_episode_steps"])
    return orc, m, st, crossing_weights(n_vf, seed), wide_chain(m, n_opt), mask


CASES = [
    # map, envs, options, block, seed, share of envs running an option, gestating, layout
    ("pinball_simple", 2048, 3, 256, 1, 0.3, 0, "chunked"),
    ("pinball_simple", 1000, 5, 256, 2, 0.6, 0, "padded"),          # (full blocks <= runs)
    ("pinball_maze", 1536, 4, 128, 3, 0.5, 0b10000, "chunked"),     # a gestating option's off-policy items
    ("pinball_maze", 300, 5, 64, 4, 0.9, 0, "padded"),
    ("pinball_simple", 1200, 3, 64, 5, 0.25, 0, "chunked"),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-n{c[1]}-o{c[2]}-b{c[3]}")
def test_emulator_reproduces_sco_step_without_interrupts(case):
    with oracle_block(case[3]):
        orc, m, st, W, clf, mask = _case(*case)
        layout = env_order_layout(st["option_id"], orc.n_vf, case[3])
        assert layout == case[7]
        gest = case[6]
        plain = copy_state(st)
        G, n_k = orc.step(plain, W, clf, 11, mask)
        post, Ge, nke, info = ilm.step(orc, st, W, clf, 11, mask, gest=gest, interrupt=False, recompute=True)
        assert info["keep"].sum() > 0
        for f in EnvState.FIELDS:
            assert np.array_equal(post[f].view(np.uint8), plain[f].view(np.uint8)), f
        assert np.array_equal(nke, n_k)
        for k in range(orc.n_vf):
            assert n_k[k] > 0, k
            assert np.array_equal(Ge[k], G[k]), f"VF {k}: {np.sum(Ge[k] != G[k])} elements differ"


def test_emulator_acting_equals_a_step_by_step_oracle_emulation_of_section_11():
    """The emulator's interrupted envs, found from the physics and the classifiers, against §11's rule applied to sco_step's outputs
    the way the §11 tests do it (acting_emulator, v_option="qcache"): two derivations of each input of the rule.
      keep   option_rules.option_end on s' (ilm.step)       against  option_rules.kept_by_counters: opt_steps went up;
      V_o    sco_q_values of W_o at s_next (ilm.step)       against  the option's qcache as the plain step left it."""
    n, n_opt = 1500, 4
    orc, m, st, W, clf, mask = _case("pinball_simple", n, n_opt, 256, 7, 0.5)
    total = 0
    for t in range(30, 34):
        post, G, n_k, info = ilm.step(orc, st, W, clf, t, mask, interrupt=True, recompute=False)
        emu = oracle_emulator(orc, copy_state(st), W, clf, mask, interrupt=True, v_option="qcache")
        _, cut = emu.step(t)
        assert np.array_equal(info["keep"], emu.keep), f"t {t}: keep from the option's end and from the counters differ"
        assert np.array_equal(info["interrupted"], cut)
        for f in EnvState.FIELDS:
            assert np.array_equal(post[f].view(np.uint8), emu.st[f].view(np.uint8)), f"t {t}: {f}"
        total += int(cut.sum())
        st = post
    assert total > 0 and emu.kept > emu.interrupted > 0


def test_fmaf_is_fused():
    a, b, c = np.float32(1 + 2 ** -12), np.float32(1 - 2 ** -12), np.float32(-1)
    assert ilm.fmaf(a, b, c) == np.float32(-2.0 ** -24)        # a*b - 1 exactly; unfused it rounds to 0
