"""SPEC §20, host side (no GPU): the header and the binding of scg_feature_gram_targets; valuefit.ridge_solve_shared against
ridge_solve on the tiled system, bit for bit; valuefit.branch_targets against a plain loop; valuefit.greedy_table on hand-made
means and values."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scg_abi.h")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_header_binding_and_limit_agree(pkg):
    from skill_chaining_with_graphs_amd import _lib
    text = open(HEADER).read()
    assert int(re.search(r"#define\s+SCG_GRAM_MAX_TARGETS\s+(\d+)", text).group(1)) == _lib.GRAM_MAX_TARGETS == 16
    m = re.search(r"\bint\s+scg_feature_gram_targets\s*\((.*?)\)\s*;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["scg_ctx *ctx", "int64_t n", "const float *x", "const float *y", "const float *vx", "const float *vy",
                    "const float *Y", "int32_t n_tgt", "int32_t n_seg", "const int64_t *offsets", "float *A", "float *B", "void *stream"]
    res, sig = _lib._SIGS["scg_feature_gram_targets"]
    want = {"scg_ctx *ctx": C.c_void_p, "int64_t n": C.c_int64, "int32_t n_tgt": C.c_int32, "int32_t n_seg": C.c_int32}
    assert res is C.c_int and sig == [want.get(a, C.c_void_p) for a in args]
    assert "scg_feature_gram_targets" in pkg.EXPORTED_SYMBOLS
    lib = pkg.load_library()
    assert lib.scg_feature_gram_targets(None, 0, *([None] * 5), 5, 1, None, None, None, None) == -1
    assert b"scg_feature_gram_targets: null ctx" in lib.scg_last_error(None)


# ---------------------------------------------------------------------------------------------------- ridge_solve_shared

F = 40


def _system(seed, C_, n):
    rng = np.random.default_rng(seed)
    phi = rng.standard_normal((max(n, 1), F)).astype(np.float32)
    A = (phi.T @ phi).astype(np.float32)
    A = np.triu(A) + np.triu(A, 1).T
    B = rng.standard_normal((C_, F)).astype(np.float32) * 100
    scale = (1.0 / (1.0 + np.arange(F))).astype(np.float32)
    return A, B, scale


@pytest.mark.parametrize("n_rhs", [1, 5])
def test_ridge_solve_shared_is_ridge_solve_on_the_tiled_system_by_bits(pkg, n_rhs):
    from skill_chaining_with_graphs_amd.valuefit import ridge_solve, ridge_solve_shared
    for n in (7, 300):                                                # (7 < F: the ridge term alone makes it definite)
        A, B, scale = _system(n_rhs + n, n_rhs, n)
        got = ridge_solve_shared(A, B, n, 1e-3, scale)
        want = ridge_solve(np.repeat(A[None], n_rhs, axis=0), B, [n] * n_rhs, 1e-3, scale)
        assert got.dtype == np.float64 and got.shape == (n_rhs, F) and same_bits(got, want)
        assert np.abs(got).max() > 0
        # it solves the system: (A + Lambda) Delta = B to float64 accuracy
        Mx = A.astype(np.float64) + np.diag(1e-3 * n / scale.astype(np.float64) ** 2)
        assert np.allclose(got @ Mx, B, rtol=1e-8, atol=1e-8 * np.abs(B).max())
        # the upper triangle is not read, as in ridge_solve
        A2 = A.copy()
        A2[np.triu_indices(F, 1)] = 7.0
        assert same_bits(ridge_solve_shared(A2, B, n, 1e-3, scale), got)


def test_ridge_solve_shared_without_samples_is_exactly_zero(pkg):
    from skill_chaining_with_graphs_amd.valuefit import ridge_solve, ridge_solve_shared
    A, B, scale = _system(3, 5, 0)
    got = ridge_solve_shared(np.zeros_like(A), B, 0, 1e-3, scale)
    assert got.shape == (5, F) and not got.view(np.uint64).any()
    assert same_bits(got, ridge_solve(np.zeros((5, F, F), np.float32), B, [0] * 5, 1e-3, scale))


# ---------------------------------------------------------------------------------------------------- branch_targets

def _loop_targets(g, q):
    M, A, R = g.shape
    gbar, se2, D = np.zeros((M, A)), np.zeros((M, A)), np.zeros((A, M), np.float32)
    for i in range(M):
        for a in range(A):
            s = 0.0
            for r in range(R):                                        # in replicate order
                s = s + float(g[i, a, r])
            mean = s / R
            v = 0.0
            for r in range(R):
                d = float(g[i, a, r]) - mean
                v = v + d * d
            gbar[i, a] = mean
            se2[i, a] = v / (R - 1) / R if R > 1 else 0.0
            D[a, i] = np.float32(mean - float(q[i, a]))               # the float64 difference, rounded once
    return gbar, se2, D


@pytest.mark.parametrize("R", [1, 2, 8])
def test_branch_targets_against_a_plain_loop(pkg, R):
    from skill_chaining_with_graphs_amd.valuefit import branch_targets
    rng = np.random.default_rng(R)
    g = (rng.standard_normal((37, 5, R)) * np.array([1.0, 1e3, 1e-3, 1e4, 50.0])[None, :, None]).astype(np.float32)
    g[0, 0], g[1, 1] = 0.0, 1e4                                       # replicates that agree: variance exactly 0
    q = (g.astype(np.float64).mean(axis=2) + rng.standard_normal((37, 5)) * 10).astype(np.float32)
    gbar, se2, D = branch_targets(g, q)
    wb, ws, wd = _loop_targets(g, q)
    assert gbar.dtype == se2.dtype == np.float64 and D.dtype == np.float32 and D.shape == (5, 37) and D.flags["C_CONTIGUOUS"]
    assert same_bits(gbar, wb) and same_bits(se2, ws) and same_bits(D, wd)
    assert se2[0, 0] == 0.0 and se2[1, 1] == 0.0
    if R == 1:
        assert not se2.any() and same_bits(gbar, g[:, :, 0].astype(np.float64))
    else:
        assert (se2[2:] > 0).all()


def test_branch_targets_rounds_the_float64_difference_once(pkg):
    from skill_chaining_with_graphs_amd.valuefit import branch_targets
    # gbar = (1 + 2^-24 + 1) / 2 is not a binary32 number: rounding gbar first and subtracting in binary32 gives another D
    g = np.array([[[1.0, np.float32(1.0 + 2.0 ** -23)]]], np.float32)
    q = np.array([[-np.float32(2.0 ** -30)]], np.float32)
    gbar, se2, D = branch_targets(g, q)
    exact = (1.0 + 2.0 ** -24) + 2.0 ** -30                           # just above the tie between 1 and 1 + 2^-23
    assert gbar[0, 0] == 1.0 + 2.0 ** -24 and D[0, 0] == np.float32(exact) == np.float32(1.0 + 2.0 ** -23)
    assert np.float32(gbar[0, 0]) - q[0, 0] == np.float32(1.0)         # (ties-to-even takes gbar to 1.0 first, and 2^-30 is lost)
    with pytest.raises(ValueError):
        branch_targets(g, np.zeros((1, 2), np.float32))
    with pytest.raises(ValueError):
        branch_targets(np.zeros((3, 5, 0), np.float32), np.zeros((3, 5), np.float32))


# ---------------------------------------------------------------------------------------------------- greedy_table

def test_greedy_table_on_hand_made_values(pkg):
    from skill_chaining_with_graphs_amd.valuefit import greedy_table
    #                  a* (first max)      a_old (first max)     a_new (first max)
    gbar = np.array([[1.0, 5.0, 5.0],   # 1                       0 (tie 0 / 2 -> 0)     1 (tie 1 / 2 -> 1): gain 5 - 1 = 4
                     [3.0, 3.0, 0.0],   # 0 (tie -> 0)            1                      1: nothing changed, gain 0
                     [0.0, -1.0, 2.0],  # 2                       2                      0: gain 0 - 2 = -2
                     [7.0, 1.0, 1.0]])  # 0                       0                      0 (all equal -> 0): nothing changed
    q_old = np.array([[2.0, 1.0, 2.0], [0.0, 9.0, 1.0], [1.0, 1.0, 5.0], [4.0, 3.0, 3.0]], np.float32)
    q_new = np.array([[0.0, 3.0, 3.0], [0.0, 1.0, 0.5], [6.0, 1.0, 5.0], [1.0, 1.0, 1.0]], np.float32)
    t = greedy_table(gbar, q_old, q_new)
    assert t["n"] == 4
    assert t["agreement_old"] == 2 / 4                                # states 2 and 3
    assert t["agreement_new"] == 2 / 4                                # states 0 and 3
    assert t["changed"] == 2 / 4
    gain = np.array([4.0, 0.0, -2.0, 0.0])
    assert t["one_step_gain"] == gain.mean() == 0.5
    assert t["one_step_gain_se"] == pytest.approx(np.std(gain, ddof=1) / 2.0, rel=1e-15)
    same = greedy_table(gbar, q_old, q_old)                           # nothing changed anywhere: the gain is exactly 0
    assert same["changed"] == 0.0 and same["one_step_gain"] == 0.0 and same["one_step_gain_se"] == 0.0
    assert same["agreement_new"] == same["agreement_old"] == 0.5
    one = greedy_table(gbar[:1], q_old[:1], q_new[:1])
    assert one["n"] == 1 and one["one_step_gain"] == 4.0 and one["one_step_gain_se"] == 0.0
    none = greedy_table(gbar[:0], q_old[:0], q_new[:0])
    assert none["n"] == 0 and all(np.isnan(none[f]) for f in ("agreement_old", "agreement_new", "changed", "one_step_gain"))
