"""Bitwise comparison of binary32 arrays (SPEC preamble: the two sides agree bit for bit, floats included).

`np.array_equal` calls -0.0 and +0.0 equal and cannot hold a NaN; `assert_bits_equal` compares the uint32 views, so the sign
of a zero, every subnormal and the class of every Inf / NaN count. The one exception, under `allow_nan=True`: a NaN matches
a NaN of any sign and payload (x86 and gfx950 produce different default NaNs, and the SPEC pins no payload)."""
import numpy as np

_EXP, _MAN, _ABS = np.uint32(0x7F800000), np.uint32(0x007FFFFF), np.uint32(0x7FFFFFFF)

CLASSES = ("zero sign", "flushed", "Inf/NaN", "other")


def _u32(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, f"binary32 expected, got {a.dtype}"
    return a.view(np.uint32)


def is_subnormal(a):
    u = _u32(a)
    return ((u & _EXP) == 0) & ((u & _MAN) != 0)


def is_neg_zero(a):
    return _u32(a) == np.uint32(0x80000000)


def classify(got, want, allow_nan=False):
    """(mismatch mask, class index per element: 0 zero sign, 1 flushed, 2 Inf/NaN class, 3 other; -1 where equal)."""
    g, w = _u32(got), _u32(want)
    assert g.shape == w.shape, f"shapes differ: {g.shape} against {w.shape}"
    bad = g != w
    g_nan, w_nan = (g & _ABS) > _EXP, (w & _ABS) > _EXP
    if allow_nan:
        bad &= ~(g_nan & w_nan)
    g_zero, w_zero = (g & _ABS) == 0, (w & _ABS) == 0
    g_sub, w_sub = ((g & _EXP) == 0) & ~g_zero, ((w & _EXP) == 0) & ~w_zero
    g_nf, w_nf = (g & _EXP) == _EXP, (w & _EXP) == _EXP
    cls = np.full(g.shape, 3, np.int8)
    cls[g_nf | w_nf] = 2
    cls[(g_sub & w_zero) | (g_zero & w_sub)] = 1
    cls[g_zero & w_zero] = 0
    cls[~bad] = -1
    return bad, cls


def assert_bits_equal(got, want, allow_nan=False, msg=""):
    bad, cls = classify(got, want, allow_nan)
    if not bad.any():
        return
    counts = ", ".join(f"{name}: {int(np.sum(cls == i))}" for i, name in enumerate(CLASSES))
    idx = np.argwhere(bad)[:5]
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    first = "; ".join(f"{tuple(int(v) for v in i)}: got {float(g[tuple(i)])!r} (0x{int(g.view(np.uint32)[tuple(i)]):08x}) "
                      f"want {float(w[tuple(i)])!r} (0x{int(w.view(np.uint32)[tuple(i)]):08x})" for i in idx)
    raise AssertionError(f"{msg} {int(bad.sum())} of {bad.size} binary32 values differ by bits ({counts}); first {first}")
