"""tests/bits.py rejects every kind of difference that np.array_equal lets through (or cannot hold), and names its class."""
import numpy as np
import pytest

from bits import assert_bits_equal, classify


def _base():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((4, 50)).astype(np.float32)
    a[0, 0], a[0, 1] = 0.0, -0.0
    a[1, 0], a[1, 1] = np.float32(1e-40), np.float32(-2 ** -149)
    a[2, 0], a[2, 1] = np.inf, -np.inf
    a[3, 0] = np.nan
    return a


def _nan(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# (index, replacement, class the report must name, what np.array_equal says of the pair)
MUTATIONS = [
    ((0, 0), np.float32(-0.0), "zero sign", True),
    ((0, 1), np.float32(0.0), "zero sign", True),
    ((1, 0), np.float32(0.0), "flushed", False),
    ((1, 1), np.float32(-0.0), "flushed", False),
    ((0, 0), np.float32(2 ** -149), "flushed", False),
    ((2, 0), -np.inf, "Inf/NaN", False),
    ((2, 1), np.float32(-3.4e38), "Inf/NaN", False),
    ((2, 2), np.float32(np.nan), "Inf/NaN", False),
    ((3, 0), np.float32(1.0), "Inf/NaN", False),
    ((1, 0), np.nextafter(np.float32(1e-40), np.float32(1)), "other", False),       # the next subnormal
    ((3, 3), None, "other", False),                     # one ulp of a normal number
]


@pytest.mark.parametrize("idx,value,cls,np_equal", MUTATIONS, ids=[f"{m[2]}-{i}" for i, m in enumerate(MUTATIONS)])
@pytest.mark.parametrize("allow_nan", [False, True])
def test_every_mutation_is_rejected_and_classified(idx, value, cls, np_equal, allow_nan):
    want = _base()                                       # holds one NaN, at (3, 0): equal bits, so it passes either way
    got = want.copy()
    assert_bits_equal(got, want, allow_nan=allow_nan)
    got[idx] = np.nextafter(want[idx], np.float32(9)) if value is None else value
    if np_equal:                                         # what the suite compared with until now does not see it
        fin = ~np.isnan(want)
        assert np.array_equal(got[fin], want[fin])
    with pytest.raises(AssertionError) as e:
        assert_bits_equal(got, want, allow_nan=allow_nan, msg="mutated")
    text = str(e.value)
    assert text.startswith("mutated 1 of 200") and f"{cls}: 1" in text and f"{idx}:" in text
    for other in ("zero sign", "flushed", "Inf/NaN", "other"):
        if other != cls:
            assert f"{other}: 0" in text
    bad, c = classify(got, want, allow_nan)
    assert bad.sum() == 1 and bad[idx] and c[idx] == ("zero sign", "flushed", "Inf/NaN", "other").index(cls)


def test_identical_arrays_pass_and_nan_payloads_only_under_allow_nan():
    a = _base()
    a[3, 0] = 2.0
    assert_bits_equal(a, a.copy())
    x86, gfx, neg, sig = _nan(0xFFC00000), _nan(0x7FC00000), _nan(0xFFFFFFFF), _nan(0x7F800001)
    want = a.copy(); want[3, 0] = x86
    for other in (gfx, neg, sig):
        got = a.copy(); got[3, 0] = other
        assert_bits_equal(got, want, allow_nan=True)
        with pytest.raises(AssertionError, match="Inf/NaN: 1"):
            assert_bits_equal(got, want)
    assert_bits_equal(want, want.copy())                 # the same NaN bits are equal bits
    got = a.copy(); got[3, 0] = np.inf                   # NaN against Inf, either way round, fails even under allow_nan
    with pytest.raises(AssertionError, match="Inf/NaN: 1"):
        assert_bits_equal(got, want, allow_nan=True)
    with pytest.raises(AssertionError, match="Inf/NaN: 1"):
        assert_bits_equal(want, got, allow_nan=True)


def test_counts_and_first_indices_are_reported():
    want = np.zeros(100, np.float32)
    got = want.copy()
    got[10:20] = -0.0
    got[30] = 1e-42
    got[40] = np.nan
    got[50] = 1.0
    with pytest.raises(AssertionError) as e:
        assert_bits_equal(got, want, allow_nan=True, msg="ctx")
    t = str(e.value)
    assert t.startswith("ctx 13 of 100") and "zero sign: 10" in t and "flushed: 1" in t and "Inf/NaN: 1" in t and "other: 1" in t
    assert "(10,)" in t and "(14,)" in t and "(15,)" not in t


def test_dtype_and_shape_are_checked():
    with pytest.raises(AssertionError):
        assert_bits_equal(np.zeros(3), np.zeros(3, np.float32))
    with pytest.raises(AssertionError):
        assert_bits_equal(np.zeros(3, np.float32), np.zeros(4, np.float32))
