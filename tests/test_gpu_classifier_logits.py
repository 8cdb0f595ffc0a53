"""SPEC §24.2 on the GPU (scg_classifier_logits): z is the value whose sign scg_classifier_predict tests. (z > 0) equals the
prediction of the HIP path and of the oracle exactly, on every input, NaN included; on finite inputs z lies within
tests/ref64.py::clf_model's binary32 bound of the float64 value; the refusals are scg_classifier_predict's in its sequence and
a refused call, or n = 0, writes nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import skill_chaining_with_graphs_amd as scg
from skill_chaining_with_graphs_amd._lib import ScgError
from gpu_util import as_bytes, dev, make_pair
from ref64 import clf_model
from util import disc_weights

pytestmark = pytest.mark.gpu

CX, CY, R = 0.6, 0.45, 0.3
GUARD, PAD = -777.25, 64


@pytest.fixture(scope="module")
def pair():
    ctx, orc, m = make_pair("pinball_simple", 64)
    yield ctx, orc
    ctx.close()


def _rows():
    disc = disc_weights(CX, CY, R)
    mixed = disc.copy()
    mixed[1], mixed[4] = np.float32(2.0 ** 100), np.float32(2.0 ** -140)        # a huge and a subnormal weight in one row
    assert 0 < mixed[4] < np.finfo(np.float32).tiny
    rng = np.random.default_rng(4)
    return {"disc": disc, "zeros": np.zeros(8, np.float32), "huge and subnormal": mixed,
            "random": np.r_[rng.standard_normal(6), 0, 0].astype(np.float32)}


def _points():
    rng = np.random.default_rng(5)
    rnd = rng.random((4096, 2)).astype(np.float32)
    a = np.linspace(0.0, 2 * np.pi, 86, endpoint=False)
    bx, by = (CX + R * np.cos(a)).astype(np.float32), (CY + R * np.sin(a)).astype(np.float32)       # on the disc's boundary ...
    rim_x = np.concatenate([bx, np.nextafter(bx, np.float32(2)), np.nextafter(bx, np.float32(-2))])   # ... and next to it, both ways
    rim_y = np.concatenate([by, by, by])
    bad = np.array([[np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [-np.inf, 0.5], [0.5, np.inf], [0.5, -np.inf], [np.inf, -np.inf],
                    [np.nan, np.nan]], np.float32)
    return {"random 4096": (rnd[:, 0].copy(), rnd[:, 1].copy()), "rim 258": (rim_x, rim_y), "non-finite": (bad[:, 0].copy(), bad[:, 1].copy()),
            "n = 1": (rnd[:1, 0].copy(), rnd[:1, 1].copy()), "n = 257": (rnd[:257, 0].copy(), rnd[:257, 1].copy())}


@pytest.mark.parametrize("row", list(_rows()))
def test_logits_sign_is_the_prediction_and_the_value_is_within_the_bound(pair, row):
    ctx, orc = pair
    w8 = _rows()[row]
    for name, (x, y) in _points().items():
        z = ctx.classifier_logits(dev(x), dev(y), dev(w8)).cpu().numpy()
        pred = ctx.classifier_predict(dev(x), dev(y), dev(w8)).cpu().numpy()
        assert z.dtype == np.float32 and z.shape == x.shape
        assert np.array_equal(z > 0, pred != 0), f"{row} / {name}: (z > 0) differs from scg_classifier_predict"
        assert np.array_equal(z > 0, orc.classifier_predict(x.copy(), y.copy(), w8) != 0), f"{row} / {name}: ... from the oracle"
        fin = np.isfinite(x) & np.isfinite(y)
        z64, tol = clf_model(w8, x[fin], y[fin])
        err = np.abs(z[fin].astype(np.float64) - z64)
        print(f"{row} / {name}: n {x.size}, inside {int((z > 0).sum())}, max |z - z64| / bound "
              f"{float(np.max(err / np.where(tol > 0, tol, 1.0))) if fin.any() else 0.0:.3f}")
        assert np.all(np.isfinite(z[fin])) and np.all(err <= tol), f"{row} / {name}: z leaves clf_model's bound"
        if name == "non-finite" and row == "disc":
            assert not (z > 0).any() and np.isnan(z).any()
    if row == "disc":                                             # the cases bite: both sides of the rim are met, one ulp apart
        x, y = _points()["rim 258"]
        z = ctx.classifier_logits(dev(x), dev(y), dev(w8)).cpu().numpy()
        assert 0 < int((z > 0).sum()) < z.size and len({tuple(r) for r in (z.reshape(3, -1) > 0).T.tolist()}) > 1
    if row == "zeros":
        x, y = _points()["random 4096"]
        z = ctx.classifier_logits(dev(x), dev(y), dev(w8)).cpu().numpy()
        assert np.array_equal(as_bytes(z), as_bytes(np.zeros_like(z)))            # +0 everywhere: the empty set


def test_refusals_in_their_sequence_and_the_write_set(pair):
    ctx, _ = pair
    lib = ctx.lib
    n = 257
    x, y, w8 = dev(np.full(n, 0.6, np.float32)), dev(np.full(n, 0.45, np.float32)), dev(disc_weights(CX, CY, R))
    buf = torch.full((PAD + n + PAD,), GUARD, dtype=torch.float32, device=ctx.device)
    z = buf[PAD:PAD + n]
    before = [t.clone() for t in (x, y, w8)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(c, n_, x_, y_, w_, z_):
        rc = lib.scg_classifier_logits(c, C.c_int32(n_), p(x_), p(y_), p(w_), p(z_), ctx._stream())
        return rc, lib.scg_last_error(c).decode()

    rc, msg = call(None, -1, None, None, None, None)               # the null ctx comes before the arguments
    assert rc == -1 and msg == "scg_classifier_logits: null ctx"
    for args in ((-1, x, y, w8, z), (n, None, y, w8, z), (n, x, None, w8, z), (n, x, y, None, z), (n, x, y, w8, None), (0, None, y, w8, z)):
        rc, msg = call(ctx._ctx, *args)
        assert rc == -1 and msg == "scg_classifier_logits: bad argument", msg
    lib.scg_debug_raise_async(ctx._ctx, C.c_uint32(0x1 | (0x100 << 2)))          # an earlier launch's failure: behind the arguments ...
    try:
        rc, msg = call(ctx._ctx, n, None, y, w8, z)
        assert rc == -1 and msg == "scg_classifier_logits: bad argument", msg
        rc, msg = call(ctx._ctx, n, x, y, w8, z)                                 # ... and before any launch, n = 0 included
        assert rc == -5, msg
        assert call(ctx._ctx, 0, x, y, w8, z)[0] == -5
        with pytest.raises(ScgError, match="earlier launch failed"):
            ctx.classifier_logits(x, y, w8)
    finally:
        ctx.clear_async_error()
    assert call(ctx._ctx, 0, x, y, w8, z)[0] == 0                               # n = 0 succeeds and writes nothing
    torch.cuda.synchronize()
    assert int((buf != GUARD).sum()) == 0, "a refused call, or n = 0, wrote z"
    assert ctx.classifier_logits(x[:0], y[:0], w8).numel() == 0
    assert call(ctx._ctx, n, x, y, w8, z)[0] == 0
    torch.cuda.synchronize()
    assert int((buf[:PAD] != GUARD).sum()) == 0 and int((buf[PAD + n:] != GUARD).sum()) == 0, "z was written outside its n entries"
    assert int((z == GUARD).sum()) == 0
    for t, b in zip((x, y, w8), before):
        assert np.array_equal(as_bytes(t), as_bytes(b)), "an input was written"
    for bad in ((x[:5], y, w8), (x, y, w8[:6]), (x.double(), y, w8), (x.cpu(), y, w8)):
        with pytest.raises(ScgError):
            ctx.classifier_logits(*bad)


def test_it_needs_no_map():
    """A context on which scg_set_map was never called (ScgContext always calls it: the library is driven directly)."""
    from skill_chaining_with_graphs_amd._lib import ScgConfig
    lib = scg.load_library()
    c = C.c_void_p()
    assert lib.scg_create(C.byref(c), C.byref(ScgConfig(n_envs=64, n_options=0, fourier_order=5, device=0))) == 0
    try:
        x = dev(np.linspace(0, 1, 33, dtype=np.float32))
        y, w8 = x.flip(0).contiguous(), dev(disc_weights(CX, CY, R))
        z = torch.full((33,), GUARD, dtype=torch.float32, device=x.device)
        out = torch.full((33,), 9, dtype=torch.uint8, device=x.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        assert lib.scg_classifier_logits(c, C.c_int32(33), p(x), p(y), p(w8), p(z), None) == 0, lib.scg_last_error(c)
        assert lib.scg_classifier_predict(c, C.c_int32(33), p(x), p(y), p(w8), p(out), None) == 0, lib.scg_last_error(c)
        torch.cuda.synchronize()
        assert np.array_equal(z.cpu().numpy() > 0, out.cpu().numpy() == 1) and 0 < int((z > 0).sum()) < 33
    finally:
        assert lib.scg_destroy(c) == 0
