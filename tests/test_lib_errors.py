"""_lib.check reads a failure's text from the library that made the call (no GPU: both refusals below come before scg_create looks
for a device). A refused scg_create has no context to hold its text: it lies in a thread_local of the library that refused, and
each of the three block builds has its own."""
import ctypes as C

import pytest


def _refused_create(lib, **kw):
    from skill_chaining_with_graphs_amd._lib import ScgConfig
    ctx = C.c_void_p()
    cfg = dict(n_envs=4, n_options=0, fourier_order=5, device=0)
    cfg.update(kw)
    rc = lib.scg_create(C.byref(ctx), C.byref(ScgConfig(**cfg)))
    assert rc == -1 and not ctx.value
    return rc


@pytest.mark.parametrize("block", [64, 128, 256])
def test_check_reports_the_refusing_builds_own_text(block):
    from skill_chaining_with_graphs_amd import _lib
    _refused_create(_lib.load(256), reoffer_period=3)            # an earlier failure on the default build: its text stays there
    assert b"reoffer_period" in _lib.load(256).scg_last_error(None)
    lib = _lib.load(block)
    rc = _refused_create(lib, n_envs=0)
    with pytest.raises(_lib.ScgError) as e:
        _lib.check(rc, None, "scg_create", lib)
    text = str(e.value)
    assert "n_envs must be >= 1" in text and "reoffer_period" not in text, text
    assert text.startswith("scg_create failed (") and lib.scg_strerror(rc).decode() in text
