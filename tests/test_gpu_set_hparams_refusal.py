"""A refused scg_set_hparams changes nothing: not the library's settings, not ScgContext.cfg, and nothing that the next accepted
call sends. Through the C-ABI and through the façade, on a context that has stepped; against a twin that never saw the call."""
import pytest

import skill_chaining_with_graphs_amd as scg
from test_gpu_reconfigure import S1, assert_same, warm
from util import HP

pytestmark = pytest.mark.gpu

# every field differs from S1 (the context's current settings); only reoffer_period (or the floor) makes the call invalid
OTHER = dict(gamma=0.5, alpha=0.5, epsilon=0.9, r_option_success=7.0, max_episode_steps=9, max_option_steps=3,
             update_count_floor=11)
ORDER = ("gamma", "alpha", "epsilon", "r_option_success", "max_episode_steps", "max_option_steps", "update_count_floor",
         "reoffer_period")


def _refuse(ctx, via, **bad):
    hp = dict(OTHER, reoffer_period=4)
    hp.update(bad)
    assert all(hp[k] != S1[k] for k in OTHER)
    if via == "abi":
        assert ctx.lib.scg_set_hparams(ctx._ctx, *[hp[k] for k in ORDER]) == -1          # SCG_ERR_INVALID
    else:
        with pytest.raises(scg.ScgError):
            ctx.set_hparams(**hp)


@pytest.mark.parametrize("bad", [dict(reoffer_period=3), dict(reoffer_period=-1), dict(reoffer_period=6),
                                 dict(update_count_floor=-1)], ids=lambda b: "-".join(f"{k}{v}" for k, v in b.items()))
@pytest.mark.parametrize("via", ["abi", "facade"])
def test_a_refused_set_hparams_changes_nothing(via, bad):
    a, twin = warm(256), warm(256)
    before = bytes(a.ctx.cfg)
    _refuse(a.ctx, via, **bad)
    assert bytes(a.ctx.cfg) == before == bytes(twin.ctx.cfg)
    a.step(2)
    twin.step(2)
    assert_same(a, twin, f"the step after a refused call ({via})")
    a.ctx.set_hparams(epsilon=0.3)                         # the next accepted call sends none of the refused values along
    twin.ctx.set_hparams(epsilon=0.3)
    assert bytes(a.ctx.cfg) == bytes(twin.ctx.cfg)
    for k in OTHER:
        if k != "epsilon":
            assert getattr(a.ctx.cfg, k) == pytest.approx(S1[k], rel=1e-7), k
    a.step(3, interrupt=True)
    twin.step(3, interrupt=True)
    assert_same(a, twin, f"the step after the next accepted call ({via})")


def test_create_and_set_hparams_refuse_the_same_settings():
    """scg_create refused a negative count floor while scg_set_hparams clamped it to 0: both refuse now, as both refuse a
    re-offer period that is no power of two."""
    m = scg.load_map("pinball_simple")
    for bad in (dict(update_count_floor=-1), dict(reoffer_period=3), dict(reoffer_period=-4)):
        with pytest.raises(scg.ScgError):
            scg.ScgContext(64, 1, m, **dict(HP, **bad))
    ctx = scg.ScgContext(64, 1, m, **HP)
    for ok in (dict(update_count_floor=0), dict(update_count_floor=1 << 30), dict(reoffer_period=0), dict(reoffer_period=1 << 30)):
        ctx.set_hparams(**ok)
    with pytest.raises(scg.ScgError):
        ctx.set_hparams(no_such_setting=1)
