"""CPU: the interface of the device plan of the lattice arc posteriors (amx_latpost_cfg.plan, amx_latpost_plan_dev, amx_latpost_plan_shape)
where no device is needed: the default, the option's values, the refusals of a handle without a context."""
import ctypes as C

import numpy as np
import pytest

from tests import latpost_reference as lr


def test_the_plan_defaults_to_the_host():
    from rasr_amd import _lib
    cfg = _lib.LatpostCfg(2, 0, 0, 7, 1)   # five positional values stay valid; the new field is the last
    assert cfg.plan == _lib.AMX_LATPOST_PLAN_HOST == 0 and _lib.AMX_LATPOST_PLAN_DEVICE == 1
    cfg.plan = 1
    _lib.lib().amx_latpost_cfg_default(C.byref(cfg))
    assert cfg.plan == _lib.AMX_LATPOST_PLAN_HOST


def test_the_option_takes_host_and_device_only():
    import rasr_amd
    rasr_amd.LatticePosterior(None, plan="device").close()
    with pytest.raises(ValueError, match="plan"):
        rasr_amd.LatticePosterior(None, plan="gpu")
    cfg = rasr_amd._lib.LatpostCfg(0, 1, 1, 100, 0, 7)
    with pytest.raises(rasr_amd.AmxError, match="plan 7"):
        rasr_amd._lib.check(rasr_amd._lib.lib().amx_latpost_create(None, C.byref(cfg), C.byref(C.c_void_p())))


@pytest.mark.parametrize("plan", ["host", "device"])
def test_plan_dev_without_a_context_checks_first(plan):
    import rasr_amd
    good = lr.small_cases()["diamond"]
    outside = dict(good, arc_target=np.array([1, 4, 3, 3], np.int32))
    lp = rasr_amd.LatticePosterior(None, plan=plan)
    with pytest.raises(rasr_amd.AmxError, match="segment 1: arc 1 of state 0 has target 4 outside its 4 states") as e:
        lp.plan_dev([good, outside, good])
    assert e.value.status == rasr_amd._lib.AMX_ERR_INVALID
    with pytest.raises(rasr_amd.AmxError, match="without a context") as e:
        lp.plan_dev([good])
    assert e.value.status == rasr_amd._lib.AMX_ERR_STATE
    lp.close()


def test_plan_shape_reports_the_switch_points():
    import rasr_amd
    shape = rasr_amd.LatticePosterior.plan_shape()
    assert set(shape) == {"threads", "lds_states", "lds_stack"} and all(v > 0 for v in shape.values())
    assert shape["threads"] % 64 == 0
